"""Reference fixtures for patch dropout (FLIP) in the EVA towers: tests/golden/patch_dropout_<tag>.pt.

Runs the REFERENCE tower (oracle.ref_import: the reference tree, CPU, fp32) with its own PatchDropout (model/evaclip/transformer.py:144-185)
in training mode and every block in eval mode (no DropPath, no dropout), under a fixed seed, and records the kept patch indices, the output
tokens and the gradient digests of a weighted-sum backward.  Same recipe as oracle/make_golden.py:vit_fixture (weights, inputs, digests).
RoPE towers run with RoPE=1 (the only setting in which a RoPE tower with patch dropout runs there: rope.py:120-136 gathers the kept
positions' table rows); the plain tower (g/14, no RoPE) with RoPE=0, where PatchDropout returns the tokens alone.

    python tools/make_patch_dropout_golden.py          (needs the reference tree; writes under tests/golden/)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from oracle import ref_import  # noqa: E402
from oracle.make_golden import fill, grad_digest  # noqa: E402
from common import save_golden  # noqa: E402

DRAW_SEED = 1234      # torch.manual_seed right before the forward: the patch-dropout draw is the first random number the pass takes
INPUT_SEED = 77
CASES = [("evaclip02_base", 0.5, "b16_d2_p50"), ("evaclip01_giant", 0.5, "g14_d2_p50"), ("evaclip01_giant", 0.75, "g14_d2_p75")]


def fixture(vtype, prob, tag, depth=2):
    ns = ref_import.load()
    torch.manual_seed(0)
    m = ref_import.build_mico(vtype, depth=depth)
    fill(m)
    vis = m.vision_encoder.visual
    os.environ["RoPE"] = "1" if vis.rope is not None else "0"
    vis.patch_dropout = ns.ref_eva.PatchDropout(prob)
    vis.train()
    for blk in vis.blocks:
        blk.eval()
    keeps = []

    def tap(mod, inp, out):
        # the kept indices: returned with RoPE=1; recovered by matching the gathered rows otherwise (an exact gather of distinct rows)
        x_in = inp[0]
        x_out = out[0] if isinstance(out, tuple) else out
        rows = []
        for f in range(x_in.shape[0]):
            eq = (x_out[f, 1:, None, :] == x_in[f, None, 1:, :]).all(-1)
            assert bool((eq.sum(-1) == 1).all()), "kept tokens must match exactly one input patch"
            rows.append(eq.float().argmax(-1))
        idx = torch.stack(rows)
        if isinstance(out, tuple):
            assert torch.equal(out[1], idx)
        keeps.append(idx)

    h = vis.patch_dropout.register_forward_hook(tap)
    g = torch.Generator().manual_seed(INPUT_SEED)
    x = torch.randn((2, 3, 224, 224), generator=g)
    for p in m.parameters():
        p.requires_grad_(True)
    torch.manual_seed(DRAW_SEED)
    out = vis(x, return_all_features=True)
    h.remove()
    w = torch.randn(out.shape, generator=g) / out.numel() ** 0.5
    (out * w).sum().backward()
    names = ["patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "pos_embed", "norm.weight", "norm.bias"]
    for i in sorted({0, depth - 1}):
        for k, _ in vis.blocks[i].named_parameters():
            names.append(f"blocks.{i}.{k}")
    named = dict(vis.named_parameters())
    (keep,) = keeps
    fx = dict(
        keep=keep.clone(), out=out.detach().clone(),
        # per-row norms of the positional table's gradient: rows of patches no frame kept are exactly zero, the others carry their tokens'
        pos_grad_row_norm=named["pos_embed"].grad.detach()[0].norm(dim=-1).clone(),
        grads={n: grad_digest(named[n].grad) for n in names if named[n].grad is not None},
        meta=dict(vtype=vtype, depth=depth, prob=prob, input_seed=INPUT_SEED, draw_seed=DRAW_SEED, rope=vis.rope is not None),
    )
    save_golden(fx, f"patch_dropout_{tag}.pt")
    print("wrote", f"patch_dropout_{tag}.pt", tuple(out.shape), "keep", tuple(keep.shape), float(out.abs().max()))


if __name__ == "__main__":
    for vtype, prob, tag in CASES:
        fixture(vtype, prob, tag)
