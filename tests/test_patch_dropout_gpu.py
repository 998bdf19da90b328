"""Patch dropout (FLIP) in the EVA towers on the MI355X: the four kernels (mico_im2row_keep, mico_patch_pos_keep, mico_rope_keep,
mico_pos_grad_keep), the tower against the reference's own patch-dropping pass (tests/golden/patch_dropout_*.pt, written by
tools/make_patch_dropout_golden.py) in the parity and the timed fp16 configurations, composition with stochastic depth and the
staged MiCo step against the fp32 oracle, and the identities that keep every existing path bit for bit."""
import pytest
import torch

from common import golden, rel_err, build_model, grad_digest_check, precision_config, PRECISION_CONFIGS
from mico_amd import ops, runtime
from mico_amd import functional as Fn
from mico_amd.model.evaclip import PatchDropout
from mico_amd.weights import synth_inputs
from oracle import mico_oracle as O

pytestmark = pytest.mark.gpu

FWD_TOL = {torch.float16: 1e-3, torch.bfloat16: 1.2e-2}      # the gates of tests/test_model_gpu.py
GRAD_TOL = {torch.float16: 2e-2, torch.bfloat16: 6e-2}
_EVA_VIT_FORWARD = O.eva_vit_forward      # (the MiCo-level test replaces the oracle's tower; the restatement keeps the original)
FIXTURES = [("evaclip02_base", "b16_d2_p50"), ("evaclip01_giant", "g14_d2_p50"), ("evaclip01_giant", "g14_d2_p75")]


def _keep_table(frames, np_, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(np_, generator=g)[:k] for _ in range(frames)])


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,P,k", [(3, 14, 128), (1, 14, 64), (3, 16, 98)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_im2row_keep_is_im2row_then_row_selection(cuda, C, P, k, dtype):
    B, np_ = 3, (224 // P) ** 2
    kpad = (C * P * P + 63) // 64 * 64
    px = torch.randn(B, C, 224, 224, device=cuda)
    full = torch.empty(B * np_, kpad, dtype=dtype, device=cuda)
    ops.im2row(px, full, P, kpad)
    keep = _keep_table(B, np_, k)
    rows = torch.empty(B * k, kpad, dtype=dtype, device=cuda)
    ops.im2row_keep(px, rows, keep.to(cuda, torch.int32), P, kpad)
    sel = full.view(B, np_, kpad)[torch.arange(B)[:, None], keep.to(cuda)].reshape(B * k, kpad)
    assert torch.equal(rows.view(torch.int16), sel.view(torch.int16))


def test_patch_pos_keep(cuda):
    B, np_, k, D = 3, 256, 128, 1408
    keep = _keep_table(B, np_, k)
    x = torch.randn(B * (k + 1), D, device=cuda)
    cls, pos = torch.randn(D, device=cuda), torch.randn(np_ + 1, D, device=cuda)
    want = x.clone().view(B, k + 1, D)
    want[:, 0] = cls + pos[0]
    want[:, 1:] += pos[1:][keep.to(cuda)]
    ops.patch_pos_keep(x, keep.to(cuda, torch.int32), cls, pos)
    assert torch.equal(x.view(B, k + 1, D), want)


def _ulp16(t, dtype):
    t = t.abs().float()
    e = torch.floor(torch.log2(t.clamp_min(torch.finfo(dtype).tiny)))
    return torch.exp2(e - (10 if dtype == torch.float16 else 7))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("with_map", [False, True])
def test_rope_keep_forward_and_inverse(cuda, dtype, with_map):
    """Within 1 ulp of an fp32 torch evaluation on the same 16-bit input (rope.py:120-136 with the kept rows' table rows)."""
    from mico_amd.model.evaclip.eva_vit_model import _rope_tables
    B, H, hd, grid, k = 4, 12, 64, 14, 98
    np_, N, D = grid * grid, k + 1, H * hd
    cos, sin = (t.to(cuda) for t in _rope_tables(hd, grid))
    table = _keep_table(6, np_, k)
    fmap = torch.tensor([5, 0, 3, 2], dtype=torch.int32) if with_map else None
    frames = fmap.long() if with_map else torch.arange(B)
    qkv = torch.randn(B * N, 3 * D, device=cuda).to(dtype)
    x0 = qkv.float().view(B, N, 3, H, hd)[:, 1:, :2]          # q and k, tokens 1..
    c = cos[table[frames].to(cuda)][:, :, None, None]          # [B, k, 1, 1, hd]
    s = sin[table[frames].to(cuda)][:, :, None, None]
    x1, x2 = x0.reshape(*x0.shape[:-1], -1, 2).unbind(-1)
    rot = torch.stack((-x2, x1), -1).reshape(x0.shape)
    for inverse in (False, True):
        out = qkv.clone()
        args = (B, N, H, hd, cos, sin, table.to(cuda, torch.int32))
        kw = dict(frame_map=fmap.to(cuda) if with_map else None, inverse=inverse)
        ops.rope_keep(out, N * 3 * D, 3 * D, *args, **kw)
        ops.rope_keep(out[:, D:], N * 3 * D, 3 * D, *args, **kw)
        if not inverse:
            want = x0 * c + rot * s
        else:      # the transpose: y = x cos - rotate_half(x sin) ... written out per pair
            xs = x0 * s
            s1, s2 = xs.reshape(*xs.shape[:-1], -1, 2).unbind(-1)
            want = x0 * c + torch.stack((s2, -s1), -1).reshape(x0.shape)
        got = out.float().view(B, N, 3, H, hd)[:, 1:, :2]
        err = (got - want).abs()
        # 1 ulp of the 16-bit result, plus what the fp32 evaluation itself is uncertain by where the two products cancel (a few fp32 ulps
        # of the products: the kernel may fuse a multiply-add that torch rounds twice)
        terms = (x0 * c).abs() + (rot * s).abs()
        tol = _ulp16(want, dtype) * 1.0001 + terms * 2.0 ** -22
        assert bool((err <= tol).all()), (inverse, float((err / tol).max()))
        assert torch.equal(out.view(B, N, 3 * D)[:, 0], qkv.view(B, N, 3 * D)[:, 0])          # CLS untouched
        assert torch.equal(out.view(B, N, 3, D)[:, :, 2], qkv.view(B, N, 3, D)[:, :, 2])      # v untouched


def test_pos_grad_keep(cuda):
    """dpos[0] = sum_f g[f, 0], dpos[1 + keep[f, r]] += g[f, 1 + r]: against an fp32 index_add to 1e-6, and bit-identical across launches."""
    B, np_, k, D = 37, 256, 128, 1408
    keep = _keep_table(B, np_, k)
    g = torch.randn(B * (k + 1), D, device=cuda)
    want = torch.zeros(np_ + 1, D, dtype=torch.float64, device=cuda)
    gv = g.view(B, k + 1, D).double()
    want[0] = gv[:, 0].sum(0)
    want.index_add_(0, (1 + keep).reshape(-1).to(cuda), gv[:, 1:].reshape(-1, D))
    kd = keep.to(cuda, torch.int32)
    a = ops.pos_grad_keep(g, kd, np_)
    b = ops.pos_grad_keep(g, kd, np_)
    assert torch.equal(a, b)
    err = ((a.double() - want).abs().max() / want.abs().max()).item()
    assert err < 1e-6, err
    dropped = torch.ones(np_, dtype=torch.bool)
    dropped[keep.reshape(-1)] = False
    assert bool((a[1:][dropped.to(cuda)] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the tower against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _tower_case(tag, vtype, cuda, **over):
    fx = golden(f"patch_dropout_{tag}.pt")
    m, sd = build_model(vtype, 2, device=cuda, patch_dropout=fx["meta"]["prob"], **over)
    g = torch.Generator().manual_seed(fx["meta"]["input_seed"])
    x = torch.randn((2, 3, 224, 224), generator=g)
    w = torch.randn(fx["out"].shape, generator=g) / fx["out"].numel() ** 0.5
    return fx, m, sd, x, w


@pytest.mark.parametrize("vtype,tag", FIXTURES)
@pytest.mark.parametrize("config", PRECISION_CONFIGS)
def test_tower_vs_reference(cuda, vtype, tag, config):
    """The reference's own patch-dropping pass (training mode, blocks in eval) with its keep indices injected: 99 tokens (B/16, RoPE),
    129 (g/14: the resident attention forward and the one-pass backward), 65 (g/14: the general kernels)."""
    fx, m, sd, x, w = _tower_case(tag, vtype, cuda)
    vis = m.vision_encoder.visual.train()
    depth = len(vis.blocks)
    ones = torch.ones(depth, 2, 2)        # DropPath off (the fixture's blocks ran in eval mode)
    m.zero_grad(set_to_none=True)
    with precision_config(config):
        out = vis.forward_groups([x.to(cuda)], drop_path_scale=ones, patch_keep=fx["keep"])
        assert out.shape == fx["out"].shape
        e = rel_err(out, fx["out"])
        (out * w.to(cuda)).sum().backward()
        torch.cuda.synchronize()
    named = dict(vis.named_parameters())
    worst = max(grad_digest_check(d, named[n].grad, None) for n, d in fx["grads"].items())
    pos_rows = named["pos_embed"].grad[0].norm(dim=-1).cpu()
    assert torch.equal(pos_rows == 0, fx["pos_grad_row_norm"] == 0)       # exactly the rows no frame kept stay zero
    print(f"{tag} {config}: N = {out.shape[1]}, fwd rel err {e:.2e}, worst grad err {worst:.2e}")
    assert e < FWD_TOL[torch.float16] and worst < GRAD_TOL[torch.float16], (e, worst)


# ---------------------------------------------------------------------------------------------------------------------------------
# composition with stochastic depth: fp32 restatement from the oracle's building blocks
# ---------------------------------------------------------------------------------------------------------------------------------
def eva_vit_forward_pd(sd, x, arch, keep, pre="vision_encoder.visual.", drop_path_scale=None):
    """O.eva_vit_forward with the reference's patch dropout (transformer.py:144-185) after the position embedding and, for RoPE towers,
    per-frame gathered table rows (rope.py:120-136).  keep: int64 [B, k] (None: O.eva_vit_forward itself)."""
    if keep is None:
        return _EVA_VIT_FORWARD(sd, x, arch, pre=pre, drop_path_scale=drop_path_scale)
    B = x.shape[0]
    t = O.patch_embed(sd, pre, x, arch["patch"])
    t = torch.cat((sd[pre + "cls_token"].expand(B, -1, -1), t), dim=1) + sd[pre + "pos_embed"]
    t = torch.cat((t[:, :1], t[:, 1:][torch.arange(B)[:, None], keep]), dim=1)
    rope = None
    if arch["rope"]:
        cos, sin = O.rope_tables(arch["width"] // arch["heads"], x.shape[-1] // arch["patch"])
        rope = (cos[keep][:, None], sin[keep][:, None])        # [B, 1, k, hd]: broadcast over the heads
    for i in range(O.vit_depth(sd, pre)):
        p = pre + f"blocks.{i}."
        a = O.eva_attention(sd, p + "attn.", O.layer_norm(t, sd[p + "norm1.weight"], sd[p + "norm1.bias"], O.VIT_EPS), arch, rope)
        if drop_path_scale is not None:
            a = a * drop_path_scale[i, 0].view(B, 1, 1)
        t = t + a
        mm = O.eva_mlp(sd, p + "mlp.", O.layer_norm(t, sd[p + "norm2.weight"], sd[p + "norm2.bias"], O.VIT_EPS), arch)
        if drop_path_scale is not None:
            mm = mm * drop_path_scale[i, 1].view(B, 1, 1)
        t = t + mm
    return O.layer_norm(t, sd[pre + "norm.weight"], sd[pre + "norm.bias"], O.VIT_EPS)


@pytest.mark.parametrize("vtype,prob", [("evaclip02_base", 0.5), ("evaclip01_giant", 0.5), ("evaclip01_giant", 0.75)])
def test_patch_dropout_with_frame_skipping(cuda, vtype, prob):
    """Patch dropout with injected DropPath masks at depth 3 (the shape of test_droppath_gpu.py::test_tower_frame_skipping): the compact
    frame lists of the kept branches index the per-frame keep table (RoPE rows, LayerNorm frame maps, gradient hand-over)."""
    depth, B = 3, 5
    m, sd = build_model(vtype, depth, device=cuda, patch_dropout=prob)
    vis = m.vision_encoder.visual.train()
    np_ = vis.patch_embed.num_patches
    keep = _keep_table(B, np_, Fn.patch_keep_count(np_, prob), seed=3)
    scale = torch.ones(depth, 2, B)
    scale[0, 0, 1] = 0
    scale[1, 1, [0, 3]] = 0
    scale[2, 0, 4] = 0
    scale[2, 1, 2] = 0
    scale[scale != 0] = 1 / 0.8
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 3, 224, 224, generator=g)
    m.zero_grad(set_to_none=True)
    with runtime.precision(torch.float16):
        out = vis.forward_groups([x.to(cuda)], drop_path_scale=scale, patch_keep=keep)
        w = torch.randn(out.shape, generator=g) / out.numel() ** 0.5
        (out * w.to(cuda)).sum().backward()
    pre = "vision_encoder.visual."
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith(pre) and v.is_floating_point()}
    arch = O.ARCHS[vtype]
    ref = eva_vit_forward_pd(sdo, x, arch, keep, drop_path_scale=scale)
    (ref * w).sum().backward()
    e = rel_err(out, ref)
    named = dict(vis.named_parameters())
    worst = 0.0
    for n in ("patch_embed.proj.weight", "patch_embed.proj.bias", "cls_token", "pos_embed", f"blocks.0.norm1.weight", f"blocks.{depth - 1}.mlp."
              + ("w3.weight" if arch["swiglu"] else "fc2.weight")):
        r = sdo[pre + n].grad
        worst = max(worst, ((named[n].grad.float().cpu() - r).abs().max() / r.abs().max()).item())
    print(f"{vtype} p={prob}: fwd {e:.2e} grad {worst:.2e}")
    assert e < FWD_TOL[torch.float16] and worst < GRAD_TOL[torch.float16], (e, worst)


# ---------------------------------------------------------------------------------------------------------------------------------
# MiCo level: train mode, injected draws, direct and staged step against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staged", [False, True])
def test_mico_step_with_patch_dropout(cuda, monkeypatch, staged):
    vt, b, prob = "evaclip02_base", 2, 0.5
    m, sd = build_model(vt, 2, device=cuda, patch_dropout=prob)
    m.train()
    m.multimodal_encoder.bert.config.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    inp = synth_inputs(dict(b=b, vision=1, audio=2, depth=1, S=12), seed=11)
    import random
    mi, lab = O.token_masker(inp["input_ids"], 0.6, random.Random(0))
    idx = torch.arange(b).roll(1)
    np_ = m.vision_encoder.visual.patch_embed.num_patches
    k = Fn.patch_keep_count(np_, prob)
    keeps = {"v": _keep_table(b * 1, np_, k, 1), "a": _keep_table(b * 2, np_, k, 2), "d": _keep_table(b * 1, np_, k, 3)}
    depth = len(m.vision_encoder.visual.blocks)
    dps = {mod: torch.ones(depth, 2, keeps[mod].shape[0]) for mod in keeps}
    injected = {"tva": dict(neg_cond_idx=idx, neg_text_idx=idx), "tvd": dict(neg_cond_idx=idx, neg_text_idx=idx),
                "cap": dict(masked_ids=mi, labels=lab), "drop_path_scale": dps, "patch_keep": keeps}
    task = "ret%tva%tvd_cap%tva"
    # oracle: the towers run the patch-dropping restatement, the modalities in encode_batch's order (v, a, d)
    order = [keeps["v"], keeps["a"], keeps["d"]]
    calls = []

    def vit_pd(sd_, x, arch, pre="vision_encoder.visual.", drop_path_scale=None, taps=None):
        kt = order[len(calls)]
        calls.append(x.shape[0])
        assert kt.shape[0] == x.shape[0]
        return eva_vit_forward_pd(sd_, x, arch, kt, pre=pre, drop_path_scale=drop_path_scale)

    monkeypatch.setattr(O, "eva_vit_forward", vit_pd)
    sdo = {k_: v.clone().requires_grad_(v.is_floating_point()) for k_, v in sd.items()}
    sdo["multimodal_encoder.cls.predictions.decoder.weight"] = sdo["multimodal_encoder.bert.embeddings.word_embeddings.weight"]
    ref, _ = O.mico_forward(sdo, O.ARCHS[vt], inp, task, dict(itm_ratio=0.1), injected=injected)
    assert calls == [2, 4, 2]
    sum(ref.values()).backward()
    batch = {k_: v.to(cuda) for k_, v in inp.items()}
    batch["_injected"] = injected
    m.zero_grad(set_to_none=True)
    with precision_config("parity"):
        out = m(dict(batch), task, compute_loss=True, backward_scale=1.0 if staged else None)
        sum(out.values()).backward()
        torch.cuda.synchronize()
    for key in ref:
        a, r = float(out[key].detach()), float(ref[key].detach())
        assert abs(a - r) <= 1e-3 * max(abs(r), 1e-6), (key, a, r)
    worst = 0.0
    for n in ("vision_encoder.visual.pos_embed", "vision_encoder.visual.patch_embed.proj.weight", "vision_encoder.visual.blocks.0.attn.q_proj.weight",
              "vision_encoder.visual.blocks.1.mlp.w3.weight"):
        r = sdo[n].grad
        gpu = dict(m.named_parameters())[n].grad.float().cpu()
        worst = max(worst, ((gpu - r).abs().max() / r.abs().max()).item())
    print(f"staged={staged}: losses {({k_: float(v) for k_, v in out.items()})}, worst grad err {worst:.2e}")
    assert worst < 2e-2, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# identities and modes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vtype", ["evaclip02_base", "evaclip01_giant"])
def test_inactive_patch_dropout_is_bit_identical(cuda, vtype):
    """Eval mode at p = 0.5 and train mode at p = 0 give outputs torch.equal to a model built without the knob (same weights, same
    DropPath draw)."""
    depth, B = 2, 3
    base, _ = build_model(vtype, depth, device=cuda)
    half, _ = build_model(vtype, depth, device=cuda, patch_dropout=0.5)
    zero, _ = build_model(vtype, depth, device=cuda, patch_dropout=0.0)
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(9)).to(cuda)
    scale = torch.ones(depth, 2, B)
    scale[1, 0, 1] = 0
    scale[scale != 0] = 1 / 0.9
    with runtime.precision(torch.float16):
        ref_eval = base.vision_encoder.visual.eval().forward_groups([x])
        got_eval = half.vision_encoder.visual.eval().forward_groups([x])
        ref_train = base.vision_encoder.visual.train().forward_groups([x], drop_path_scale=scale)
        got_train = zero.vision_encoder.visual.train().forward_groups([x], drop_path_scale=scale)
    assert torch.equal(ref_eval, got_eval)
    assert torch.equal(ref_train, got_train)


def test_fp8_step_with_patch_dropout(cuda):
    """One fp8-mode training step at p = 0.5 (g/14 architecture, 2 blocks): finite losses and gradients."""
    import bench
    m, _ = build_model("evaclip01_giant", 2, device=cuda, patch_dropout=0.5)
    m.train()
    inp = synth_inputs(dict(b=2, vision=1, audio=2, S=12), seed=4)
    batch = {k: v.to(cuda) for k, v in inp.items()}
    old = runtime.snapshot()
    try:
        bench.set_precision("fp8")
        m.zero_grad(set_to_none=True)
        out = m(dict(batch), "ret%tva_cap%tva", compute_loss=True, backward_scale=1.0)
        sum(out.values()).backward()
        torch.cuda.synchronize()
        assert runtime.last_tower_plan["tokens_per_frame"] == 129
    finally:
        runtime.restore(old)
        runtime.clear_weight_cache()
    assert all(torch.isfinite(v.detach()).all() for v in out.values())
    for n, p in m.vision_encoder.visual.named_parameters():
        if not n.startswith("head."):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n


def test_full_size_step_fits_one_pass(cuda):
    """ViT-g/14 depth 40, one configs[2]-shaped batch (b = 64: image + 4 audio windows + 77 text tokens, 320 tower frames), train mode,
    staged step: at p = 0.5 the tower runs in one pass keeping every activation (129 tokens per frame), and its allocated peak is below
    the p = 0 peak of the same batch."""
    import bench
    from mico_amd.model import default_cfg
    model, _ = bench.build_model(default_cfg("evaclip01_giant", vision_layers=None))
    model.to(cuda).train()
    inp = synth_inputs(dict(b=64, vision=1, audio=4, S=77), seed=7)
    batch = {k: v.to(cuda) for k, v in inp.items()}
    vis = model.vision_encoder.visual
    old = runtime.snapshot()
    peaks, plans = {}, {}
    try:
        bench.set_precision("fp16")
        for p in (0.0, 0.5):
            vis.patch_dropout = PatchDropout(p) if p > 0 else torch.nn.Identity()
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(cuda)
            out = model(dict(batch), "ret%tva_cap%tva", compute_loss=True, backward_scale=1.0)
            sum(out.values()).backward()
            torch.cuda.synchronize()
            assert all(torch.isfinite(v.detach()).all() for v in out.values())
            peaks[p] = torch.cuda.max_memory_allocated(cuda)
            plans[p] = dict(runtime.last_tower_plan)
            del out
    finally:
        runtime.restore(old)
        runtime.clear_weight_cache()
    print("peaks GiB", {p: v / 2 ** 30 for p, v in peaks.items()}, "plans", plans)
    assert plans[0.5]["tokens_per_frame"] == 129 and plans[0.0]["tokens_per_frame"] == 257
    assert plans[0.5]["frames_per_pass"] == 320 and plans[0.5]["diet"] == 0
    assert peaks[0.5] < peaks[0.0]
