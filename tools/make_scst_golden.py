"""Reference fixture for the SCST scoring pass (BertForMaskedLM.sequence_logprobs): tests/golden/scst_b16_d2.pt.

Runs the REFERENCE model (oracle.ref_import: the reference tree, CPU, fp32) the way tools/make_qa_golden.py runs the QA loss: its own towers
and condition packing, then its own multimodal_encoder STEP BY STEP under its [MASK]-append protocol (prepare_inputs_for_generation,
model/bert.py:1126-1143: the prefix plus one [MASK], the mask grown by one position) on stored token ids - the schedule of its sample_scst,
one pass with grad per generated position - for the condition tokens of tv and tva.  At every step log_softmax of the [MASK] row is gathered
at the stored token; positions after a row's [SEP] are 0.  sum_st sum(w[row] * logp[row, t]) with stored per-row weights is differentiated.
Stored: tensors, ints and strings only; pixels and weights are regenerated from seeds.

    python tools/make_scst_golden.py          (needs the reference tree; writes under tests/golden/)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from oracle import ref_import  # noqa: E402
from oracle.make_golden import fill, grad_digest  # noqa: E402
from mico_amd.weights import synth_inputs  # noqa: E402
from common import save_golden  # noqa: E402
from make_qa_golden import GRAD_NAMES  # noqa: E402

VTYPE, DEPTH, TAG = "evaclip02_base", 2, "b16_d2"
B, T = 3, 6
INPUT_SEED, TOKEN_SEED = 4321, 83
SUBTASKS = ("tv", "tva")
WEIGHTS = (1.0, -0.75, 0.0)      # per row: one negative (the row that ends early), one zero
CLS, SEP, PAD = 101, 102, 0


def tokens():
    """[CLS] + T generated ids [B, 1 + T]; row 1 reaches [SEP] at step 3 and is padded after it."""
    g = torch.Generator().manual_seed(TOKEN_SEED)
    ids = torch.randint(1000, 30000, (B, 1 + T), generator=g)
    ids[:, 0] = CLS
    ids[1, 3] = SEP
    ids[1, 4:] = PAD
    return ids


def fixture():
    torch.manual_seed(0)
    m = ref_import.build_mico(VTYPE, depth=DEPTH)
    fill(m)
    for p in m.parameters():
        p.requires_grad_(True)
        p.grad = None
    inp = synth_inputs(dict(b=B, vision=2, audio=1, S=0), seed=INPUT_SEED)
    ids = tokens()
    gen = ids[:, 1:]
    is_eos = (gen == SEP).long()
    valid = ((is_eos.cumsum(1) - is_eos) == 0).float()
    w = torch.tensor(WEIGHTS)

    vo = m.forward_vision_encoder(inp["vision_pixels"])
    ao = m.forward_audio_encoder(inp["audio_spectrograms"])
    cv, ca = m.get_multimodal_forward_input_vision(vo), m.get_multimodal_forward_input_audio(ao)
    cond = {"tv": cv, "tva": torch.cat((cv, ca), dim=1)}
    me = m.multimodal_encoder
    logp, top = {}, 0.0
    for st in SUBTASKS:
        mask = torch.ones(B, 1, 1, dtype=torch.long)
        steps = []
        for t in range(T):
            step = me.prepare_inputs_for_generation(ids[:, :1 + t], attention_mask=mask, encoder_hidden_states=cond[st])
            logits = me(input_ids=step["input_ids"], attention_mask=step["attention_mask"],
                        encoder_hidden_states=step["encoder_hidden_states"]).logits[:, -1]
            top = max(top, float(logits.detach().abs().max()))
            steps.append(torch.log_softmax(logits.float(), dim=-1).gather(1, gen[:, t:t + 1].clamp_min(0))[:, 0])
            mask = step["attention_mask"]
        logp[st] = torch.stack(steps, dim=1) * valid
    total = sum((w[:, None] * logp[st]).sum() for st in SUBTASKS)
    total.backward()
    named = dict(m.named_parameters())
    names = [n.format("w3" if "vision_encoder.visual.blocks.1.mlp.w3.weight" in named else "fc2") for n in GRAD_NAMES]
    fx = dict(ids=ids, weights=w, valid=valid, logp={st: v.detach().clone() for st, v in logp.items()}, objective=total.detach().clone(),
              grads={n: grad_digest(named[n].grad) for n in names},
              meta=dict(vtype=VTYPE, depth=DEPTH, b=B, vision=2, audio=1, T=T, subtasks="%".join(SUBTASKS), input_seed=INPUT_SEED,
                        token_seed=TOKEN_SEED, max_abs_logit=top))
    save_golden(fx, f"scst_{TAG}.pt")
    print("wrote", f"scst_{TAG}.pt", "objective", float(total), {st: v.detach().tolist() for st, v in logp.items()}, "max |logit|", top)


if __name__ == "__main__":
    torch.set_num_threads(16)
    fixture()
