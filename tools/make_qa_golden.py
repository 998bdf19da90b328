"""Reference fixture for the question-answering loss (MiCo.forward_qa): tests/golden/qa_b16_d2.pt.

Runs the REFERENCE model (oracle.ref_import: the reference tree, CPU, fp32) the way oracle/make_golden.py:loss_fixture runs the captioning loss:
its own towers and condition packing, then its own multimodal_encoder(input_ids, attention_mask, encoder_hidden_states, labels) on inputs put
together as data/model/vast.py:588-599 prescribes - [question | answer masked at 0.99], labels -100 over the question, the part-causal 3-D mask -
for the task qa%tv%tva.  The TokenMasker draw is oracle.mico_oracle.token_masker's and is stored, as are the token ids; pixels and weights are
regenerated from seeds.  Stored: tensors, ints and strings only.

    python tools/make_qa_golden.py          (needs the reference tree; writes under tests/golden/)
"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from oracle import ref_import  # noqa: E402
from oracle.make_golden import fill, grad_digest  # noqa: E402
from oracle.mico_oracle import token_masker  # noqa: E402
from mico_amd.weights import synth_inputs  # noqa: E402
from common import save_golden  # noqa: E402

VTYPE, DEPTH, TAG = "evaclip02_base", 2, "b16_d2"
B, LQ, LA = 3, 8, 10
INPUT_SEED, TOKEN_SEED, MASKER_SEED = 4321, 61, 17
TASK = "qa%tv%tva"
GRAD_NAMES = ["hidden_trans_vision_multimodal.0.weight", "vision_frame_embedding", "audio_type_embeddings",
              "vision_encoder.visual.patch_embed.proj.weight", "vision_encoder.visual.blocks.1.mlp.{}.weight",
              "multimodal_encoder.bert.embeddings.word_embeddings.weight", "multimodal_encoder.bert.embeddings.position_embeddings.weight",
              "multimodal_encoder.bert.encoder.layer.0.attention.self.query.weight",
              "multimodal_encoder.bert.encoder.layer.5.crossattention.self.key.weight",
              "multimodal_encoder.bert.encoder.layer.11.output.dense.weight",
              "multimodal_encoder.cls.predictions.transform.dense.weight", "multimodal_encoder.cls.predictions.bias"]


def tokens():
    """Question ids [B, LQ] (sample 1 ends in three pads) and answer ids [B, LA] (sample 2 is [CLS][SEP] and pads), BERT style."""
    g = torch.Generator().manual_seed(TOKEN_SEED)

    def ragged(width, lens):
        ids = torch.randint(1000, 30000, (B, width), generator=g)
        lens = torch.tensor(lens)
        mask = (torch.arange(width)[None] < lens[:, None]).long()
        ids[:, 0] = 101
        ids[torch.arange(B), lens - 1] = 102
        return ids * mask, mask

    q_ids, q_mask = ragged(LQ, [LQ, LQ - 3, LQ])
    a_ids, a_mask = ragged(LA, [6, LA, 2])
    return q_ids, q_mask, a_ids, a_mask


def fixture():
    torch.manual_seed(0)
    m = ref_import.build_mico(VTYPE, depth=DEPTH)
    fill(m)
    for p in m.parameters():
        p.requires_grad_(True)
        p.grad = None
    inp = synth_inputs(dict(b=B, vision=2, audio=1, S=0), seed=INPUT_SEED)
    q_ids, q_mask, a_ids, a_mask = tokens()
    masked_ids, labels = token_masker(a_ids, 0.99, random.Random(MASKER_SEED))

    # the QA pass's inputs, vast.py:588-599
    input_ids = torch.cat((q_ids, masked_ids), dim=1)
    all_labels = torch.cat((torch.full_like(q_ids, -100), labels), dim=1)
    keys = torch.cat((q_mask, a_mask), dim=1)
    pos = torch.arange(LQ + LA)
    row, col = pos[:, None], pos[None, :]
    visible = (col < LQ) | ((row >= LQ) & (col <= row))      # question columns for every row; answer columns causally for answer rows
    mask3 = keys[:, None, :] * visible[None].long()

    vo = m.forward_vision_encoder(inp["vision_pixels"])
    ao = m.forward_audio_encoder(inp["audio_spectrograms"])
    cv, ca = m.get_multimodal_forward_input_vision(vo), m.get_multimodal_forward_input_audio(ao)
    cond = {"tv": cv, "tva": torch.cat((cv, ca), dim=1)}
    losses = {st: m.multimodal_encoder(input_ids=input_ids, attention_mask=mask3, encoder_hidden_states=cond[st], labels=all_labels).loss
              for st in TASK.split("%")[1:]}
    loss = sum(losses.values()) / len(losses)
    loss.backward()
    named = dict(m.named_parameters())
    names = [n.format("w3" if "vision_encoder.visual.blocks.1.mlp.w3.weight" in named else "fc2") for n in GRAD_NAMES]
    fx = dict(question_ids=q_ids, question_mask=q_mask, answer_ids=a_ids, answer_mask=a_mask, masked_ids=masked_ids, labels=labels,
              loss_qa=loss.detach().clone(), losses={st: v.detach().clone() for st, v in losses.items()},
              grads={n: grad_digest(named[n].grad) for n in names},
              meta=dict(vtype=VTYPE, depth=DEPTH, b=B, vision=2, audio=1, Lq=LQ, La=LA, task=TASK, input_seed=INPUT_SEED,
                        token_seed=TOKEN_SEED, masker_seed=MASKER_SEED, mask_prob="0.99"))
    save_golden(fx, f"qa_{TAG}.pt")
    print("wrote", f"qa_{TAG}.pt", "loss_qa", float(loss), {st: float(v) for st, v in losses.items()},
          "labelled answer tokens", int((labels != -100).sum()))


if __name__ == "__main__":
    torch.set_num_threads(16)
    fixture()
