"""Question answering (MiCo.forward_qa, BertForMaskedLM.generate(rows_per_condition=...), mico_attn_decode_ragged): everything that needs
no GPU - the part-causal mask against a hand-written one, the plain-torch restatement of the loss against the reference's own value
(tests/golden/qa_b16_d2.pt), argument checks that come before any launch, the ABI, the host-side first-row table."""
import os
import re

import pytest
import torch

import qa_oracle
from common import golden, build_model
from mico_amd import functional as Fn
from mico_amd import ops
from mico_amd.model.bert import BertForMaskedLM
from mico_amd.model.mico_forward import qa_attention_mask
from mico_amd.weights import synth_inputs
from oracle import mico_oracle as O

_SMALL = dict(num_hidden_layers=1, vocab_size=128, intermediate_size=64)


def test_qa_attention_mask_by_hand():
    """Lq = 3, La = 3, the last question token and the last answer token padded: question rows see the unpadded question only; answer
    rows see it and the unpadded answer positions up to their own."""
    expected = torch.tensor([[[1, 1, 0, 0, 0, 0],
                              [1, 1, 0, 0, 0, 0],
                              [1, 1, 0, 0, 0, 0],
                              [1, 1, 0, 1, 0, 0],
                              [1, 1, 0, 1, 1, 0],
                              [1, 1, 0, 1, 1, 0]]])
    qm, am = torch.tensor([[1, 1, 0]]), torch.tensor([[1, 1, 0]])
    got = qa_attention_mask(qm, am)
    assert got.shape == (1, 6, 6) and got.is_contiguous() and torch.equal(got, expected)
    assert torch.equal(qa_oracle.qa_mask(qm, am), expected)
    # two samples with different padding, against the entry-by-entry restatement
    qm, am = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]]), torch.tensor([[1, 1, 0], [1, 1, 1]])
    assert torch.equal(qa_attention_mask(qm, am), qa_oracle.qa_mask(qm, am))


def test_restatement_reproduces_the_reference_loss():
    """tests/qa_oracle.py on the fixture's inputs gives the reference's loss_qa (fp32 against fp32: the bound test_oracle_vs_golden.py
    puts on the captioning loss)."""
    fx = golden("qa_b16_d2.pt")
    meta = fx["meta"]
    assert (meta["Lq"], meta["La"], meta["b"], meta["task"]) == (8, 10, 3, "qa%tv%tva")
    assert fx["question_mask"][1].tolist() == [1] * 5 + [0] * 3                       # a question with trailing pads
    assert fx["answer_ids"][2].tolist() == [101, 102] + [0] * 8                        # an answer of [CLS][SEP] alone
    assert (fx["labels"][:, 0] == -100).all() and ((fx["labels"] != -100).sum(1) >= 1).all()
    torch.set_num_threads(16)
    _, sd = build_model(meta["vtype"], meta["depth"])
    sd = dict(sd)
    sd["multimodal_encoder.cls.predictions.decoder.weight"] = sd["multimodal_encoder.bert.embeddings.word_embeddings.weight"]
    inp = synth_inputs(dict(b=meta["b"], vision=meta["vision"], audio=meta["audio"], S=0), seed=meta["input_seed"])
    with torch.no_grad():
        loss, each = qa_oracle.qa_loss(sd, O.ARCHS[meta["vtype"]], inp, fx, meta["task"].split("%")[1:])
    print("loss_qa", loss.item(), fx["loss_qa"].item(), {k: v.item() for k, v in each.items()})
    v = fx["loss_qa"].item()
    assert abs(loss.item() - v) < 2e-5 * max(1.0, abs(v))
    for st, l in each.items():
        assert abs(l.item() - fx["losses"][st].item()) < 2e-5 * max(1.0, abs(fx["losses"][st].item())), st


def test_rows_per_condition_argument_errors_come_before_any_launch():
    """Host tensors throughout: a launch would fail differently."""
    m = BertForMaskedLM(_SMALL).eval()
    ids = torch.full((4, 2), 101)
    mask = ids.new_ones(4, 2, 2)
    cond = torch.zeros(3, 5, 768)
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=2, num_beams=2)
    for use_cache in (False, True):
        with pytest.raises(ValueError, match="adds up to 5"):
            m.generate(encoder_hidden_states=cond, rows_per_condition=[2, 1, 2], use_cache=use_cache, **kw)
        with pytest.raises(ValueError, match="2 entries for 3 condition sets"):
            m.generate(encoder_hidden_states=cond, rows_per_condition=[2, 2], use_cache=use_cache, **kw)
        with pytest.raises(ValueError, match="negative"):
            m.generate(encoder_hidden_states=cond, rows_per_condition=[5, -1, 0], use_cache=use_cache, **kw)
        with pytest.raises(ValueError, match="condition sets"):
            m.generate(encoder_hidden_states=None, rows_per_condition=[4], use_cache=use_cache, **kw)
    with pytest.raises(ValueError, match="beam search only"):
        m.generate(input_ids=ids, attention_mask=mask, encoder_hidden_states=cond, rows_per_condition=[2, 0, 2], do_sample=True)


def test_forward_qa_refuses_other_task_families():
    from mico_amd.model import MiCo
    assert callable(MiCo.forward_qa)
    with pytest.raises(ValueError, match="qa%"):
        MiCo.forward_qa(None, {}, "cap%tv")
    with pytest.raises(ValueError, match="qa%"):
        MiCo.forward_qa(None, {}, "qa")
    with pytest.raises(ValueError, match="zz"):                 # an unknown sub-task, before the model (None) is touched
        MiCo.forward_qa(None, {}, "qa%zz")


def test_abi_declares_and_exports_the_ragged_decode():
    from mico_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mico_hip.h")).read()
    l = _lib.lib()
    assert l.mico_version() == _lib.ABI_VERSION >= 118
    for name in ("mico_attn_decode_ragged", "mico_attn_decode_ragged_ws_bytes"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES and getattr(l, name) is not None
    # the workspace twin is host arithmetic: the uniform launch's size at the largest set's query count
    assert l.mico_attn_decode_ragged_ws_bytes(3, 2, 5, 2, 70, 1) == 0
    assert l.mico_attn_decode_ragged_ws_bytes(3, 2, 5, 2, 197, 3) == l.mico_attn_decode_ws_bytes(3, 2, 10, 197, 3) > 0
    assert l.mico_attn_decode_ragged_ws_bytes(3, 2, 0, 2, 197, 3) == -1
    # refusals before any launch (fake pointers are never dereferenced)
    import ctypes
    fake = ctypes.c_void_p(4096)
    args = lambda **o: [o.get(k, d) for k, d in (("q", fake), ("q_rs", 128), ("k", fake), ("v", fake), ("kv_ss", 70 * 256), ("kv_rs", 256),
                                                 ("o", fake), ("o_rs", 128), ("mask", None), ("mask_rs", 0), ("mask_qs", 0), ("sets", 3),
                                                 ("set_row0", fake), ("rows", 8), ("max_rows", 5), ("q_per_row", 2), ("H", 2), ("Sk", 70),
                                                 ("hd", 64), ("scale", 0.125), ("splits", 1), ("ws", None), ("ws_bytes", 0), ("dtype", 0),
                                                 ("stream", None))]
    for bad in (dict(set_row0=None), dict(hd=32), dict(max_rows=9), dict(max_rows=2), dict(rows=0), dict(splits=2, Sk=197)):
        assert l.mico_attn_decode_ragged(*args(**bad)) == -22, bad
    assert b"mico_attn_decode_ragged" in l.mico_last_error_string()


def test_decode_cache_first_row_table_is_built_on_the_host():
    t = Fn.BertDecodeCache.set_row_table((3, 0, 6))
    assert t.dtype == torch.int32 and t.device.type == "cpu" and t.tolist() == [0, 3, 3, 9]
    assert ops.decode_set_row0([4]).tolist() == [0, 4]
    for bad in ((), (2, -1, 3)):
        with pytest.raises(ValueError):
            Fn.BertDecodeCache.set_row_table(bad)
