"""Device-side beam search and the logits processors of BertForMaskedLM.generate, the parts that need no GPU: the pure-torch processor
function against transformers' processors, the host beam search with processors over scripted logits, generate()'s argument errors, and
the C ABI of the three beam entry points."""
import ctypes
import os
import re

import pytest
import torch

from mico_amd.model.bert import BertForMaskedLM, apply_logits_processors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLS, SEP, PAD = 101, 102, 0
NEG_INF = float("-inf")


def _same(got, ref):
    """finite entries bit-equal, -inf in the same places"""
    assert torch.equal(torch.isinf(got), torch.isinf(ref))
    fin = torch.isfinite(ref)
    assert torch.equal(got[fin].view(torch.int32), ref[fin].view(torch.int32))


def _proc_case():
    g = torch.Generator().manual_seed(11)
    scores = torch.log_softmax(3 * torch.randn(5, 97, generator=g), dim=-1)
    ids = torch.randint(1, 97, (5, 14), generator=g)
    ids[0] = torch.tensor([5, 6, 7, 5, 6, 9, 0, 5, 6, 7, 8, 5, 6, 7])       # bigram (5, 6) and trigram (5, 6, 7) repeat, a pad in the middle
    ids[1] = torch.tensor([3, 3, 3, 3, 0, 3, 3, 4, 3, 3, 5, 9, 3, 3])
    ids[2, 6] = PAD
    ids[3, -2:] = ids[3, 2:4]
    return scores, ids


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("p", [1.3, 0.8])
def test_processor_function_matches_transformers(n, p):
    scores, ids = _proc_case()
    try:
        from transformers.generation.logits_process import (MinLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                            RepetitionPenaltyLogitsProcessor)
        hf = True
    except ImportError:      # only the comparison is skipped: the properties below are checked either way
        hf = False
    for cur in (n - 2, n - 1, n, 14):      # cur + 1 < n, cur + 1 == n: not one complete window yet
        if cur < 1:
            continue
        sub = ids[:, :cur].contiguous()
        got_pen = apply_logits_processors(scores, sub, SEP, repetition_penalty=p)
        got_ng = apply_logits_processors(scores, sub, SEP, no_repeat_ngram_size=n)
        got_all = apply_logits_processors(scores, sub, 7, repetition_penalty=p, no_repeat_ngram_size=n, ban_eos=True)
        if hf:
            ref_pen = RepetitionPenaltyLogitsProcessor(penalty=p)(sub, scores.clone())
            ref_ng = NoRepeatNGramLogitsProcessor(n)(sub, scores.clone())
            ref_all = MinLengthLogitsProcessor(cur + 1, 7)(sub, NoRepeatNGramLogitsProcessor(n)(sub, ref_pen.clone()))
            _same(got_pen, ref_pen)
            _same(got_ng, ref_ng)
            _same(got_all, ref_all)
        # the definitions themselves, entry by entry
        for r in range(sub.shape[0]):
            row = sub[r].tolist()
            seen = set(row)
            banned = {row[i + n - 1] for i in range(cur - n + 1) if row[i:i + n - 1] == row[cur - n + 1:]} if cur >= n else set()
            for t in range(scores.shape[1]):
                s = float(scores[r, t])
                s32 = scores[r, t]
                assert float(got_pen[r, t]) == (float(s32 * p if s < 0 else s32 / p) if t in seen else s)
                assert (float(got_ng[r, t]) == NEG_INF) == (t in banned)
                assert (float(got_all[r, t]) == NEG_INF) == (t in banned or t == 7)
        assert torch.equal(scores, _proc_case()[0]), "the input scores are not modified"
    # an id outside [0, V) names no score
    wild = ids.clone()
    wild[:, 4] = 97
    wild[:, 5] = -3
    ref = apply_logits_processors(scores, torch.cat([ids[:, :4], ids[:, 6:]], dim=1), SEP, repetition_penalty=p)
    _same(apply_logits_processors(scores, wild, SEP, repetition_penalty=p), ref)
    assert torch.isfinite(apply_logits_processors(scores, wild, None, no_repeat_ngram_size=1, ban_eos=True)[:, 96]).all()


class _ScriptedStep:
    """next_token_logits from a seeded table: the row's logits depend on its last token and its length only; eos is the largest logit."""

    def __init__(self, vocab=40, eos_gap=1.0, seed=5, by_length=True):
        g = torch.Generator().manual_seed(seed)
        self.table = 2 * torch.randn(64, vocab, generator=g)
        self.table[:, SEP % vocab] = self.table.max(dim=1).values + eos_gap
        self.vocab, self.by_length = vocab, by_length

    def next_token_logits(self, ids, parent=None):
        key = (ids[:, -1] * 7 + (ids.shape[1] if self.by_length else 0)) % self.table.shape[0]
        return self.table[key]


def _generate(monkeypatch, step, **kw):
    m = BertForMaskedLM.__new__(BertForMaskedLM)
    torch.nn.Module.__init__(m)
    monkeypatch.setattr(BertForMaskedLM, "_model_step", lambda self, *a, **k: step)
    ids = torch.tensor([[1, 2, 3], [1, 2, 3], [4, 4, 5]])
    return m.generate(input_ids=ids, attention_mask=torch.ones(3, 3, 3, dtype=torch.long), max_new_tokens=12, num_beams=3,
                      eos_token_id=SEP % step.vocab, pad_token_id=PAD, length_penalty=0.6, **kw)


def _new_tokens(row, eos, start=3):
    toks = row.tolist()[start:]
    return toks[:toks.index(eos)] if eos in toks else [t for t in toks]


def test_host_generate_with_processors_over_scripted_logits(monkeypatch):
    step = _ScriptedStep()
    eos = SEP % step.vocab
    plain = _generate(monkeypatch, step)
    assert torch.equal(plain, _generate(monkeypatch, step, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0,
                                        device_search=False, done_check_every=1))
    assert any(len(_new_tokens(r, eos)) < 4 for r in plain), "the stub's eos logit is the largest: without a minimum rows end early"
    out = _generate(monkeypatch, step, min_new_tokens=4)
    assert all(len(_new_tokens(r, eos)) >= 4 for r in out)
    assert all(len(_new_tokens(r, eos, 0)) >= 9 for r in _generate(monkeypatch, step, min_length=9))
    # without eos the rows run to the full length; the stub's logits depend on the last token, so bigrams repeat unless banned
    free = _ScriptedStep(vocab=24, eos_gap=-50.0, by_length=False)
    eos = SEP % free.vocab
    rep = _generate(monkeypatch, free)
    big = lambda row: [tuple(row[i:i + 2]) for i in range(len(row) - 1)]
    assert any(len(set(big(r.tolist()))) < len(big(r.tolist())) for r in rep), "the case was meant to repeat a bigram"
    out = _generate(monkeypatch, free, no_repeat_ngram_size=2)
    for r in out:
        row = r.tolist()
        row = row[:row.index(eos)] if eos in row else row
        assert len(set(big(row))) == len(big(row)), row
    one = _generate(monkeypatch, free, no_repeat_ngram_size=1, repetition_penalty=1.5)
    for r in one:
        row = r.tolist()[2:]            # (the prompt [4, 4, 5] repeats a token itself)
        row = row[:row.index(eos)] if eos in row else row
        assert len(set(row)) == len(row), row


def test_generate_argument_errors():
    m = BertForMaskedLM.__new__(BertForMaskedLM)
    torch.nn.Module.__init__(m)
    ids, mask = torch.full((2, 1), CLS), torch.ones(2, 1, 1, dtype=torch.long)
    call = lambda **kw: m.generate(input_ids=ids, attention_mask=mask, **kw)
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(no_repeat_ngram_size=-1), dict(min_length=-2),
                dict(min_new_tokens=-1), dict(device_search=True, num_beams=9), dict(done_check_every=0)):
        with pytest.raises(ValueError):
            call(**bad)
    for beam_only in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_length=3), dict(min_new_tokens=3),
                      dict(device_search=True), dict(done_check_every=2)):
        with pytest.raises(ValueError, match="beam search only"):
            call(do_sample=True, **beam_only)
    with pytest.raises(TypeError):
        call(temperature=0.7)
    with pytest.raises(TypeError):
        call(early_stopping=True)


def test_beam_entry_points_declared_exported_and_bound():
    from mico_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mico_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("mico_beam_topk", 19), ("mico_beam_step", 2), ("mico_beam_finalize", 2), ("mico_beam_params_layout", 2)):
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, hdr, re.S)
        assert decl, f"{name} is not declared in include/mico_hip.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name])
        assert hasattr(lib, name), f"{name} is not exported"
    l = _lib.lib()
    assert l.mico_version() == _lib.ABI_VERSION >= 122
    # mico_beam_params: header order = ctypes order = compiled layout
    body = re.search(r"typedef struct mico_beam_params \{(.*?)\} mico_beam_params;", hdr, re.S).group(1)
    names = [re.search(r"(\w+)\s*$", f.strip()).group(1) for f in body.split(";") if f.strip()]
    assert names == [n for n, _ in _lib.BeamParams._fields_]
    n = l.mico_beam_params_layout(None, 0)
    buf = (ctypes.c_int * n)()
    assert l.mico_beam_params_layout(buf, n) == n and buf[n - 1] == -1
    assert buf[0] == ctypes.sizeof(_lib.BeamParams)
    assert list(buf[1:n - 1]) == [getattr(_lib.BeamParams, f).offset for f, _ in _lib.BeamParams._fields_]
    # shape limits are refused before any launch (no GPU is touched: the checks are host code)
    f = ctypes.c_void_p(8)
    bad = lambda sets, nb, V, ids, cur: l.mico_beam_topk(f, V, sets, nb, V, f, None, ids, 512, cur, 1.0, 0, 0, -1, f, f, f, f, None)
    assert bad(1, 9, 100, None, 0) == -22 and bad(1, 0, 100, None, 0) == -22      # nb
    assert bad(1, 4, 7, None, 0) == -22                                          # V < 2 nb
    assert bad(1, 2, 65537, f, 4) == -22 and bad(1, 2, 300, f, 513) == -22       # processors: V, cur_len
    assert l.mico_beam_step(None, None) == -22 and l.mico_beam_finalize(None, None) == -22
    p = _lib.BeamParams()
    p.sets, p.nb, p.cur_len, p.max_length = 1, 9, 1, 4
    assert l.mico_beam_step(ctypes.byref(p), None) == -22
    with pytest.raises(_lib.MicoHipError):
        ops.beam_topk(torch.zeros(3, 50), torch.zeros(3), 3)
    assert ops.BEAM_NB_MAX == 8 and hasattr(ops, "beam_step") and hasattr(ops, "beam_finalize")
