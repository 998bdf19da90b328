"""Device-side sampling decode, the parts that need no GPU: the pure-torch warper function against transformers' warpers and against
hand-written cases, BertForMaskedLM.sample(device_search=False) over scripted logits (against generate(do_sample=True, top_k=k), and with the
logits processors), sample()'s argument errors, and the C ABI of mico_warp_sample."""
import ctypes
import os
import re

import pytest
import torch

from mico_amd.model.bert import BertForMaskedLM, apply_logits_warpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLS, SEP, PAD = 101, 102, 0
NEG_INF = float("-inf")


def _mass_before(s64, kept_topk):
    """float64: per column the probability mass of the columns ranked ahead of it, under the softmax over the top-k survivors"""
    ranked, order = torch.sort(s64.masked_fill(~kept_topk, NEG_INF), dim=-1, descending=True, stable=True)
    p = torch.softmax(ranked, dim=-1)
    before = torch.cat([torch.zeros_like(p[:, :1]), p.cumsum(-1)[:, :-1]], dim=-1)
    return torch.zeros_like(before).scatter_(1, order, before)


@pytest.mark.parametrize("V", [70, 257, 1000])
@pytest.mark.parametrize("k", [1, 10, 64])
def test_warper_function_matches_transformers(V, k):
    """random rows without ties.  The masks are compared in float64 (both sides' sums are then exact to ~1e-13, far inside the asserted 1e-6
    margin of every rank's mass to top_p); the temperature and top-k stages, which involve no sum, also bit for bit in fp32."""
    wr = pytest.importorskip("transformers.generation.logits_process")
    g = torch.Generator().manual_seed(100 * V + k)
    scores = torch.randn(6, V, generator=g)
    assert all(len(set(r.tolist())) == V for r in scores), "the case was meant to have no ties"
    ids = torch.zeros(6, 1, dtype=torch.long)
    for p in (0.5, 0.9, 1.0):
        for T in (0.7, 1.0, 1.5):
            s64 = scores.double()
            ref = wr.TemperatureLogitsWarper(T)(ids, s64.clone()) if T != 1.0 else s64.clone()
            ref = wr.TopKLogitsWarper(top_k=k)(ids, ref)
            topk_kept = ref > NEG_INF
            ref = wr.TopPLogitsWarper(top_p=p)(ids, ref)
            margin = float((_mass_before(s64 / T, topk_kept)[topk_kept] - p).abs().min())
            assert margin > 1e-6, f"a rank's mass lies {margin:.2e} from top_p = {p}: choose another seed"
            got, kept = apply_logits_warpers(s64, k, p, T)
            assert torch.equal(got == NEG_INF, ref == NEG_INF), (p, T)
            assert torch.equal(kept, got > NEG_INF)
            assert torch.equal(got[kept], ref[kept])
            # fp32: temperature and top-k alone are exact statements
            ref32 = wr.TopKLogitsWarper(top_k=k)(ids, wr.TemperatureLogitsWarper(T)(ids, scores.clone()) if T != 1.0 else scores.clone())
            got32, kept32 = apply_logits_warpers(scores, k, 1.0, T)
            assert torch.equal(got32 == NEG_INF, ref32 == NEG_INF)
            assert torch.equal(got32[kept32].view(torch.int32), ref32[kept32].view(torch.int32))
            assert torch.equal(kept32.sum(-1), torch.full((6,), min(k, V)))
    # top_k = 0: the nucleus over the whole row
    for p in (0.5, 0.9):
        s64 = scores.double()
        ref = wr.TopPLogitsWarper(top_p=p)(ids, s64.clone())
        assert float((_mass_before(s64, torch.ones_like(s64, dtype=torch.bool)) - p).abs().min()) > 1e-6
        got, kept = apply_logits_warpers(s64, 0, p, 1.0)
        assert torch.equal(got == NEG_INF, ref == NEG_INF) and torch.equal(kept, got > NEG_INF)


def test_warper_function_hand_written_cases():
    s = torch.tensor([[1.0, 3.0, 2.0, 3.0, 0.5, 2.0, 3.0]])
    # rank 0 is kept whatever top_p says (min_tokens_to_keep = 1): the first of the three 3.0
    got, kept = apply_logits_warpers(s, 0, 1e-6, 1.0)
    assert kept.tolist() == [[False, True, False, False, False, False, False]]
    assert got.tolist() == [[NEG_INF, 3.0, NEG_INF, NEG_INF, NEG_INF, NEG_INF, NEG_INF]]
    # ties at the k-th score go by ascending column
    assert apply_logits_warpers(s, 2, 1.0, 1.0)[1].tolist() == [[False, True, False, True, False, False, False]]
    assert apply_logits_warpers(s, 4, 1.0, 1.0)[1].tolist() == [[False, True, True, True, False, False, True]]
    assert apply_logits_warpers(s, 64, 1.0, 1.0)[1].all()
    # temperature divides; the input is not modified
    got, _ = apply_logits_warpers(s, 0, 1.0, 0.7)
    assert torch.equal(got, s / torch.tensor(0.7)) and s[0, 0] == 1.0
    # top_p over three candidates of probability 0.5, 0.25, 0.25: masses ahead 0, 0.5, 0.75
    e = torch.log(torch.tensor([[0.25, 0.5, 0.25]], dtype=torch.float64))
    assert apply_logits_warpers(e, 0, 0.5, 1.0)[1].tolist() == [[False, True, False]]      # 0.5 < 0.5 is false
    assert apply_logits_warpers(e, 0, 0.6, 1.0)[1].tolist() == [[True, True, False]]       # the first of the two equal ones
    assert apply_logits_warpers(e, 0, 0.8, 1.0)[1].tolist() == [[True, True, True]]
    # a row of -inf except one entry, and a row without any finite entry: -inf is never kept
    lone = torch.full((2, 9), NEG_INF)
    lone[0, 4] = -2.0
    for k, p in ((0, 1.0), (3, 1.0), (0, 0.3), (3, 0.3)):
        got, kept = apply_logits_warpers(lone, k, p, 1.3)
        assert kept.tolist() == [[c == 4 for c in range(9)], [False] * 9]
        assert got[0, 4] == torch.tensor(-2.0) / torch.tensor(1.3) and bool((got[1] == NEG_INF).all())


class _ScriptedStep:
    """next_token_logits from a seeded table (tests/test_beam_device_cpu.py): the row's logits depend on its last token and its length only"""

    def __init__(self, vocab=40, eos_gap=1.0, seed=5, by_length=True):
        g = torch.Generator().manual_seed(seed)
        self.table = 2 * torch.randn(64, vocab, generator=g)
        self.table[:, SEP % vocab] = self.table.max(dim=1).values + eos_gap
        self.vocab, self.by_length = vocab, by_length

    def next_token_logits(self, ids, parent=None):
        key = (ids[:, -1] * 7 + (ids.shape[1] if self.by_length else 0)) % self.table.shape[0]
        return self.table[key]


def _decode(monkeypatch, step, how, **kw):
    m = BertForMaskedLM.__new__(BertForMaskedLM)
    torch.nn.Module.__init__(m)
    monkeypatch.setattr(BertForMaskedLM, "_model_step", lambda self, *a, **k: step)
    ids = torch.tensor([[1, 2, 3], [1, 2, 3], [4, 4, 5]])
    return getattr(m, how)(input_ids=ids, attention_mask=torch.ones(3, 3, 3, dtype=torch.long), max_new_tokens=12,
                           eos_token_id=SEP % step.vocab, pad_token_id=PAD, **kw)


def _new_tokens(row, eos, start=3):
    toks = row.tolist()[start:]
    return toks[:toks.index(eos)] if eos in toks else toks


def test_host_sample_over_scripted_logits(monkeypatch):
    step = _ScriptedStep()
    eos = SEP % step.vocab
    g = torch.Generator().manual_seed(2)
    for trial in range(4):
        noise = torch.rand(6, 12, generator=g)
        for k in (1, 5, 10):      # only top_k set: generate(do_sample=True, top_k=k), id for id
            ref = _decode(monkeypatch, step, "generate", do_sample=True, top_k=k, sample_noise=noise, num_return_sequences=2)
            out, lp = _decode(monkeypatch, step, "sample", top_k=k, sample_noise=noise, num_return_sequences=2, device_search=False,
                              return_logprobs=True)
            assert torch.equal(out, ref), (trial, k)
            assert lp.shape == (6, out.shape[1] - 3) and bool((lp <= 0).all())
            fin = torch.tensor([[t >= len(_new_tokens(r, eos)) + 1 for t in range(lp.shape[1])] for r in out])
            assert bool((lp[fin] == 0).all()), "finished rows carry log-prob 0"
            if k == 1:
                assert bool((lp == 0).all())
    noise = torch.rand(3, 12, generator=g)
    plain = _decode(monkeypatch, step, "sample", top_k=10, sample_noise=noise, device_search=False)
    assert any(len(_new_tokens(r, eos)) < 4 for r in plain), "the stub's eos logit is the largest: without a minimum rows end early"
    out = _decode(monkeypatch, step, "sample", top_k=10, sample_noise=noise, device_search=False, min_new_tokens=4)
    assert all(len(_new_tokens(r, eos)) >= 4 for r in out)
    assert all(len(_new_tokens(r, eos, 0)) >= 9 for r in _decode(monkeypatch, step, "sample", sample_noise=noise, device_search=False, min_length=9))
    # a low temperature with a narrow nucleus is the argmax chain
    greedy = _decode(monkeypatch, step, "sample", top_k=1, sample_noise=noise, device_search=False)
    assert torch.equal(_decode(monkeypatch, step, "sample", top_p=0.05, temperature=0.05, sample_noise=noise, device_search=False), greedy)
    # without eos the rows run on; the stub's logits depend on the last token, so bigrams repeat unless banned
    free = _ScriptedStep(vocab=24, eos_gap=-50.0, by_length=False)
    eos = SEP % free.vocab
    big = lambda row: [tuple(row[i:i + 2]) for i in range(len(row) - 1)]
    rep = _decode(monkeypatch, free, "sample", top_k=2, sample_noise=noise, device_search=False)
    assert any(len(set(big(r.tolist()))) < len(big(r.tolist())) for r in rep), "the case was meant to repeat a bigram"
    for kw in (dict(top_k=2), dict(top_p=0.6, temperature=0.8)):
        out = _decode(monkeypatch, free, "sample", sample_noise=noise, device_search=False, no_repeat_ngram_size=2, **kw)
        for r in out:
            row = r.tolist()
            row = row[:row.index(eos)] if eos in row else row
            assert len(set(big(row))) == len(big(row)), row


def test_sample_argument_errors():
    m = BertForMaskedLM.__new__(BertForMaskedLM)
    torch.nn.Module.__init__(m)
    ids, mask = torch.full((2, 1), CLS), torch.ones(2, 1, 1, dtype=torch.long)
    for bad in (dict(top_k=-1), dict(top_k=65), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(temperature=0.0),
                dict(temperature=-1.0), dict(temperature=float("nan")), dict(repetition_penalty=0.0), dict(no_repeat_ngram_size=-1),
                dict(min_length=-2), dict(min_new_tokens=-1), dict(max_new_tokens=0), dict(num_return_sequences=0), dict(done_check_every=0),
                dict(sample_noise=torch.zeros(2, 3), max_new_tokens=4)):
        for dev in (True, False):
            with pytest.raises(ValueError):
                m.sample(input_ids=ids, attention_mask=mask, device_search=dev, **bad)
    with pytest.raises(TypeError):
        m.sample(input_ids=ids, attention_mask=mask, num_beams=3)


def test_warp_sample_entry_points_declared_exported_and_bound():
    from mico_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mico_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("mico_warp_sample", 2), ("mico_warp_sample_params_layout", 2)):
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, hdr, re.S)
        assert decl, f"{name} is not declared in include/mico_hip.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name])
        assert hasattr(lib, name), f"{name} is not exported"
    l = _lib.lib()
    assert l.mico_version() == _lib.ABI_VERSION >= 124
    # mico_warp_sample_params: header order = ctypes order = compiled layout
    body = re.search(r"typedef struct mico_warp_sample_params \{(.*?)\} mico_warp_sample_params;", hdr, re.S).group(1)
    names = [re.search(r"(\w+)\s*$", f.strip()).group(1) for f in body.split(";") if f.strip()]
    assert names == [n for n, _ in _lib.WarpSampleParams._fields_]
    n = l.mico_warp_sample_params_layout(None, 0)
    buf = (ctypes.c_int * n)()
    assert l.mico_warp_sample_params_layout(buf, n) == n and buf[n - 1] == -1
    assert buf[0] == ctypes.sizeof(_lib.WarpSampleParams)
    assert list(buf[1:n - 1]) == [getattr(_lib.WarpSampleParams, f).offset for f, _ in _lib.WarpSampleParams._fields_]
    # the limits are refused before any launch (no GPU is touched: the checks are host code)
    f = ctypes.c_void_p(8)

    def rc(**kw):
        p = _lib.WarpSampleParams()
        p.logits, p.u, p.token, p.ld, p.rows, p.V = f, f, f, 100, 2, 100
        p.top_p, p.temperature, p.rep_penalty, p.eos_id = 1.0, 1.0, 1.0, -1
        for key, v in kw.items():
            setattr(p, key, v)
        return l.mico_warp_sample(ctypes.byref(p), None)

    assert l.mico_warp_sample(None, None) == -22
    for bad in (dict(top_k=-1), dict(top_k=65), dict(top_p=0.0), dict(top_p=1.0001), dict(top_p=float("nan")), dict(temperature=0.0),
                dict(temperature=-2.0), dict(temperature=float("nan")), dict(V=0), dict(ld=99), dict(ids=f, ld_ids=600, V=65537, ld=65537),
                dict(ids=f, ld_ids=600, cur_len=513), dict(ids=f, ld_ids=600, cur_len=-1), dict(ids=f, ld_ids=8, cur_len=8, append=1),
                dict(logits=None), dict(token=None)):
        assert rc(**bad) == -22, bad
        assert b"mico_warp_sample" in l.mico_last_error_string()
    assert rc(rows=0) == 0 and rc(rows=0, top_k=64, top_p=0.5, temperature=0.1, ids=f, ld_ids=9, cur_len=8, append=1) == 0
    with pytest.raises(_lib.MicoHipError):
        ops.warp_sample(torch.zeros(3, 50), torch.zeros(3))      # CPU tensors: no fallback
    assert ops.SAMPLE_TOPK_MAX == 64
