"""Device-side sampling decode on the GPU: mico_warp_sample against a float64 reference (apply_logits_processors, then apply_logits_warpers, on
float64 copies) in top-k mode, in nucleus mode and with the logits processors, its finished-row bookkeeping and its limits, and
BertForMaskedLM.sample against generate(do_sample=True), the CPU oracle and its own host path, with the number of host reads of a decode."""
import math

import pytest
import torch

from common import build_model
from mico_amd import ops, runtime
from mico_amd._lib import MicoHipError
from mico_amd.model.bert import apply_logits_processors, apply_logits_warpers
from oracle import mico_oracle as O
from test_beam_device_gpu import _count_syncs

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
TOL = 3e-5       # log-prob: a few fp32 roundings at |score| <= 64 (tests/test_beam_device_gpu.py derives the same bound)
WORST = {}
# seed offsets chosen so that the conditions asserted on the references hold (a decided nucleus boundary, few tokens in the band)
SEED_TOPK, SEED_NUCLEUS, SEED_PROC = 14000000, 0, 1000000


def _inputs(rows, V, ld, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.full((rows, ld), 50.0)         # (past V: larger than anything inside - a read past the row's end would show)
    logits[:, :V] = 3 * torch.randn(rows, V, generator=g)
    return logits


def _reference(x, T, k, p, ids=None, eos=None, **proc):
    """x: fp32 [rows, V].  (s32: the processed scores / T in fp32, what the kernel ranks; warped float64, -inf outside the kept set; kept)"""
    x32 = apply_logits_processors(x, ids, eos, **proc) if ids is not None else x
    x64 = apply_logits_processors(x.double(), ids, eos, **proc) if ids is not None else x.double()
    s32 = apply_logits_warpers(x32, 0, 1.0, T)[0]
    warped, kept = apply_logits_warpers(x64, k, p, T)
    return s32, warped, kept


def _ranked(warped, kept):
    """(order [rows, V] by descending score, n_kept [rows], probabilities of the kept ranks float64 [rows, V], mass ahead of each rank)"""
    ranked, order = torch.sort(warped, dim=-1, descending=True, stable=True)
    pr = torch.softmax(ranked, dim=-1)
    return order, kept.sum(-1), pr, torch.cat([torch.zeros_like(pr[:, :1]), pr.cumsum(-1)[:, :-1]], dim=-1)


def _pick_targets(n, pr, before, turn, floor=2e-3):
    """per row a target rank among the ranks holding >= floor of the kept mass - the first, the last, a middle one in turn - and u = the
    midpoint of its CDF interval"""
    ranks, us = [], []
    for r in range(pr.shape[0]):
        elig = [q for q in range(int(n[r])) if float(pr[r, q]) >= floor]
        q = (elig[0], elig[-1], elig[len(elig) // 2])[(turn + r) % 3]
        ranks.append(q)
        us.append(float(before[r, q] + pr[r, q] / 2))
    u = torch.tensor(us, dtype=torch.float64).float()
    assert bool((u < 1).all())
    return torch.tensor(ranks), u


def _check_topk_mode(cuda, x, V, k, p, T, turn, ids=None, eos=None, **proc):
    """one call in top-k mode against the reference; returns the reference's kept mask"""
    xv = x[:, :V]
    s32, warped, kept = _reference(xv, T, k, p, ids, eos, **proc)
    order, n, pr, before = _ranked(warped, kept)
    kk = min(k, V)
    head = torch.sort(s32, dim=-1, descending=True).values[:, :kk + 1]
    gaps = head[:, :-1] - head[:, 1:]
    assert bool((gaps[torch.isfinite(gaps)] > 0).all()), "the fp32 scores of the best k + 1 were meant to differ"
    if p < 1.0:      # the nucleus boundary of the reference is decided: the mass ahead of every top-k survivor is > 1e-3 from top_p
        fullk = _ranked(*apply_logits_warpers(apply_logits_processors(xv.double(), ids, eos, **proc) if ids is not None else xv.double(), k, 1.0, T))
        clear = (fullk[3][:, :kk] - p).abs()
        assert float(clear[torch.isfinite(clear)].min()) > 1e-3, f"nucleus boundary {float(clear.min()):.2e} from top_p: choose another seed"
    ranks, u = _pick_targets(n, pr, before, turn)
    rows = torch.arange(x.shape[0])
    want_tok = order[rows, ranks]
    want_lp = pr[rows, ranks].log()
    kw = dict(ids=ids.to(cuda), eos_token_id=eos, **proc) if ids is not None else {}
    tok, lp, nk, km = (t.cpu() for t in ops.warp_sample(x.to(cuda)[:, :V], u.to(cuda), top_k=k, top_p=p, temperature=T, **kw))
    err = float((lp.double() - want_lp).abs().max())
    WORST["topk"] = max(WORST.get("topk", 0.0), err)
    print(f"V {V} k {k} p {p} T {T}: n_kept {n.tolist()} ranks {ranks.tolist()} largest log-prob error {err:.3e} (worst so far {WORST['topk']:.3e}, "
          f"tolerance {TOL:.0e})")
    assert tok.tolist() == want_tok.tolist()
    assert nk.tolist() == n.tolist()
    assert torch.equal(km, s32[rows, order[rows, n - 1]]), "kept_min is the fp32 processed score of the last kept rank"
    assert err <= TOL
    return kept


@pytest.mark.parametrize("rows,V,ld,k", [(1, 70, 70, 1), (3, 257, 264, 10), (4, 30522, 30528, 10), (2, 1000, 1000, 64), (2, 30522, 30522, 50),
                                         (2, 36000, 36003, 10)])      # (the last: a row too long to be staged in LDS)
def test_top_k_mode_against_float64(cuda, rows, V, ld, k):
    turn = 0
    for T in (1.0, 0.7):
        for p in (1.0, 0.8):
            x = _inputs(rows, V, ld, SEED_TOPK + 7 * V + k + int(10 * T) + int(100 * p))
            _check_topk_mode(cuda, x, V, k, p, T, turn)
            turn += 1


def test_top_k_mode_ties_go_by_column(cuda):
    x = torch.randn(2, 300, generator=torch.Generator().manual_seed(1))
    x[:, [250, 17, 200, 3]] = 9.0
    x[:, [40, 41]] = 8.0
    for k, cols in ((2, [3, 17]), (3, [3, 17, 200]), (5, [3, 17, 200, 250, 40])):
        for i, c in enumerate(cols):      # u in the middle of rank i's interval
            w = torch.tensor([math.exp(float(x[0, j]) - 9.0) for j in cols], dtype=torch.float64)
            u = float((w[:i].sum() + w[i] / 2) / w.sum())
            tok, lp, nk, km = ops.warp_sample(x.to(cuda), torch.full((2,), u, device=cuda), top_k=k)
            assert tok.tolist() == [c, c] and nk.tolist() == [k, k] and km.tolist() == [float(x[0, cols[-1]])] * 2
            assert abs(float(lp[0]) - math.log(float(w[i] / w.sum()))) <= TOL
    _, kept = apply_logits_warpers(x, 5, 1.0, 1.0)
    assert kept[0].nonzero().flatten().tolist() == [3, 17, 40, 200, 250]


DELTA = 1e-4      # of the total: the band in which the mass sums may place the nucleus boundary (their own error stays below 1.6e-5)


def _mass_before(s64):
    ranked, order = torch.sort(s64, dim=-1, descending=True, stable=True)
    pr = torch.softmax(ranked, dim=-1)
    before = torch.cat([torch.zeros_like(pr[:, :1]), pr.cumsum(-1)[:, :-1]], dim=-1)
    return torch.zeros_like(before).scatter_(1, order, before)


def _check_draw_in_column_order(cuda, x, V, s64, kept_set, turn, **kw):
    """the draw over the kernel's own kept set: float64 CDF in column order, u in the middle of a kept column holding >= 1e-3 of the kept mass"""
    w = torch.softmax(s64.masked_fill(~kept_set, NEG_INF), dim=-1)
    cdf = w.cumsum(-1)
    cols, us = [], []
    for r in range(x.shape[0]):
        elig = (w[r] >= 1e-3).nonzero().flatten().tolist()
        c = (elig[0], elig[-1], elig[len(elig) // 2])[(turn + r) % 3]
        cols.append(c)
        us.append(float(cdf[r, c] - w[r, c] / 2))
    u = torch.tensor(us, dtype=torch.float64).float()
    tok, lp, nk, km = (t.cpu() for t in ops.warp_sample(x.to(cuda)[:, :V], u.to(cuda), **kw))
    want_lp = w[torch.arange(x.shape[0]), torch.tensor(cols)].log()
    err = float((lp.double() - want_lp).abs().max())
    WORST["nucleus"] = max(WORST.get("nucleus", 0.0), err)
    print(f"   draw: columns {cols} largest log-prob error {err:.3e} (worst so far {WORST['nucleus']:.3e}, tolerance {TOL:.0e})")
    assert tok.tolist() == cols
    assert err <= TOL
    return nk, km


@pytest.mark.parametrize("rows,V,ld", [(2, 70, 70), (3, 257, 264), (4, 30522, 30528), (2, 36000, 36003)])      # (the last: not staged in LDS)
def test_nucleus_mode_against_float64(cuda, rows, V, ld):
    turn = 0
    for p in (0.5, 0.9):
        for T in (1.0, 1.5):
            x = _inputs(rows, V, ld, SEED_NUCLEUS + 11 * V + int(10 * T) + int(100 * p))
            s32, _, _ = _reference(x[:, :V], T, 0, 1.0)
            s64 = x[:, :V].double() / T
            before = _mass_before(s64)
            must, never = before < p - DELTA, before > p + DELTA
            band = int((~must & ~never).sum(-1).max())
            assert band <= 16, f"{band} tokens inside the band: choose another seed"
            _, _, nk, km = (t.cpu() for t in ops.warp_sample(x.to(cuda)[:, :V], torch.full((rows,), 0.5, device=cuda), top_p=p, temperature=T))
            kept_set = s32 >= km[:, None]
            print(f"V {V} p {p} T {T}: n_kept {nk.tolist()} certain {must.sum(-1).tolist()} in the band {band}")
            assert bool((kept_set | ~must).all()), "a token whose mass ahead is below top_p - delta is missing"
            assert not bool((kept_set & never).any()), "a token whose mass ahead is above top_p + delta was kept"
            assert nk.tolist() == kept_set.sum(-1).tolist()
            nk2, km2 = _check_draw_in_column_order(cuda, x, V, s64, kept_set, turn, top_p=p, temperature=T)
            assert torch.equal(nk2, nk) and torch.equal(km2, km), "the kept set does not depend on u"
            turn += 1


@pytest.mark.parametrize("V", [300, 30522])
def test_nucleus_mode_designed_rows(cuda, V):
    """30 head columns at random positions with geometric probabilities over a uniform tail of total mass 0.02; top_p between two head
    tokens with >= 5e-3 of clearance on either side: the kept set is exact"""
    g = torch.Generator().manual_seed(V)
    rows = 3
    x = torch.empty(rows, V)
    head = torch.stack([torch.randperm(V, generator=g)[:30] for _ in range(rows)])
    ph = 0.8 ** torch.arange(30, dtype=torch.float64)
    ph = 0.98 * ph / ph.sum()
    x[:] = math.log(0.02 / (V - 30))
    x.scatter_(1, head, ph.log().float().repeat(rows, 1))
    pr = torch.softmax(x.double(), dim=-1)
    for turn, j in enumerate((0, 5, 12)):
        cum = pr.gather(1, head).cumsum(-1)                     # head ranks are the row's ranks 0 .. 29
        p_row = cum[:, j] - pr.gather(1, head)[:, j] / 2        # the mass ahead of rank j < top_p < the mass ahead of rank j + 1
        assert float(p_row.max() - p_row.min()) < 1e-6
        p = float(p_row[0])
        before = _mass_before(x.double())
        assert float((before - p).abs().min()) >= 5e-3
        want = before < p
        assert want.sum(-1).tolist() == [j + 1] * rows
        _, _, nk, km = (t.cpu() for t in ops.warp_sample(x.to(cuda), torch.full((rows,), 0.3, device=cuda), top_p=p))
        kept_set = x >= km[:, None]
        assert torch.equal(kept_set, want) and nk.tolist() == [j + 1] * rows
        assert torch.equal(km, x.gather(1, head[:, j:j + 1])[:, 0])
        _check_draw_in_column_order(cuda, x, V, x.double(), kept_set, turn, top_p=p)


@pytest.mark.parametrize("rows,V,ld", [(3, 257, 264), (4, 30522, 30528)])
def test_trivial_point_is_the_full_softmax_draw(cuda, rows, V, ld):
    """top_k = 0, top_p = 1, temperature 1, no processors: mico_vocab_sample's rule, checked against the float64 CDF"""
    x = _inputs(rows, V, ld, 5 * V)
    x[:, 0] = NEG_INF                       # the first candidate is column 1
    x[:, V - 3:V] = NEG_INF                 # the last one with a weight is column V - 4 or before
    x[1, 1] = NEG_INF
    xg = x.to(cuda)[:, :V]
    s64 = x[:, :V].double()
    finite = torch.isfinite(x[:, :V])
    tok, lp, nk, km = (t.cpu() for t in ops.warp_sample(xg, torch.zeros(rows, device=cuda)))
    assert tok.tolist() == [2 if r == 1 else 1 for r in range(rows)], "u = 0: the first kept candidate"
    assert nk.tolist() == finite.sum(-1).tolist()
    assert torch.equal(km, x[:, :V].masked_fill(~finite, float("inf")).min(-1).values)
    hi = torch.full((rows,), 1.0).nextafter(torch.zeros(rows))
    tok, lp, _, _ = (t.cpu() for t in ops.warp_sample(xg, hi.to(cuda)))
    w32 = torch.exp(x[:, :V] - x[:, :V].max(-1, keepdim=True).values)
    assert bool((w32[torch.arange(rows), tok] > 0).all()) and bool((tok <= V - 4).all()), "u next to 1: a candidate with a weight"
    assert bool(torch.isfinite(lp).all())
    for turn in range(3):
        _check_draw_in_column_order(cuda, x, V, s64, finite, turn)
    # no finite score at all: no distribution
    dead = torch.full((2, V), NEG_INF, device=cuda)
    for kw in (dict(), dict(top_k=5), dict(top_p=0.5)):
        tok, lp, nk, km = (t.cpu() for t in ops.warp_sample(dead, torch.full((2,), 0.4, device=cuda), **kw))
        assert tok.tolist() == [0, 0] and nk.tolist() == [0, 0] and bool((lp == NEG_INF).all()) and bool((km == float("inf")).all())


def _processor_ids(logits, V):
    """12 ids per row drawn from the row's own best tokens, so that the processors hit candidates (tests/test_beam_device_gpu.py): repeated
    bigrams and trigrams, a pad in the middle and one id >= V (ignored); t11 and t12 lie just outside the best ten, where a penalty below 1
    lifts them in; the last ids are (t0, t1), which t2 and t3 have followed before"""
    t = logits[:, :V].topk(14, dim=1).indices
    pick = [0, 1, 2, 0, 1, 3, -1, -2, 11, 12, 0, 1]
    cols = []
    for p in pick:
        cols.append(t[:, p] if p >= 0 else torch.full_like(t[:, 0], 0 if p == -1 else V + 5))
    return torch.stack(cols, dim=1).contiguous()


@pytest.mark.parametrize("V", [300, 30522])
def test_processors_against_float64(cuda, V):
    rows, eos, k = 3, 102, 10
    x = _inputs(rows, V, V + 6, SEED_PROC + 4242 + V)
    ids = _processor_ids(x, V)
    x[:, eos] = 14.0                                    # eos is every row's best token (and not among the ids): the ban changes the kept set
    plain = _check_topk_mode(cuda, x, V, k, 1.0, 1.0, 0)
    turn = 1
    for name, kw in (("penalty", dict(repetition_penalty=1.3)), ("penalty < 1", dict(repetition_penalty=0.8)),
                     ("bigrams", dict(no_repeat_ngram_size=2)), ("unigrams", dict(no_repeat_ngram_size=1)), ("eos", dict(ban_eos=True)),
                     ("all", dict(repetition_penalty=1.3, no_repeat_ngram_size=3, ban_eos=True))):
        for T, p in ((1.0, 1.0), (0.7, 0.8)):
            print(name, end=": ")
            kept = _check_topk_mode(cuda, x, V, k, p, T, turn, ids=ids, eos=eos, **kw)
            turn += 1
            if p == 1.0:
                assert not torch.equal(kept, plain), f"{name}: the processor was meant to change the kept set"
                # the kept set itself: the best ten differ in fp32, so it is s >= kept_min
                s32 = _reference(x[:, :V], T, k, p, ids, eos, **kw)[0]
                km = ops.warp_sample(x.to(cuda)[:, :V], torch.full((rows,), 0.5, device=cuda), top_k=k, ids=ids.to(cuda), eos_token_id=eos, **kw)[3]
                assert torch.equal(s32 >= km.cpu()[:, None], kept)
    # nucleus mode with all of them: the band test of test_nucleus_mode_against_float64 over the processed scores
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, ban_eos=True)
    s32, _, _ = _reference(x[:, :V], 0.7, 0, 1.0, ids, eos, **kw)
    s64 = apply_logits_processors(x[:, :V].double(), ids, eos, **kw) / 0.7
    before = _mass_before(s64)
    must, never = (before < 0.9 - DELTA) & torch.isfinite(s64), (before > 0.9 + DELTA) | ~torch.isfinite(s64)
    assert int((~must & ~never).sum(-1).max()) <= 16
    run = dict(top_p=0.9, temperature=0.7, ids=ids.to(cuda), eos_token_id=eos, **kw)
    _, _, nk, km = (t.cpu() for t in ops.warp_sample(x.to(cuda)[:, :V], torch.full((rows,), 0.5, device=cuda), **run))
    kept_set = s32 >= km[:, None]
    assert bool((kept_set | ~must).all()) and not bool((kept_set & never).any()) and nk.tolist() == kept_set.sum(-1).tolist()
    _check_draw_in_column_order(cuda, x, V, s64, kept_set, 0, **run)
    # ids as a view with a row stride, cur_len shorter than the view
    wide = torch.zeros(rows, 40, dtype=torch.long, device=cuda)
    wide[:, :12] = ids.to(cuda)
    u = torch.full((rows,), 0.37, device=cuda)
    a = ops.warp_sample(x.to(cuda)[:, :V], u, top_k=k, ids=wide[:, :12], repetition_penalty=1.3, no_repeat_ngram_size=2)
    b = ops.warp_sample(x.to(cuda)[:, :V], u, top_k=k, ids=ids.to(cuda), repetition_penalty=1.3, no_repeat_ngram_size=2)
    c = ops.warp_sample(x.to(cuda)[:, :V], u, top_k=k, ids=wide, cur_len=12, repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in zip(a, b, c))


def test_bookkeeping(cuda):
    rows, V, eos, pad, cur = 6, 300, 102, 5, 4
    x = _inputs(rows, V, V, 99)
    x[[0, 3], eos] = 60.0                                   # rows 0 and 3 draw eos whatever u is
    x[[1, 2], eos] = NEG_INF
    x[5, eos] = NEG_INF
    u = torch.tensor([0.1, 0.5, 0.9, 0.99, 0.3, 0.6], device=cuda)
    for kw in (dict(top_k=5), dict(top_p=0.9)):
        unfinished = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8, device=cuda)
        not_done = torch.tensor([4], dtype=torch.int32, device=cuda)
        ids = torch.full((rows, 9), -7, dtype=torch.long, device=cuda)
        ids[:, :cur] = torch.arange(200, 200 + cur, device=cuda)
        before = ids.clone()
        tok, lp, nk, km = ops.warp_sample(x.to(cuda), u, ids=ids, cur_len=cur, eos_token_id=eos, pad_token_id=pad, unfinished=unfinished,
                                          not_done=not_done, append=True, **kw)
        free = ops.warp_sample(x.to(cuda), u, **kw)           # (no processor is on: the same draw without the ids)
        assert tok.tolist()[0] == eos and tok.tolist()[3] == eos
        assert tok[[1, 4]].tolist() == [pad, pad] and lp[[1, 4]].tolist() == [0.0, 0.0] and nk[[1, 4]].tolist() == [0, 0]
        assert torch.equal(tok[[0, 2, 3, 5]], free[0][[0, 2, 3, 5]]) and torch.equal(lp[[0, 2, 3, 5]], free[1][[0, 2, 3, 5]])
        assert tok[2] != eos and tok[5] != eos
        assert unfinished.tolist() == [0, 0, 1, 0, 0, 1]
        assert int(not_done) == 2, "decremented by exactly the rows that drew eos"
        assert torch.equal(ids[:, cur], tok)
        ids[:, cur] = -7
        assert torch.equal(ids, before), "append writes column cur_len and nothing else"
        # without append the ids stay; without the flags eos is a token like any other
        tok2 = ops.warp_sample(x.to(cuda), u, ids=ids, cur_len=cur, eos_token_id=eos, pad_token_id=pad, **kw)[0]
        assert torch.equal(ids, before) and torch.equal(tok2, free[0])
        # a bool tensor serves as the flags; no counter
        flags = torch.ones(rows, dtype=torch.bool, device=cuda)
        ops.warp_sample(x.to(cuda), u, eos_token_id=eos, unfinished=flags, **kw)
        assert flags.tolist() == [False, True, True, False, True, True]


def test_limits_are_refused_before_any_launch(cuda):
    x, u = torch.randn(2, 100, device=cuda), torch.full((2,), 0.5, device=cuda)
    ids = torch.zeros(2, 8, dtype=torch.long, device=cuda)
    out = tuple(torch.full((2,), -3, dtype=dt, device=cuda) for dt in (torch.int64, torch.float32, torch.int32, torch.float32))
    for bad in (dict(top_k=-1), dict(top_k=65), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(temperature=0.0),
                dict(temperature=-1.0), dict(cols=0), dict(ids=ids, cur_len=8, append=True), dict(ids=ids, repetition_penalty=0.0),
                dict(ids=ids, no_repeat_ngram_size=-1)):
        with pytest.raises(MicoHipError, match="mico_warp_sample"):
            ops.warp_sample(x, u, out=out, **bad)
    with pytest.raises(MicoHipError, match="65536"):
        ops.warp_sample(torch.zeros(1, 65537, device=cuda), u[:1], ids=ids[:1])
    with pytest.raises(MicoHipError, match="cur_len"):
        ops.warp_sample(x, u, ids=torch.zeros(2, 513, dtype=torch.long, device=cuda))
    torch.cuda.synchronize()
    assert all(bool((t == -3).all()) for t in out), "nothing was launched"
    for bad in (dict(u=u[:1]), dict(unfinished=torch.ones(3, dtype=torch.uint8, device=cuda)), dict(not_done=torch.zeros(1, device=cuda))):
        with pytest.raises(MicoHipError):
            ops.warp_sample(x, bad.pop("u", u), **bad)
    with pytest.raises(MicoHipError):
        ops.warp_sample(x.half(), u)
    tok = ops.warp_sample(torch.zeros(1, 70000, device=cuda), u[:1], top_k=3)[0]      # without ids the vocabulary is not limited
    assert tok.tolist() in ([0], [1], [2])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
_MODEL = {}


def _model(cuda, sep_bias):
    """the captioner of tests/test_generate_gpu.py with the [SEP] output bias raised by sep_bias; 3 condition sets"""
    if not _MODEL:
        m, sd = build_model("evaclip02_base", 1, device=cuda)
        sdo = dict(sd)
        sdo["multimodal_encoder.cls.predictions.decoder.weight"] = sdo["multimodal_encoder.bert.embeddings.word_embeddings.weight"]
        _MODEL.update(m=m, sdo=sdo, bias=sdo["multimodal_encoder.cls.predictions.bias"].clone())
    bias = _MODEL["bias"].clone()
    bias[102] += sep_bias
    sdo = dict(_MODEL["sdo"])
    sdo["multimodal_encoder.cls.predictions.bias"] = bias
    with torch.no_grad():
        _MODEL["m"].multimodal_encoder.cls.predictions.bias.copy_(bias.to(cuda))
    cond = torch.randn(3, 7, 768, generator=torch.Generator().manual_seed(3))
    return _MODEL["m"].multimodal_encoder, sdo, cond


def _draw_margin(me, cuda, cond6, noise, max_new, k):
    """the host's top-k sampling loop over the product's own (recomputing) step, which also measures how decided the draws were: the smallest
    distance, over all steps and rows still alive, of the draw target to an edge of the float64 CDF, relative to the total"""
    B = cond6.shape[0]
    ids, mask = torch.full((B, 1), 101), torch.ones(B, 1, 1, dtype=torch.long)
    alive, margin = torch.ones(B, dtype=torch.bool), float("inf")
    for step in range(max_new):
        logits = me.next_token_logits(ids.to(cuda), mask.to(cuda), cond6, None).float().cpu()
        top_s, top_i = torch.topk(logits, k, dim=-1)
        cdf = torch.softmax(top_s, -1).double().cumsum(-1)
        tgt = noise[:, step].double() * cdf[:, -1]
        margin = min(margin, float(((cdf - tgt[:, None]).abs().min(-1).values / cdf[:, -1])[alive].min()))
        tok = top_i[torch.arange(B), (cdf < tgt[:, None]).sum(-1).clamp_max(k - 1)]
        tok = torch.where(alive, tok, torch.zeros_like(tok))
        alive = alive & (tok != 102)
        ids, mask = torch.cat([ids, tok[:, None]], 1), O.grow_mask(mask)
        if not bool(alive.any()):
            break
    return ids, margin


@pytest.mark.parametrize("sep_bias,max_new", [(2.5, 6), (4.0, 8)])
def test_sample_top_k_matches_generate_and_oracle(cuda, sep_bias, max_new):
    """seed 4, 3 sets x 2 sequences (another seed may be chosen where the margin assertion fails; the equality is never loosened)"""
    torch.set_num_threads(16)
    me, sdo, cond = _model(cuda, sep_bias)
    tk = me.tokenizer
    noise = torch.rand(6, max_new, generator=torch.Generator().manual_seed(4))
    init = torch.full((3, 1), tk.bos_token_id, dtype=torch.long, device=cuda)
    kw = dict(input_ids=init, attention_mask=init.new_ones(3, 1, 1), encoder_hidden_states=cond.to(cuda), max_new_tokens=max_new, top_k=10,
              eos_token_id=tk.sep_token_id, pad_token_id=tk.pad_token_id, sample_noise=noise, num_return_sequences=2)
    with runtime.precision(torch.float16), torch.no_grad():
        cond6 = cond.to(cuda).repeat_interleave(2, dim=0).contiguous()
        restated, margin = _draw_margin(me, cuda, cond6, noise, max_new, 10)
        print(f"smallest distance of a draw target to a CDF edge {margin:.3e}")
        assert margin >= 1e-4
        step = lambda ids, mask: me.next_token_logits(ids.to(cuda), mask.to(cuda), cond6, None).float().cpu()
        ref = O.generate_sample(sdo, cond6.float().cpu(), max_new, 10, noise, step_logits=step)
        assert restated.tolist() == ref.tolist()
        for use_cache in (False, True):
            host = me.generate(do_sample=True, use_cache=use_cache, **kw)
            assert host.cpu().tolist() == ref.tolist(), use_cache
            for dev in (True, False):
                out, lp = me.sample(use_cache=use_cache, device_search=dev, return_logprobs=True, **kw)
                assert out.cpu().tolist() == ref.tolist(), (use_cache, dev)
                assert lp.shape == (6, out.shape[1] - 1) and bool((lp <= 0).all())
                pads = out[:, 1:] == tk.pad_token_id
                assert bool((lp[pads] == 0).all())
    print(sep_bias, ref.tolist())
    assert (ref == 102).any(), "the case was meant to finish rows early"


def test_sample_nucleus_with_processors_device_equals_host(cuda, monkeypatch):
    torch.set_num_threads(16)
    me, _, cond = _model(cuda, 7.0)      # ([SEP] against the whole vocabulary, not the best ten: about a third of the mass per step)
    tk = me.tokenizer
    T = 8
    noise = torch.rand(6, T, generator=torch.Generator().manual_seed(6)).to(cuda)
    init = torch.full((3, 1), tk.bos_token_id, dtype=torch.long, device=cuda)
    kw = dict(input_ids=init, attention_mask=init.new_ones(3, 1, 1), encoder_hidden_states=cond.to(cuda), max_new_tokens=T, top_k=0, top_p=0.9,
              temperature=0.7, repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=3, eos_token_id=tk.sep_token_id,
              pad_token_id=tk.pad_token_id, sample_noise=noise, num_return_sequences=2, use_cache=True)
    with runtime.precision(torch.float16), torch.no_grad():
        host = me.sample(device_search=False, **kw)
        dev1, lp = me.sample(device_search=True, return_logprobs=True, **kw)
        print("host  ", host.tolist(), "\ndevice", dev1.tolist())
        assert torch.equal(dev1, host)
        for row in host.cpu().tolist():
            new = row[1:row.index(tk.sep_token_id)] if tk.sep_token_id in row else row[1:]
            assert len(new) >= 3 and len(set(zip(new, new[1:]))) == len(new) - 1, row
        free = me.sample(device_search=True, **dict(kw, min_new_tokens=0))
        assert any(tk.sep_token_id in r[1:4] for r in free.cpu().tolist()), "without the minimum a row was meant to end before 3 new tokens"
        # done_check_every does not change the ids; the host reads of a device decode of T steps: ceil(T / every) checks + the final one
        dev4 = me.sample(device_search=True, done_check_every=4, **kw)
        assert torch.equal(dev4, dev1)
        torch.cuda.synchronize()
        for every in (1, 4):
            out, sites = _count_syncs(me, monkeypatch, lambda: me.sample(device_search=True, done_check_every=every, **kw))
            print(f"done_check_every {every}: {len(sites)} synchronising calls after the prefill {sorted(set(sites))}")
            assert torch.equal(out, dev1)
            assert len(sites) <= math.ceil(T / every) + 1, sites


def test_forward_cap_captioner_mode_device_sampling(cuda, monkeypatch):
    """MiCo.forward(batch, "cap%tv", compute_loss=False) with captioner_mode: config decode_device_sampling returns the captions of the same
    call with the key off (injected noise), with and without the cached decode"""
    from mico_amd.weights import synth_inputs
    torch.set_num_threads(16)
    m, _ = build_model("evaclip02_base", 1, device=cuda, max_caption_len=5, captioner_mode=True, generate_nums=2)
    inp = synth_inputs(dict(b=2, vision=2, S=8), seed=8)
    noise = torch.rand(4, 5, generator=torch.Generator().manual_seed(1))
    batch = {k: v.to(cuda) for k, v in inp.items()}
    batch["_injected"] = {"sample_noise": noise}
    calls = []
    real = ops.warp_sample
    monkeypatch.setattr(ops, "warp_sample", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with runtime.precision(torch.float16), torch.no_grad():
        for cached in (False, True):
            m.config["decode_use_cache"] = cached
            m.config["decode_device_sampling"] = False
            want = m(dict(batch), "cap%tv", compute_loss=False)
            assert not calls
            m.config["decode_device_sampling"] = True
            got = m(dict(batch), "cap%tv", compute_loss=False)
            assert calls and got == want and len(got["generated_captions_tv"]) == 4
            del calls[:]


def test_demo_sampled_captions(cuda, tmp_path):
    """inference_demo.run_demo(sample_captions=N): N sampled captions next to the beam caption, which stays what it was"""
    import numpy as np
    import inference_demo as demo
    from PIL import Image
    from mico_amd.model.imageprocessor import ImageProcessor
    from mico_amd.model.mico import MiCo
    path = str(tmp_path / "test.jpeg")
    Image.fromarray((np.random.RandomState(0).rand(428, 640, 3) * 255).astype(np.uint8)).save(path, quality=95)
    pdir = str(tmp_path / "MiCo-synth")
    demo.write_synthetic_pretrain_dir(pdir, "evaclip02_base", steps=(3, 12), vision_layers=2, max_vision_sample_num=8)
    ckpt, opts = demo.load_from_pretrained_dir(pdir)
    old = runtime.compute_dtype()
    runtime.set_compute_dtype(torch.float16)
    try:
        model = MiCo.from_pretrained(opts, ckpt).to(cuda).eval()
        x = ImageProcessor(224, "swin", training=True)(path)
        texts = ["a man is skiing in a snowy day.", "it's a hot day"]
        base = demo.run_demo(model, x, texts, cuda)
        assert "sampled_captions" not in base
        torch.manual_seed(0)
        out = demo.run_demo(model, x, texts, cuda, use_cache=True, sample_captions=3, top_k=5, top_p=0.9, temperature=0.8, no_repeat_ngram_size=2)
        caps = out["sampled_captions"]
        assert len(caps) == 3 and all(isinstance(c, str) for c in caps)
        assert len(set(caps)) > 1, "three draws from random-init logits were meant to differ"
    finally:
        runtime.set_compute_dtype(old)
