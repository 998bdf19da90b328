"""Device-side beam search on the GPU: mico_beam_topk against a float64 reference (with and without the logits processors),
mico_beam_step / mico_beam_finalize against the host bookkeeping (the module's own _BeamHypotheses) bit for bit, generate(device_search=True)
against the host search and the CPU oracle, and the number of host reads of a device search."""
import os
import traceback
import warnings

import pytest
import torch

from common import build_model
from mico_amd import ops, runtime
from mico_amd.model.bert import BertForMaskedLM, _BeamHypotheses, apply_logits_processors
from oracle import mico_oracle as O

pytestmark = pytest.mark.gpu

GAP = 3e-4       # asserted on the reference: every gap among the best 2 nb + 1 candidates of a set
TOL = 3e-5       # a few fp32 roundings at |score| <= 64 (the lse, one subtraction, one addition): a tenth of GAP, so it cannot reorder anything


def _reference(logp64, beam_scores, nb, keep):
    """(scores, beams, tokens) [sets, keep] of the float64 scores [rows, V] + beam_scores: stable descending sort, ties by ascending flat index"""
    rows, V = logp64.shape
    flat = (logp64 + beam_scores.double()[:, None]).view(rows // nb, nb * V)
    s, i = torch.sort(flat, dim=1, descending=True, stable=True)
    return s[:, :keep], i[:, :keep] // V, i[:, :keep] % V


def _inputs(sets, nb, V, ld, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.full((sets * nb, ld), 50.0)         # (past V: larger than anything inside - a read past the row's end would show)
    logits[:, :V] = 3 * torch.randn(sets * nb, V, generator=g)
    return logits, -30 * torch.rand(sets * nb, generator=g)


def _check(got, ref, nb, tol=TOL):
    """ref: the best 2 nb + 1; the gap condition on the reference, then candidates equal and scores within tol"""
    K = 2 * nb
    rs, rb, rt = ref
    gaps = (rs[:, :-1] - rs[:, 1:])
    gaps = gaps[torch.isfinite(gaps)]
    assert gaps.numel() and float(gaps.min()) > GAP, f"the case's smallest gap {float(gaps.min()):.3e} does not exceed {GAP}"
    s, b, t = (x.cpu() for x in got)
    err = float((s.double() - rs[:, :K]).abs().max())
    print(f"smallest gap {float(gaps.min()):.3e}   largest score error {err:.3e}   tolerance {tol:.3e}")
    assert torch.equal(b.long(), rb[:, :K]) and torch.equal(t.long(), rt[:, :K])
    assert err <= tol


@pytest.mark.parametrize("sets,nb,V,ld", [(1, 1, 70, 70), (2, 3, 257, 264), (3, 3, 30522, 30528), (2, 8, 1000, 1000), (4, 2, 30522, 30522)])
def test_beam_topk_against_float64(cuda, sets, nb, V, ld):
    for s in range(3):
        logits, bs = _inputs(sets, nb, V, ld, 1000 * s + V + nb)
        ref = _reference(torch.log_softmax(logits[:, :V].double(), dim=-1), bs, nb, 2 * nb + 1)
        got = ops.beam_topk(logits.to(cuda)[:, :V], bs.to(cuda), nb)
        _check(got, ref, nb)


def test_beam_topk_first_step_ties_and_done_sets(cuda):
    sets, nb, V = 3, 3, 300
    K = 2 * nb
    # the first step of a search: every candidate comes from beam 0
    logits, _ = _inputs(sets, nb, V, V, 77)
    bs = torch.tensor([0.0, -1e9, -1e9]).repeat(sets)
    ref = _reference(torch.log_softmax(logits.double(), dim=-1), bs, nb, K + 1)
    got = ops.beam_topk(logits.to(cuda), bs.to(cuda), nb)
    assert int(got[1].abs().max()) == 0
    _check(got, (ref[0][:, :K + 1], ref[1], ref[2]), nb)
    # exact ties: equal logits inside a row, and two identical rows of a set with equal beam scores - ascending beam * V + token
    g = torch.Generator().manual_seed(5)
    base = torch.randn(V, generator=g)
    base[[200, 17]] = 10.0
    base[[250, 3]] = 9.0
    tied = torch.stack([base, base, base]).contiguous()
    got = ops.beam_topk(tied.to(cuda), torch.tensor([-1.0, -1.0, -40.0], device=cuda), nb)
    assert got[1].cpu().tolist() == [[0, 0, 1, 1, 0, 0]] and got[2].cpu().tolist() == [[17, 200, 17, 200, 3, 250]]
    s = got[0].cpu()[0]
    assert s[0] == s[1] == s[2] == s[3] and s[4] == s[5] and s[3] > s[4]
    ref = _reference(torch.log_softmax(tied.double(), dim=-1), torch.tensor([-1.0, -1.0, -40.0]), nb, K)
    assert ref[1].tolist() == got[1].cpu().tolist() and ref[2].tolist() == got[2].cpu().tolist()
    # a done set is skipped: its outputs stay as they were
    logits, bs = _inputs(sets, nb, V, V, 78)
    full = ops.beam_topk(logits.to(cuda), bs.to(cuda), nb)
    out = (torch.full((sets, K), -7.0, device=cuda), torch.full((sets, K), -7, dtype=torch.int32, device=cuda),
           torch.full((sets, K), -7, dtype=torch.int32, device=cuda))
    done = torch.tensor([0, 1, 0], dtype=torch.uint8, device=cuda)
    part = ops.beam_topk(logits.to(cuda), bs.to(cuda), nb, done=done, out=out)
    for f, p in zip(full, part):
        assert torch.equal(f[[0, 2]], p[[0, 2]]) and bool((p[1] == -7).all())


def _processor_ids(logits, V):
    """12 ids per row drawn from the row's own best tokens t0 .. t5, so that the processors hit candidates: repeated bigrams and trigrams,
    a pad in the middle and one id >= V (ignored); the last ids are (t0, t1), which t2 and t3 have followed before"""
    t = logits[:, :V].topk(8, dim=1).indices
    pick = [0, 1, 2, 0, 1, 3, -1, -2, 4, 5, 0, 1]
    cols = []
    for p in pick:
        cols.append(t[:, p] if p >= 0 else torch.full_like(t[:, 0], 0 if p == -1 else V + 5))
    return torch.stack(cols, dim=1).contiguous()


@pytest.mark.parametrize("sets,nb,V", [(2, 3, 30522), (1, 2, 300)])
def test_beam_topk_with_processors(cuda, sets, nb, V):
    K = 2 * nb
    logits, bs = _inputs(sets, nb, V, V + 6, 4242 + V)
    eos = 102
    ids = _processor_ids(logits, V)
    logits[:, eos] = 14.0                                   # eos is every row's best token (and not among the ids): the ban changes the candidates
    logp = torch.log_softmax(logits[:, :V].double(), dim=-1)
    lg, bsg, idg = logits.to(cuda)[:, :V], bs.to(cuda), ids.to(cuda)
    plain = _reference(logp, bs, nb, K)
    for name, kw in (("penalty", dict(repetition_penalty=1.3)), ("penalty < 1", dict(repetition_penalty=0.8)),
                     ("bigrams", dict(no_repeat_ngram_size=2)), ("unigrams", dict(no_repeat_ngram_size=1)), ("eos", dict(ban_eos=True)),
                     ("all", dict(repetition_penalty=1.3, no_repeat_ngram_size=3, ban_eos=True))):
        ref64 = apply_logits_processors(logp, ids, eos, **kw)
        ref = _reference(ref64, bs, nb, K + 1)
        if name != "penalty < 1":      # (a penalty below 1 lifts the seen tokens, which lead already)
            assert not torch.equal(ref[2][:, :K], plain[2]), f"{name}: the processor was meant to change the candidates"
        got = ops.beam_topk(lg, bsg, nb, ids=idg, eos_token_id=eos, **kw)
        print(name, end=": ")
        _check(got, ref, nb, tol=TOL * kw.get("repetition_penalty", 1.0))
        banned = torch.isinf(ref64)                         # no banned token among the candidates
        rows = (torch.arange(sets)[:, None] * nb + got[1].cpu().long())
        assert not bool(banned[rows, got[2].cpu().long()].any())
    # ids as a view with a row stride (the search's double buffer), cur_len shorter than the view
    wide = torch.zeros(sets * nb, 40, dtype=torch.long, device=cuda)
    wide[:, :12] = idg
    a = ops.beam_topk(lg, bsg, nb, ids=wide[:, :12], repetition_penalty=1.3, no_repeat_ngram_size=2)
    b = ops.beam_topk(lg, bsg, nb, ids=idg, repetition_penalty=1.3, no_repeat_ngram_size=2)
    c = ops.beam_topk(lg, bsg, nb, ids=wide, cur_len=12, repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))


# ---- bookkeeping ---------------------------------------------------------------------------------------------------------------------
EOS, PADT = 102, 0


def _scripted_candidates(sets, nb, steps, seed):
    """per step (scores fp32 [sets, 2 nb] descending, beams, tokens).  Set 0: eos at ranks 0 .. nb - 1 of step 1, then scores that fall fast - it
    closes at step 2; set 1 never sees eos (finalised from its open beams); set 2: scores that RISE from step to step with eos at rank 0 every
    time, so later hypotheses evict earlier ones; set 3: eos at rank nb (skipped) at steps 2 and 5, at rank 0 at step 3; the others: eos at up
    to nb random ranks"""
    g = torch.Generator().manual_seed(seed)
    K = 2 * nb
    ramp = 0.1 * torch.arange(K, dtype=torch.float32)
    out = []
    for t in range(1, steps + 1):
        score = (-0.5 * t - ramp - 0.05 * torch.rand(sets, 1, generator=g)).contiguous()
        beam = torch.randint(0, nb, (sets, K), generator=g, dtype=torch.int32)
        tok = torch.randint(200, 900, (sets, K), generator=g, dtype=torch.int32)
        score[0] = -0.2 - 3.0 * (t - 1) - ramp
        if t == 1:
            tok[0, :nb] = EOS
        score[2] = -5.0 + 0.4 * t - ramp
        tok[2, 0] = EOS
        if t in (2, 5):
            tok[3, nb] = EOS
        if t == 3:
            tok[3, 0] = EOS
        for b in range(4, sets):
            tok[b, torch.randperm(K, generator=g)[:int(torch.randint(0, nb + 1, (1,), generator=g))]] = EOS
        out.append((score, beam, tok))
    return out


def _host_step(hyps, done, cand, ids, nb, stats):
    """the body of generate()'s host loop over one step's candidates (done sets: pad, score 0, their own rows as parents)"""
    score, beam, tok = cand
    sets, L = len(hyps), ids.shape[1]
    nxt_s, nxt_t = torch.zeros(sets, nb), torch.full((sets, nb), PADT, dtype=torch.long)
    nxt_b = torch.arange(sets * nb).view(sets, nb).clone()
    for b in range(sets):
        if done[b]:
            continue
        k = 0
        for rank in range(2 * nb):
            row = b * nb + int(beam[b, rank])
            if int(tok[b, rank]) == EOS:
                stats["eos_low" if rank < nb else "eos_high"] += 1
                if rank >= nb:
                    continue
                full = len(hyps[b].beams) == nb
                before = [id(h[1]) for h in hyps[b].beams]
                hyps[b].add(ids[row].clone(), float(score[b, rank]))
                stats["evictions"] += full and [id(h[1]) for h in hyps[b].beams] != before
            else:
                nxt_s[b, k], nxt_t[b, k], nxt_b[b, k] = score[b, rank], tok[b, rank], row
                k += 1
            if k == nb:
                break
        assert k == nb
        done[b] = done[b] or hyps[b].is_done(float(score[b].max()), L + 1)
    parent = nxt_b.view(-1)
    return nxt_s.view(-1), parent, torch.cat([ids[parent], nxt_t.view(-1, 1)], dim=1)


def _host_finalize(hyps, done, ids, beam_scores, nb, max_length):
    best = []
    for b in range(len(hyps)):
        if not done[b]:
            for k in range(nb):
                hyps[b].add(ids[b * nb + k], float(beam_scores[b * nb + k]))
        best.append(max(hyps[b].beams, key=lambda h: h[0])[1])
    lens = [int(h.shape[0]) for h in best]
    width = min(max(lens) + 1, max_length)
    out = torch.full((len(hyps), width), PADT, dtype=torch.long)
    for b, h in enumerate(best):
        out[b, :lens[b]] = h
        if lens[b] < width:
            out[b, lens[b]] = EOS
    return out, lens


@pytest.mark.parametrize("nb,length_penalty", [(3, 0.6), (3, 1.0), (1, 0.6), (1, 1.0)])
def test_beam_step_and_finalize_match_host_bookkeeping(cuda, nb, length_penalty):
    sets, steps, P = 5, 9, 2
    rows, max_length = sets * nb, P + steps
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(1000, 2000, (rows, P), generator=g)
    hyps, done = [_BeamHypotheses(nb, length_penalty) for _ in range(sets)], [False] * sets
    stats = dict(eos_low=0, eos_high=0, evictions=0)
    state = ops.BeamState(sets, nb, max_length, length_penalty, cuda)
    buf = [torch.full((rows, max_length), -1, dtype=torch.long, device=cuda) for _ in range(2)]
    buf[0][:, :P] = ids.to(cuda)
    bs_dev = torch.full((rows,), -3.0, device=cuda)
    parent_dev = torch.full((rows,), -1, dtype=torch.long, device=cuda)
    bs, side, first_done = None, 0, {}
    for t, cand in enumerate(_scripted_candidates(sets, nb, steps, 31 + nb)):
        L = ids.shape[1]
        was_done = list(done)
        cand_dev = [c.to(cuda) for c in cand]
        for b in range(sets):      # a done set's candidates are not read: poison them
            if was_done[b]:
                cand_dev[0][b], cand_dev[1][b], cand_dev[2][b] = float("nan"), 1 << 20, -5
        bs, parent, ids = _host_step(hyps, done, cand, ids, nb, stats)
        ops.beam_step(state, tuple(cand_dev), buf[side], buf[side ^ 1], L, bs_dev, parent_dev, eos_token_id=EOS, pad_token_id=PADT)
        side ^= 1
        assert torch.equal(bs_dev.cpu(), bs), f"step {t}: beam scores"
        assert torch.equal(parent_dev.cpu(), parent), f"step {t}: parents"
        assert torch.equal(buf[side][:, :L + 1].cpu(), ids), f"step {t}: ids"
        assert state.done.cpu().tolist() == [int(d) for d in done], f"step {t}: done"
        assert int(state.not_done.cpu()) == done.count(False)
        for b in range(sets):
            if was_done[b]:
                assert parent[b * nb:(b + 1) * nb].tolist() == list(range(b * nb, (b + 1) * nb))
            if done[b]:
                first_done.setdefault(b, t)
        assert state.hyp_count.cpu().tolist() == [len(h.beams) for h in hyps]
        for b in range(sets):      # the n-best lists themselves, in insertion order, scores as fp64 bits
            assert state.hyp_score.cpu()[b, :len(hyps[b].beams)].tolist() == [h[0] for h in hyps[b].beams]
            assert state.worst.cpu()[b].item() == hyps[b].worst_score
    assert not done[1], "set 1 was meant to stay open (finalised from its open beams)"
    assert first_done.get(0) == 1, "set 0 was meant to close at the second step"
    assert stats["eos_low"] and (stats["eos_high"] or nb == 1), stats      # (one beam: the walk ends at the first token that is not eos)
    assert stats["evictions"] >= 1, "set 2 was meant to evict its worst hypothesis"
    ref, ref_lens = _host_finalize(hyps, done, ids, bs, nb, max_length)
    best, lens = ops.beam_finalize(state, buf[side], max_length, bs_dev, eos_token_id=EOS, pad_token_id=PADT)
    assert lens.cpu().tolist() == ref_lens
    assert torch.equal(best[:, :ref.shape[1]].cpu(), ref)
    assert bool((best[:, ref.shape[1]:] == PADT).all())
    assert int(state.not_done.cpu()) == 0 and bool(state.done.all())


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
_MODEL = {}


def _model(cuda, sep_bias):
    """the captioner of tests/test_generate_gpu.py::test_generate_matches_oracle with the [SEP] output bias raised by sep_bias"""
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


@pytest.mark.parametrize("num_beams,sep_bias,max_new", [(1, 0.0, 6), (3, 0.0, 6), (3, 1.2, 8), (3, 1.5, 8), (3, 1.7, 8), (2, 1.6, 8), (2, 1.8, 8)])
def test_device_search_matches_host_search_and_oracle(cuda, num_beams, sep_bias, max_new):
    torch.set_num_threads(16)
    me, sdo, cond = _model(cuda, sep_bias)
    with torch.no_grad():
        ref = O.generate_beam(sdo, cond, max_new, num_beams, 0.6)
    tk = me.tokenizer
    init = torch.full((3, 1), tk.bos_token_id, dtype=torch.long, device=cuda)
    kw = dict(attention_mask=init.new_ones(3, 1, 1), encoder_hidden_states=cond.to(cuda), max_new_tokens=max_new, num_beams=num_beams,
              eos_token_id=tk.sep_token_id, pad_token_id=tk.pad_token_id, length_penalty=0.6)
    with runtime.precision(torch.float16):
        host = me.generate(input_ids=init, **kw)
        assert host.cpu().tolist() == ref.tolist()
        for use_cache in (False, True):
            for every in (1, 4):
                out = me.generate(input_ids=init, use_cache=use_cache, device_search=True, done_check_every=every, **kw)
                assert out.cpu().tolist() == ref.tolist(), (use_cache, every)
        # ragged condition sets under the cache: two prompt rows read set 0, none reads set 1, one reads set 2
        rag = dict(kw, use_cache=True, rows_per_condition=[2, 0, 1])
        host_rag = me.generate(input_ids=init, **rag)
        for every in (1, 4):
            assert torch.equal(me.generate(input_ids=init, device_search=True, done_check_every=every, **rag), host_rag)


def _host_search_with_margins(me, init, mask, cond, nb, max_new, eos, pad, length_penalty, pen, ngram, min_new):
    """generate()'s host beam search with the processors, restated over the model's own cached step, which also measures how decided the search
    was (along the lines of tests/qa_oracle.beam_search_with_margins, but over EVERY decision, since the device search must reproduce the whole
    search state): the smallest, over all steps and prompt rows still open, of
      - every gap among the 2 nb + 1 best candidates (their order, and what the selection leaves out);
      - in _BeamHypotheses.add with a full list, |score - worst|; in is_done with a full list, |worst - bound|;
      - at the end, the best hypothesis' score minus the runner-up's.
    A device score differs from the host's by a few fp32 roundings (3e-5, test_beam_topk_against_float64), a hypothesis score by less."""
    B, P = init.shape
    max_length = P + max_new
    ids = init.repeat_interleave(nb, dim=0)
    dec = me._model_step(ids, mask.repeat_interleave(nb, dim=0), cond, nb, max_length, True)
    running = torch.zeros(B, nb)
    running[:, 1:] = -1e9
    running = running.view(-1)
    hyps, done, margin, parent = [_BeamHypotheses(nb, length_penalty) for _ in range(B)], [False] * B, float("inf"), None
    while True:
        logp = torch.log_softmax(dec.next_token_logits(ids, parent).float(), dim=-1)
        L = ids.shape[1]
        logp = apply_logits_processors(logp, ids, eos, pen, ngram, L - P < min_new).cpu() + running[:, None]
        V = logp.shape[-1]
        top_s, top_i = torch.topk(logp.view(B, nb * V), 2 * nb + 1, dim=1)
        ids_cpu = ids.cpu()
        nxt_s, nxt_t, nxt_b = torch.zeros(B, nb), torch.zeros(B, nb, dtype=torch.long), torch.arange(B * nb).view(B, nb).clone()
        for b in range(B):
            if done[b]:
                nxt_t[b] = pad
                continue
            gaps = top_s[b, :-1] - top_s[b, 1:]
            margin = min(margin, float(gaps[torch.isfinite(gaps)].min()))
            k = 0
            for rank in range(2 * nb):
                row, t = b * nb + int(top_i[b, rank]) // V, int(top_i[b, rank]) % V
                if t == eos:
                    if rank >= nb:
                        continue
                    if len(hyps[b].beams) == nb:
                        margin = min(margin, abs(float(top_s[b, rank]) / L ** length_penalty - hyps[b].worst_score))
                    hyps[b].add(ids_cpu[row].clone(), float(top_s[b, rank]))
                else:
                    nxt_s[b, k], nxt_t[b, k], nxt_b[b, k] = top_s[b, rank], t, row
                    k += 1
                if k == nb:
                    break
            if len(hyps[b].beams) == nb:
                margin = min(margin, abs(hyps[b].worst_score - float(top_s[b, 0]) / (L + 1) ** length_penalty))
            done[b] = hyps[b].is_done(float(top_s[b, 0]), L + 1)
        running, parent = nxt_s.view(-1), nxt_b.view(-1)
        ids = torch.cat([ids[parent.to(ids.device)], nxt_t.view(-1, 1).to(ids.device)], dim=1)
        if all(done) or ids.shape[1] >= max_length:
            break
    ids_cpu, best = ids.cpu(), []
    for b in range(B):
        if not done[b]:
            for k in range(nb):
                hyps[b].add(ids_cpu[b * nb + k], float(running[b * nb + k]))
        ranked = sorted(hyps[b].beams, key=lambda h: h[0])
        if len(ranked) > 1:
            margin = min(margin, ranked[-1][0] - ranked[-2][0])
        best.append(ranked[-1][1].tolist())
    return best, margin


def test_device_search_with_processors_matches_host_search(cuda):
    """seed 3, the [SEP] bias raised by 1.5, three beams: the smallest decision margin of the host search is asserted before the two are compared
    (another seed may be chosen where that fails; the equality is never loosened)"""
    me, _, cond = _model(cuda, 1.5)
    tk = me.tokenizer
    init = torch.full((3, 1), tk.bos_token_id, dtype=torch.long, device=cuda)
    mask = init.new_ones(3, 1, 1)
    proc = dict(no_repeat_ngram_size=2, repetition_penalty=1.3, min_new_tokens=3)
    kw = dict(attention_mask=mask, encoder_hidden_states=cond.to(cuda), max_new_tokens=8, num_beams=3, eos_token_id=tk.sep_token_id,
              pad_token_id=tk.pad_token_id, length_penalty=0.6, use_cache=True, **proc)
    with runtime.precision(torch.float16), torch.no_grad():
        best, margin = _host_search_with_margins(me, init, mask, cond.to(cuda), 3, 8, tk.sep_token_id, tk.pad_token_id, 0.6, 1.3, 2, 3)
        host = me.generate(input_ids=init, **kw)
        plain = me.generate(input_ids=init, **{k: v for k, v in kw.items() if k not in proc})
        print(f"smallest decision margin of the host search {margin:.3e}\nhost {host.tolist()}\nplain {plain.tolist()}")
        for row, h in zip(host.cpu().tolist(), best):
            assert row[:len(h)] == h, "the restated search and generate() disagree"
        assert margin > 1e-4
        assert not torch.equal(host, plain), "the processors were meant to change the captions"
        for row in host.cpu().tolist():
            new = row[1:row.index(tk.sep_token_id)] if tk.sep_token_id in row else row[1:]
            assert len(new) >= 3 and len(set(zip(new, new[1:]))) == len(new) - 1
        for every in (1, 4):
            assert torch.equal(me.generate(input_ids=init, device_search=True, done_check_every=every, **kw), host)


def _count_syncs(me, monkeypatch, run):
    """synchronising torch calls made from frames inside mico_amd/ during run(), counted after the decode's first model step (the prefill)
    has returned - torch.cuda.set_sync_debug_mode("warn") and a warnings hook, the method of tools/probes/sync_probe.py"""
    state = dict(on=False, sites=[])
    real = BertForMaskedLM._model_step

    class AfterPrefill:
        def __init__(self, dec):
            self.dec = dec

        def next_token_logits(self, ids, parent=None):
            out = self.dec.next_token_logits(ids, parent)
            state["on"] = True
            return out

    monkeypatch.setattr(BertForMaskedLM, "_model_step", lambda self, *a, **k: AfterPrefill(real(self, *a, **k)))

    def hook(message, category, filename, lineno, file=None, line=None):
        if not state["on"] or "synchroniz" not in str(message):
            return
        st = [f for f in traceback.extract_stack()[:-1] if os.sep + "mico_amd" + os.sep in f.filename]
        if st:
            state["sites"].append(f"{os.path.basename(st[-1].filename)}:{st[-1].lineno} {st[-1].name}")

    old = warnings.showwarning
    with warnings.catch_warnings():
        warnings.simplefilter("always")
        warnings.showwarning = hook
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = run()
        finally:
            torch.cuda.set_sync_debug_mode("default")
            warnings.showwarning = old
    monkeypatch.undo()
    return out, state["sites"]


def test_device_search_host_reads(cuda, monkeypatch):
    """a device search of 8 steps with done_check_every=4: after the prefill at most 2 reads of the not-done counter and the one read of the
    lengths at finalisation; the host search's count is printed next to it"""
    me, _, cond = _model(cuda, 0.0)
    tk = me.tokenizer
    init = torch.full((3, 1), tk.bos_token_id, dtype=torch.long, device=cuda)
    kw = dict(input_ids=init, attention_mask=init.new_ones(3, 1, 1), encoder_hidden_states=cond.to(cuda), max_new_tokens=8, num_beams=3,
              eos_token_id=tk.sep_token_id, pad_token_id=tk.pad_token_id, length_penalty=0.6, use_cache=True)
    with runtime.precision(torch.float16):
        me.generate(device_search=True, done_check_every=4, **kw)      # (warm-up: allocations, weight casts)
        torch.cuda.synchronize()
        dev_out, dev_sites = _count_syncs(me, monkeypatch, lambda: me.generate(device_search=True, done_check_every=4, **kw))
        host_out, host_sites = _count_syncs(me, monkeypatch, lambda: me.generate(**kw))
    print(f"device search: {len(dev_sites)} synchronising calls after the prefill {sorted(set(dev_sites))}")
    print(f"host search:   {len(host_sites)} synchronising calls after the prefill {sorted(set(host_sites))}")
    assert torch.equal(dev_out, host_out)
    assert len(dev_sites) <= 3, dev_sites
