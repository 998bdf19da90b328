"""SCST caption fine-tuning on the GPU: the full-vocabulary draw (mico_vocab_sample) against a float64 inverse-CDF, the per-row log-prob head
(mico_logprob_fwd_bwd) against fp32 torch and against the unchanged loss entry point, the two-stream scoring pass against the step-by-step
product path and against the reference's own step-by-step run (tests/golden/scst_b16_d2.pt), generate_scst and MiCo.forward_scst."""
import pytest
import torch

from common import golden, build_model, grad_digest_check, precision_config, rel_err, Errs, PRECISION_CONFIGS
from mico_amd import functional as Fn
from mico_amd import ops, runtime
from mico_amd.model.bert import first_eos_valid
from mico_amd.weights import synth_inputs

pytestmark = pytest.mark.gpu

CLS, SEP, PAD, MASK = 101, 102, 0, 103
NEG_INF = float("-inf")


# ---------------------------------------------------------------------------------------------------------------------
# 4. mico_vocab_sample
# ---------------------------------------------------------------------------------------------------------------------
VS_SEED = 41      # the float64 reference has every random draw of the four shapes at a margin above 1e-5 with this seed (asserted below)
VS_SHAPES = [(5, 30522, 30528), (3, 257, 257), (2, 255, 256), (1, 1, 8)]


def _vs_case(rows, cols, ld, seed=VS_SEED):
    """logits randn * 3 [rows, ld]; with more than 64 columns five -inf entries per row and, in row 0, an all -inf tail of 40 columns"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, ld, generator=g) * 3
    if cols > 64:
        for r in range(rows):
            x[r, torch.randint(0, cols - 40, (5,), generator=g)] = NEG_INF
        x[0, cols - 40:cols] = NEG_INF
    return x, g


def _vs_cdf(x, cols):
    xd = x[:, :cols].double()
    m = xd.max(1, keepdim=True).values
    w = torch.exp(xd - m)
    cdf = w.cumsum(1)
    return w, cdf, m[:, 0] + cdf[:, -1].log()


def _vs_ref(x, cols, u):
    """float64 inverse-CDF in column order: (index, log-prob, margin) - the first column whose CDF exceeds u * total (a zero-weight column
    leaves the CDF flat and is skipped), the last column with a weight if there is none; margin = the distance of u * total to the nearest
    CDF edge relative to the total"""
    w, cdf, lse = _vs_cdf(x, cols)
    tgt = u.double() * cdf[:, -1]
    idx = (cdf <= tgt[:, None]).sum(1)
    last = (w > 0).long().cumsum(1).argmax(1)
    idx = torch.where(idx >= cols, last, idx)
    logp = x[:, :cols].double().gather(1, idx[:, None])[:, 0] - lse
    return idx, logp, (cdf - tgt[:, None]).abs().min(1).values / cdf[:, -1]


@pytest.mark.parametrize("rows,cols,ld", VS_SHAPES)
def test_vocab_sample_against_float64_inverse_cdf(cuda, rows, cols, ld):
    x, g = _vs_case(rows, cols, ld)
    xg = x.to(cuda)
    w, cdf, lse = _vs_cdf(x, cols)
    p = w / cdf[:, -1:]
    # --- every target of probability > 1e-4 (at most 24 per row, the likeliest and a spread of the rest), u at the middle of its CDF interval:
    #     the margin is half the probability, far above fp32 summation error - ids exact on every draw
    rr, tt, uu = [], [], []
    for r in range(rows):
        cand = (p[r] > 1e-4).nonzero()[:, 0]
        order = cand[p[r, cand].argsort(descending=True)]
        pick = torch.cat([order[:12], order[12:][torch.linspace(0, max(len(order) - 13, 0), 12).long()] if len(order) > 12 else order[:0]])
        for t in pick.unique().tolist():
            lo = cdf[r, t - 1] if t > 0 else torch.zeros((), dtype=torch.float64)
            rr.append(r)
            tt.append(t)
            uu.append(float((lo + cdf[r, t]) / 2 / cdf[r, -1]))
    rr, tt, u = torch.tensor(rr), torch.tensor(tt), torch.tensor(uu, dtype=torch.float32)
    assert len(tt) >= rows
    tok, lp = ops.vocab_sample(xg[rr.to(cuda)], u.to(cuda), cols=cols)
    assert tok.dtype == torch.int64 and lp.dtype == torch.float32
    assert torch.equal(tok.cpu(), tt), (tok.cpu() - tt).abs().max()
    want_lp = x[rr, tt].double() - lse[rr]
    assert (lp.cpu().double() - want_lp).abs().max() < 1e-5
    # --- u = 0: the first column of non-zero weight; u = 1 - 2^-24 on the row with the -inf tail: a column in front of the tail
    x0 = x.clone()
    if cols > 64:
        x0[:, :3] = NEG_INF
    tok0, _ = ops.vocab_sample(x0.to(cuda), torch.zeros(rows, device=cuda), cols=cols)
    assert tok0.cpu().tolist() == [int((x0[r, :cols] > NEG_INF).nonzero()[0]) for r in range(rows)]
    hi = torch.full((rows,), 1.0 - 2.0 ** -24)
    tok1, lp1 = ops.vocab_sample(xg, hi.to(cuda), cols=cols)
    assert bool((tok1.cpu() < cols).all()) and bool(torch.isfinite(lp1).all())
    assert bool((x[torch.arange(rows), tok1.cpu()] > NEG_INF).all())          # never a zero-weight column
    if cols > 64:
        assert int(tok1[0]) < cols - 40
    # --- random u, the rule of test_itm_sample
    sure_all = []
    for trial in range(4):
        u = torch.rand(rows, generator=g)
        ref, ref_lp, margin = _vs_ref(x, cols, u)
        got, got_lp = ops.vocab_sample(xg, u.to(cuda), cols=cols)
        again, again_lp = ops.vocab_sample(xg, u.to(cuda), cols=cols)
        assert torch.equal(got, again) and torch.equal(got_lp, again_lp)      # two launches, the same bits
        got, got_lp = got.cpu(), got_lp.cpu()
        sure = margin > 1e-5
        assert torch.equal(got[sure], ref[sure]), (got, ref)
        assert bool(((got - ref).abs() <= 1).all())
        assert (got_lp.double()[sure] - ref_lp[sure]).abs().max() < 1e-5 if bool(sure.any()) else True
        sure_all.append(sure)
    assert torch.cat(sure_all).float().mean() >= 0.9


def test_vocab_sample_finished_rows(cuda):
    rows, cols, ld = 6, 257, 264
    x, g = _vs_case(rows, cols, ld, seed=7)
    w, cdf, lse = _vs_cdf(x, cols)
    eos = 9
    x[:, eos] = 2.0                                            # a finite weight for eos in every row
    w, cdf, lse = _vs_cdf(x, cols)
    u = torch.rand(rows, generator=g)
    for r in (1, 4):                                           # these rows draw eos: u in the middle of its interval
        u[r] = float((cdf[r, eos - 1] + cdf[r, eos]) / 2 / cdf[r, -1])
    ref, ref_lp, margin = _vs_ref(x, cols, u)
    assert bool((margin > 1e-5).all()) and ref[1] == eos and ref[4] == eos and ref[0] != eos and ref[3] != eos
    unfinished = torch.tensor([True, True, False, True, True, False], device=cuda)
    tok, lp = ops.vocab_sample(x.to(cuda), u.to(cuda), cols=cols, unfinished=unfinished, eos_token_id=eos, pad_token_id=5)
    assert tok.cpu().tolist() == [int(ref[0]), eos, 5, int(ref[3]), eos, 5]
    assert lp[2] == 0 and lp[5] == 0 and (lp.cpu().double()[[0, 1, 3, 4]] - ref_lp[[0, 1, 3, 4]]).abs().max() < 1e-5
    assert unfinished.cpu().tolist() == [True, False, False, True, False, False]     # finished stays finished, eos flips
    # without a flag tensor nothing is finished; without an eos id nothing flips
    tok2, _ = ops.vocab_sample(x.to(cuda), u.to(cuda), cols=cols)
    assert torch.equal(tok2.cpu(), ref)
    flags = torch.ones(rows, dtype=torch.bool, device=cuda)
    ops.vocab_sample(x.to(cuda), u.to(cuda), cols=cols, unfinished=flags)
    assert bool(flags.all())
    with pytest.raises(ops.MicoHipError):
        ops.vocab_sample(x.to(cuda).half(), u.to(cuda))
    with pytest.raises(ops.MicoHipError):
        ops.vocab_sample(x.to(cuda), u.to(cuda)[:3])


# ---------------------------------------------------------------------------------------------------------------------
# 5. per-row log-prob head
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_logprob_rows_against_torch_and_the_loss_entry_point(cuda, dtype):
    """7 rows over the LM head's vocabulary with its padded stride: log P(target) and the gradient under per-row upstream gradients against
    fp32 torch at the bounds of test_kernels_gpu.py's cross-entropy case for 16-bit logits (1e-4 / 1.6e-2 relative); mico_ce_fwd_bwd on the
    same logits gives the same bits before and after, and - its kernel being the same - the negated bits of the new entry point where
    the two are asked the same question."""
    rows, V = 7, 30522
    Vp = (V + Fn.VOCAB_PAD - 1) // Fn.VOCAB_PAD * Fn.VOCAB_PAD
    g = torch.Generator().manual_seed(23)
    logits = (torch.randn(rows, Vp, generator=g) * 2).to(cuda, dtype)
    tgt = torch.randint(0, V, (rows,), generator=g).to(cuda)
    tgt[3] = -100
    gout = torch.tensor([1.0, 0.0, -0.75, 0.5, 2.0, -1.5, 0.25], device=cuda)

    def ce():      # the unchanged entry point as LMHeadLossFn calls it
        loss, d = torch.empty(rows, device=cuda), torch.zeros_like(logits)
        ops.ce_fwd_bwd(logits, tgt, cols=V, row_loss=loss, dlogits=d, dscale_ptr=torch.tensor([0.5], device=cuda))
        return loss, d

    before = ce()
    lf = logits[:, :V].float().detach().requires_grad_(True)
    safe = tgt.clamp_min(0)
    ref = torch.log_softmax(lf, -1).gather(1, safe[:, None])[:, 0] * (tgt != -100)
    (gout * ref).sum().backward()
    logp = torch.empty(rows, device=cuda)
    ops.logprob_fwd_bwd(logits, tgt, cols=V, row_logp=logp)
    d = torch.full_like(logits, 7.0)
    ops.logprob_fwd_bwd(logits, tgt, cols=V, dlogits=d, row_gscale=gout)
    er = Errs(f"logprob head/{dtype}")
    er.add("logp", rel_err(logp, ref), 1e-4)
    er.add("dlogits", rel_err(d[:, :V], lf.grad), 1.6e-2)
    er.check()
    assert logp[3] == 0 and bool((d[3, :V] == 0).all()) and bool((d[1, :V] == 0).all())     # ignored row, zero upstream gradient
    assert bool((d[:, V:] == 7.0).all())                                                      # the padding columns are not written
    # in place over the logits, as the head's backward runs it
    inplace = logits.clone()
    ops.logprob_fwd_bwd(inplace, tgt, cols=V, dlogits=inplace, row_gscale=gout, gscale=3.0)
    d3 = torch.zeros_like(logits)
    ops.logprob_fwd_bwd(logits, tgt, cols=V, dlogits=d3, row_gscale=gout, gscale=3.0)
    assert torch.equal(inplace[:, :V], d3[:, :V])
    after = ce()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    half = torch.full((rows,), 0.5, device=cuda)
    dn = torch.zeros_like(logits)
    ops.logprob_fwd_bwd(logits, tgt, cols=V, dlogits=dn, row_gscale=half)
    assert torch.equal(logp, -before[0]) and torch.equal(dn[:, :V], -before[1][:, :V])
    with pytest.raises(ops.MicoHipError):
        ops.logprob_fwd_bwd(logits, tgt, cols=V, dlogits=d)


# ---------------------------------------------------------------------------------------------------------------------
# 6. sequence_logprobs = the step-by-step product path
# ---------------------------------------------------------------------------------------------------------------------
def _bert(cuda, sep_bias=0.0):
    m, _ = build_model("evaclip02_base", 1, device=cuda)
    if sep_bias:
        with torch.no_grad():
            m.multimodal_encoder.cls.predictions.bias[SEP] += sep_bias
    return m


@pytest.fixture(scope="module")
def bert_model(cuda):
    return _bert(cuda)


def _stepwise_logp(me, ids, mask0, enc, P):
    """log_softmax(next_token_logits(prefix))[token] for every generated position (the recomputing step), and the largest |logit| seen"""
    T = ids.shape[1] - P
    mask, out, top = mask0, [], 0.0
    for t in range(T):
        logits = me.next_token_logits(ids[:, :P + t], mask, enc, None).float()
        top = max(top, logits.abs().max().item())
        out.append(torch.log_softmax(logits, -1).gather(1, ids[:, P + t:P + t + 1])[:, 0])
        mask = me.update_attention_mask(mask)
    return torch.stack(out, 1), top


@pytest.mark.parametrize("kind", ["caption", "question"])
def test_sequence_logprobs_equals_the_stepwise_path(cuda, bert_model, kind):
    """One two-stream pass against T recomputing steps at the bound the decode cache is held to against the same step (2e-3 of the largest
    |logit|, absolute: both are re-orderings of the same arithmetic); positions after eos exactly 0.
    Measured (MI355X, fp16): 1.6e-4 (caption) and 2.3e-4 (question) against a bound of 5.2e-3."""
    me = bert_model.multimodal_encoder
    g = torch.Generator().manual_seed(31)
    if kind == "caption":       # 4 rows on 2 condition sets of 7 tokens, P = 1, T = 5, row 2 ends at step 2
        P, T = 1, 5
        cond = torch.randn(2, 7, 768, generator=g).repeat_interleave(2, dim=0).to(cuda)
        prompt = torch.full((4, 1), CLS)
        mask0 = torch.ones(4, 1, 1, dtype=torch.long)
        gen = torch.randint(1000, 30000, (4, T), generator=g)
        gen[2, 1], gen[2, 2:] = SEP, PAD
    else:                       # the padded question prompt of test_teacher_forced_logits_padded_question_prompt, T = 4
        P, T = 7, 4
        cond = torch.randn(2, 9, 768, generator=g).to(cuda)
        q = torch.randint(1000, 30000, (2, 6), generator=g)
        kp = torch.ones(2, 6, dtype=torch.long)
        kp[1, 4:] = 0
        q[1, 4:] = 0
        prompt = torch.cat([q, torch.full((2, 1), CLS)], 1)
        mask0 = me.update_attention_mask(kp[:, None, :].expand(2, 6, 6).contiguous())
        gen = torch.randint(1000, 30000, (2, T), generator=g)
    ids, mask0 = torch.cat([prompt, gen], 1).to(cuda), mask0.to(cuda)
    with runtime.precision(torch.float16), torch.no_grad():
        got = me.sequence_logprobs(ids, mask0, cond, prompt_len=P, eos_token_id=SEP, pad_token_id=PAD)
        want, top = _stepwise_logp(me, ids, mask0, cond, P)
    assert got.shape == (ids.shape[0], T) and got.dtype == torch.float32
    valid = first_eos_valid(ids[:, P:], SEP)
    diff = ((got - want).abs() * valid).max().item()
    print(f"sequence_logprobs vs step by step ({kind}): worst |d logp| {diff:.3e}, bound {2e-3 * top:.3e} (max |logit| {top:.3f})")
    assert diff <= 2e-3 * top, (diff, top)
    assert bool((got[~valid] == 0).all())
    if kind == "caption":
        assert not bool(valid[2, 2:].any()) and bool(valid[2, :2].all())


# ---------------------------------------------------------------------------------------------------------------------
# 7. against the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mico_model(cuda):
    return build_model("evaclip02_base", 2, device=cuda, max_caption_len=6)[0]


@pytest.mark.parametrize("pc", PRECISION_CONFIGS)
def test_sequence_logprobs_against_reference(cuda, mico_model, pc):
    """logp and the gradients of sum(w * logp) for tv and tva against the reference's own step-by-step run (tools/make_scst_golden.py):
    logp within 1e-3 of the largest |logp| (the QA loss gate), gradient digests within 2e-2.
    Measured (MI355X): parity 5.7e-5 / 3.0e-3, timed 1.0e-4 / 1.3e-3."""
    m = mico_model
    fx = golden("scst_b16_d2.pt")
    meta = fx["meta"]
    inp = synth_inputs(dict(b=meta["b"], vision=meta["vision"], audio=meta["audio"], S=0), seed=meta["input_seed"])
    batch = {k: v.to(cuda) for k, v in inp.items()}
    ids, w = fx["ids"].to(cuda), fx["weights"].to(cuda)
    me = m.multimodal_encoder
    er = Errs(f"scst/{pc}")
    with precision_config(pc):
        m.zero_grad(set_to_none=True)
        enc = m.encode_batch(batch)
        total = 0.0
        for st in meta["subtasks"].split("%"):
            logp = me.sequence_logprobs(ids, ids.new_ones(ids.shape[0], 1, 1), m._condition_feats(enc, st[1:]), prompt_len=1,
                                        eos_token_id=SEP, pad_token_id=PAD)
            ref = fx["logp"][st]
            er.add(f"logp {st}", (logp.detach().cpu() - ref).abs().max() / ref.abs().max(), 1e-3)
            assert bool((logp.detach().cpu()[fx["valid"] == 0] == 0).all())
            total = total + (w[:, None] * logp).sum()
        total.backward()
    named = dict(m.named_parameters())
    worst = ("", 0.0)
    for n, d in fx["grads"].items():
        ge = grad_digest_check(d, named[n].grad, None)
        if ge > worst[1]:
            worst = (n, ge)
    er.add(f"worst grad digest ({worst[0]})", worst[1], 2e-2)
    er.check()


# ---------------------------------------------------------------------------------------------------------------------
# 8. generate_scst
# ---------------------------------------------------------------------------------------------------------------------
def test_generate_scst_end_to_end(cuda):
    """3 condition sets x 2 samples, T = 6.  A [SEP] bias of 9.5 gives [SEP] (column 102, so its CDF interval starts below 0.01) a
    probability of 0.15 .. 0.55 under the nearly flat synthetic logits: u = 0.05 draws it, u >= 0.7 does not."""
    m = _bert(cuda, sep_bias=9.5)
    me = m.multimodal_encoder
    g = torch.Generator().manual_seed(8)
    sets, K, T = 3, 2, 6
    cond = torch.randn(sets, 7, 768, generator=g).to(cuda).requires_grad_(True)
    noise = 0.7 + 0.29 * torch.rand(sets * K, T, generator=g)
    noise[0, 2] = noise[3, 0] = noise[4, 5] = 0.05
    prompt = torch.full((sets, 1), CLS, dtype=torch.long, device=cuda)
    pmask = prompt.new_ones(sets, 1, 1)
    kw = dict(max_new_tokens=T, eos_token_id=SEP, pad_token_id=PAD)
    with runtime.precision(torch.float16):
        ids, logprobs, step_lp = me.generate_scst(prompt, pmask, cond, sample_noise=noise, num_return_sequences=K, use_cache=True,
                                                  return_rollout_logprobs=True, **kw)
        assert ids.shape == (sets * K, 1 + T) and logprobs.shape == (sets * K, T) and logprobs.requires_grad and not step_lp.requires_grad
        assert bool((ids[:, 0] == CLS).all())
        gen = ids[:, 1:].cpu()
        assert gen[0, 2] == SEP and gen[3, 0] == SEP and gen[4, 5] == SEP and (gen == SEP).sum() == 3
        valid = first_eos_valid(gen, SEP)
        assert bool((gen[~valid] == PAD).all()) and int((~valid).sum()) == 3 + 5
        same = me.generate(input_ids=prompt, attention_mask=pmask, encoder_hidden_states=cond.detach(), do_sample=True, top_k=0,
                           sample_noise=noise, num_return_sequences=K, use_cache=True, **kw)
        assert torch.equal(same, ids[:, :same.shape[1]]) and bool((ids[:, same.shape[1]:] == PAD).all())
        # the recomputing roll-out draws the same tokens here (every draw sits far inside its interval)
        slow = me.generate(input_ids=prompt, attention_mask=pmask, encoder_hidden_states=cond.detach(), do_sample=True, top_k=0,
                           sample_noise=noise, num_return_sequences=K, use_cache=False, **kw)
        assert torch.equal(slow[:, 1:] == SEP, same[:, 1:] == SEP)
        again = me.sequence_logprobs(ids, pmask.repeat_interleave(K, 0), cond.repeat_interleave(K, 0), prompt_len=1, eos_token_id=SEP,
                                     pad_token_id=PAD)
        assert torch.equal(again, logprobs)
        with torch.no_grad():
            top = me.next_token_logits(prompt, pmask, cond.detach(), None).abs().max().item()
        diff = (logprobs.detach() - step_lp).abs().max().item()
        print(f"generate_scst: scoring pass vs the roll-out's own log-probs: worst |d logp| {diff:.3e}, bound {2e-3 * top:.3e}")
        assert diff <= 2e-3 * top, (diff, top)
        assert bool((logprobs.detach()[~valid.to(cuda)] == 0).all()) and bool((step_lp[~valid.to(cuda)] == 0).all())
        # greedy: the argmax roll-out, one row per set
        g_ids, g_lp = me.generate_scst(prompt, pmask, cond.detach(), do_sample=False, **kw)
        assert g_ids.shape == (sets, 1 + T) and bool((g_ids[:, 1] == SEP).all()) and bool((g_ids[:, 2:] == PAD).all())
        m.zero_grad(set_to_none=True)
        logprobs.sum().backward()
    for t in (me.bert.encoder.layer[3].attention.self.query.weight.grad, me.cls.predictions.bias.grad, cond.grad):
        assert t is not None and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0


def test_generate_top_k_positive_keeps_its_path(cuda, bert_model, monkeypatch):
    """top_k >= 1 never reaches the full-vocabulary kernel"""
    me = bert_model.multimodal_encoder
    monkeypatch.setattr(ops, "vocab_sample", lambda *a, **k: pytest.fail("top_k >= 1 must not draw through mico_vocab_sample"))
    prompt = torch.full((2, 1), CLS, dtype=torch.long, device=cuda)
    cond = torch.randn(2, 7, 768, generator=torch.Generator().manual_seed(2)).to(cuda)
    with runtime.precision(torch.float16):
        out = me.generate(input_ids=prompt, attention_mask=prompt.new_ones(2, 1, 1), encoder_hidden_states=cond, do_sample=True, top_k=10,
                          sample_noise=torch.rand(2, 3), max_new_tokens=3, eos_token_id=SEP, pad_token_id=PAD, use_cache=True)
    assert out.shape[0] == 2 and 2 <= out.shape[1] <= 4


# ---------------------------------------------------------------------------------------------------------------------
# 9. forward_scst
# ---------------------------------------------------------------------------------------------------------------------
WORDS = ["a", "the", "dog", "cat", "runs", "sleeps"]
CAPTIONS = ["a dog runs", "the cat sleeps", "a cat runs"]


def _f1(caption, reference):
    c, r = caption.split(), reference.split()
    hit = sum(min(c.count(w), r.count(w)) for w in set(c))
    return 0.0 if not hit else 2 * hit / (len(c) + len(r))


def test_forward_scst(cuda, mico_model, monkeypatch):
    """b = 3, cap%tv, 2 samples each, max_caption_len 6, reward = token-overlap F1 against raw_captions.  Six words and [SEP] get an LM-head
    bias boost so that the captions are made of them and the rewards differ."""
    m = mico_model
    me = m.multimodal_encoder
    tk = me.tokenizer
    bias = me.cls.predictions.bias
    boosted = tk.convert_tokens_to_ids(WORDS) + [SEP]
    saved = bias.detach().clone()
    inp = synth_inputs(dict(b=3, vision=2, audio=0, S=0), seed=99)
    batch = {k: v.to(cuda) for k, v in inp.items()}
    batch["raw_captions"] = CAPTIONS
    noise = torch.rand(6, 6, generator=torch.Generator().manual_seed(14))
    scored = []
    orig = me.sequence_logprobs
    monkeypatch.setattr(me, "sequence_logprobs", lambda ids, *a, **k: scored.append((ids, orig(ids, *a, **k))) or scored[-1][1])

    def reward(captions, sample_index, b):
        return [_f1(c, b["raw_captions"][i]) for c, i in zip(captions, sample_index)]

    try:
        with torch.no_grad():
            bias[boosted] += 9.0
        with precision_config("timed"):
            m.zero_grad(set_to_none=True)
            out = m.forward_scst(batch, "cap%tv", reward, num_samples=2, sample_noise=noise)
            assert set(out) == {"loss_scst", "reward_sample", "reward_greedy", "sampled_captions_tv", "greedy_captions_tv"}
            assert len(out["sampled_captions_tv"]) == 6 and len(out["greedy_captions_tv"]) == 3 and len(scored) == 1
            ids, logp = scored[0]
            assert ids.shape == (6, 7) and tk.batch_decode(ids[:, 1:], skip_special_tokens=True) == out["sampled_captions_tv"]
            r_s = torch.tensor(reward(out["sampled_captions_tv"], [0, 0, 1, 1, 2, 2], batch))
            r_g = torch.tensor(reward(out["greedy_captions_tv"], [0, 1, 2], batch))
            adv = (r_s - r_g.repeat_interleave(2)).to(cuda)
            assert float(adv.abs().max()) > 0, (out["sampled_captions_tv"], out["greedy_captions_tv"])
            n_valid = first_eos_valid(ids[:, 1:], SEP).sum()
            want = -(adv[:, None] * logp.detach()).sum() / n_valid
            assert abs(out["loss_scst"].item() - want.item()) <= 1e-6 * max(abs(want.item()), 1e-6)
            assert abs(out["reward_sample"].item() - r_s.mean().item()) < 1e-6 and abs(out["reward_greedy"].item() - r_g.mean().item()) < 1e-6
            out["loss_scst"].backward()
            for p in (m.vision_encoder.visual.patch_embed.proj.weight, me.bert.encoder.layer[5].crossattention.self.key.weight):
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
            # a constant reward: zero advantage, the loss and every gradient exactly 0
            m.zero_grad(set_to_none=True)
            flat = m.forward_scst(batch, "cap%tv", lambda c, i, b: [0.5] * len(c), num_samples=2, sample_noise=noise)
            assert flat["loss_scst"].item() == 0
            flat["loss_scst"].backward()
            grads = [p.grad for p in m.parameters() if p.grad is not None]
            assert grads and all(bool((g == 0).all()) for g in grads)
    finally:
        with torch.no_grad():
            bias.copy_(saved)
        m.zero_grad(set_to_none=True)
