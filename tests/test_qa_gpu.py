"""Question answering on the GPU: the ragged decode attention (mico_attn_decode_ragged) against fp32 torch attention and, bit for bit,
against the uniform launch; the ragged cached decode step against the recomputing one under teacher forcing; MiCo.forward_qa's loss and
gradients against the reference's own (tests/golden/qa_b16_d2.pt) and against the full-row LM head; answer decoding with the cache off and
on; the demo's answers."""
import pytest
import torch

import qa_oracle
from common import golden, build_model, grad_digest_check, precision_config, Errs, PRECISION_CONFIGS
from mico_amd import functional as Fn
from mico_amd import ops, runtime
from mico_amd.weights import synth_inputs

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
SENTINEL = 7.0


def tol(dtype, k=1.0):
    """the bound of tests/test_decode_cache_gpu.py::test_attn_decode_matches_torch"""
    return (2e-3 if dtype == torch.float16 else 1.6e-2) * k


# ---------------------------------------------------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------------------------------------------------
def _case(dev, dtype, rows_per_set, Qp, Sk, H, masked, seed):
    g = torch.Generator().manual_seed(seed)
    D, rows, sets = H * 64, sum(rows_per_set), len(rows_per_set)
    q = torch.randn(rows * Qp, D, generator=g).to(dev, dtype)
    kv = torch.randn(sets, Sk, 2 * D, generator=g).to(dev, dtype)      # [K | V] per key, as the caches hold them
    mask = torch.where(torch.rand(rows, Qp, Sk, generator=g) < 0.3, -10000.0, 0.0).to(dev) if masked else None
    return q, kv, mask


def _mask_kw(mask):
    return dict(mask=mask, mask_strides=(mask.stride(0), mask.stride(1)) if mask is not None else (0, 0))


def _ragged(q, kv, mask, rows_per_set, Qp, Sk, H, splits, tail_rows=0):
    """-> o [rows Qp + tail_rows, D], pre-filled with SENTINEL (the tail rows belong to no set)"""
    D = H * 64
    o = torch.full((q.shape[0] + tail_rows, D), SENTINEL, dtype=q.dtype, device=q.device)
    table = ops.decode_set_row0(rows_per_set).to(q.device)
    ops.attn_decode_ragged(q, kv, kv[:, :, D:], o, set_row0=table, rows=sum(rows_per_set), max_rows_per_set=max(rows_per_set), q_per_row=Qp,
                           H=H, Sk=Sk, hd=64, scale=0.125, q_rs=D, kv_strides=(kv.stride(0), kv.stride(1)), o_rs=D, splits=splits,
                           **_mask_kw(mask))
    return o


def _uniform(q, kv, mask, sets, R, Qp, Sk, H, splits):
    D = H * 64
    o = torch.full_like(q, SENTINEL)
    ops.attn_decode(q, kv, kv[:, :, D:], o, sets=sets, rows_per_set=R, q_per_row=Qp, H=H, Sk=Sk, hd=64, scale=0.125, q_rs=D,
                    kv_strides=(kv.stride(0), kv.stride(1)), o_rs=D, splits=splits, **_mask_kw(mask))
    return o


def _ref_set(q, kv_s, mask, Sk, H):
    """fp32 torch attention of one set's queries q [n, D] over its keys kv_s [Sk, 2 D]; mask [n, Sk] or None"""
    D = H * 64
    qf = q.float().view(-1, H, 64).permute(1, 0, 2)
    k = kv_s[:, :D].float().view(Sk, H, 64).permute(1, 0, 2)
    v = kv_s[:, D:].float().view(Sk, H, 64).permute(1, 0, 2)
    s = qf @ k.transpose(-1, -2) * 0.125
    if mask is not None:
        s = s + mask[None]
    return (torch.softmax(s, -1) @ v).permute(1, 0, 2).reshape(-1, D)


def _check_ragged(dev, dtype, rows_per_set, Qp, Sk, H, splits, masked, seed):
    """fp32 torch attention within the uniform kernel's bound, every set bit-identical to the uniform launch over that set alone, a repeated
    launch bit-identical, rows that belong to no set untouched"""
    tag = (Qp, masked)
    q, kv, mask = _case(dev, dtype, rows_per_set, Qp, Sk, H, masked, seed=seed)
    o = _ragged(q, kv, mask, rows_per_set, Qp, Sk, H, splits, tail_rows=4)
    n = q.shape[0]
    assert bool((o[n:] == SENTINEL).all()), tag                 # only owned rows change
    assert torch.equal(o, _ragged(q, kv, mask, rows_per_set, Qp, Sk, H, splits, tail_rows=4)), tag
    r0 = 0
    for s, R in enumerate(rows_per_set):
        if R == 0:
            continue
        sl = slice(r0 * Qp, (r0 + R) * Qp)
        ms = mask[r0:r0 + R] if masked else None
        ref = _ref_set(q[sl], kv[s], ms.reshape(R * Qp, Sk) if masked else None, Sk, H)
        err = ((o[sl].float() - ref).abs().max() / ref.abs().max()).item()
        assert err < tol(dtype, 1.5), (tag, s, err)
        alone = _uniform(q[sl], kv[s:s + 1], ms, 1, R, Qp, Sk, H, splits)
        assert torch.equal(o[sl], alone), (tag, s)
        r0 += R


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows_per_set", [(1, 5, 2), (3, 0, 4)])
@pytest.mark.parametrize("Sk,splits", [(70, 1), (197, 2), (197, 3)])
def test_ragged_decode_attention(cuda, dtype, rows_per_set, Sk, splits):
    """A set smaller than one 4-query chunk, a set that ends mid-chunk, an empty set; with and without the key split and the mask
    (_check_ragged)."""
    for Qp in (2, 3):
        for masked in (False, True):
            _check_ragged(cuda, dtype, rows_per_set, Qp, Sk, 2, splits, masked, seed=Sk + 10 * Qp + sum(rows_per_set))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows_per_set", [(1, 2, 0, 1), (2,)])
@pytest.mark.parametrize("Sk,splits", [(70, 1), (197, 3)])
def test_ragged_decode_attention_two_query_instantiation(cuda, dtype, rows_per_set, Sk, splits):
    """One query per row and no set larger than two rows: the launch takes the 2-query instantiation (the cases above all reach the 4-query
    one).  Same assertions (_check_ragged)."""
    for masked in (False, True):
        _check_ragged(cuda, dtype, rows_per_set, 1, Sk, 2, splits, masked, seed=Sk + sum(rows_per_set))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_decode_attention_equals_uniform_on_equal_sets(cuda, dtype):
    H, Qp = 2, 3
    for R, Sk, splits in ((2, 70, 1), (2, 197, 3), (5, 197, 2)):
        q, kv, mask = _case(cuda, dtype, (R, R, R), Qp, Sk, H, True, seed=R + Sk)
        o = _ragged(q, kv, mask, (R, R, R), Qp, Sk, H, splits)
        assert torch.equal(o, _uniform(q, kv, mask, 3, R, Qp, Sk, H, splits)), (R, Sk, splits)


# ---------------------------------------------------------------------------------------------------------------------
# the cached step over ragged sets against the recomputing step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(cuda):
    m, sd = build_model("evaclip02_base", 2, device=cuda, max_answer_len=5)
    return m, sd


def test_teacher_forced_logits_ragged_sets(cuda, model):
    """(2, 1, 3) prompt rows x 3 beams on three condition sets, a padded 6-token question prompt + [CLS], 8 steps of a fixed random token
    sequence with beam permutations: the ragged cache's logits against the recomputing step on condition tokens expanded per row."""
    me = model[0].multimodal_encoder
    per_set, nb, steps = (2, 1, 3), 3, 8
    prompts = sum(per_set)
    rows = prompts * nb
    g = torch.Generator().manual_seed(21)
    cond = torch.randn(3, 9, 768, generator=g).to(cuda)
    q = torch.randint(1000, 30000, (prompts, 6), generator=g)
    kp = torch.ones(prompts, 6, dtype=torch.long)
    kp[1, 4:] = 0
    kp[4, 3:] = 0
    q = q * kp
    own = torch.arange(3).repeat_interleave(torch.tensor(per_set) * nb)
    worst = 0.0
    with runtime.precision(torch.float16), torch.no_grad():
        ids = torch.cat([q, torch.full((prompts, 1), 101)], 1).repeat_interleave(nb, dim=0).to(cuda)
        mask = me.update_attention_mask(kp[:, None, :].expand(prompts, 6, 6).contiguous()).repeat_interleave(nb, dim=0).to(cuda)
        dec = me._decode_cache(ids, mask, cond, [r * nb for r in per_set], ids.shape[1] + steps)
        assert dec.kvx.shape[0] == 3 * 9 and dec.set_row0.tolist() == [0, 6, 9, 18]
        enc = cond[own.to(cuda)].contiguous()
        parent = None
        for _ in range(steps):
            a = dec.next_token_logits(ids, parent).float()
            b = me.next_token_logits(ids, mask, enc, None).float()
            diff = ((a - b).abs().max() / b.abs().max()).item()
            worst = max(worst, diff)
            assert diff <= 2e-3, diff
            top2 = b.topk(2, dim=-1).values
            sure = (top2[:, 0] - top2[:, 1]) > (a - b).abs().max(dim=-1).values * 2
            assert torch.equal(a.argmax(-1)[sure], b.argmax(-1)[sure])
            tok = torch.randint(1000, 30000, (rows, 1), generator=g).to(cuda)
            # beam search: a row continues a parent among the beams of its own prompt row
            parent = torch.cat([p * nb + torch.randperm(nb, generator=g) for p in range(prompts)])
            ids = torch.cat([ids[parent.to(cuda)], tok], 1)
            mask = me.update_attention_mask(mask)
    print("max relative logit difference", worst)


# ---------------------------------------------------------------------------------------------------------------------
# forward_qa, training
# ---------------------------------------------------------------------------------------------------------------------
def _qa_batch(fx, cuda):
    meta = fx["meta"]
    inp = synth_inputs(dict(b=meta["b"], vision=meta["vision"], audio=meta["audio"], S=0), seed=meta["input_seed"])
    batch = {k: v.to(cuda) for k, v in inp.items()}
    for k in ("question_ids", "question_mask", "answer_ids", "answer_mask"):
        batch[k] = fx[k].to(cuda)
    batch["_injected"] = {"qa": dict(masked_ids=fx["masked_ids"], labels=fx["labels"])}
    return batch


@pytest.mark.parametrize("pc", PRECISION_CONFIGS)
def test_forward_qa_loss_against_reference(cuda, model, pc):
    """loss_qa and its gradients for qa%tv%tva against the reference's own multimodal_encoder on the same inputs: the bounds of
    tests/test_model_gpu.py::test_alignment_loss."""
    m = model[0]
    fx = golden("qa_b16_d2.pt")
    er = Errs(f"qa/{pc}")
    with precision_config(pc):
        m.zero_grad(set_to_none=True)
        out = m.forward_qa(_qa_batch(fx, cuda), fx["meta"]["task"], compute_loss=True)
        assert set(out) == {"loss_qa"}
        v = fx["loss_qa"].item()
        er.add("loss_qa", abs(out["loss_qa"].item() - v) / max(abs(v), 1e-6), 1e-3)
        out["loss_qa"].backward()
    named = dict(m.named_parameters())
    worst = ("", 0.0)
    for n, d in fx["grads"].items():
        ge = grad_digest_check(d, named[n].grad, None)
        if ge > worst[1]:
            worst = (n, ge)
    er.add(f"worst grad digest ({worst[0]})", worst[1], 5e-2)
    er.check()


def test_forward_qa_answer_rows_equal_the_full_row_head(cuda, model):
    """Only the answer rows go through the LM head: same loss and gradients as BertForMaskedLM(..., labels) over all Lq + La rows with -100
    over the question."""
    from mico_amd.model.mico_forward import qa_attention_mask
    m = model[0]
    fx = golden("qa_b16_d2.pt")
    subtasks = fx["meta"]["task"].split("%")[1:]
    with precision_config("parity"):
        m.zero_grad(set_to_none=True)
        loss = m.forward_qa(_qa_batch(fx, cuda), fx["meta"]["task"], compute_loss=True)["loss_qa"]
        loss.backward()
        got = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        m.zero_grad(set_to_none=True)
        batch = _qa_batch(fx, cuda)
        enc = m.encode_batch(batch)
        ids = torch.cat((batch["question_ids"], fx["masked_ids"].to(cuda)), dim=1)
        labels = torch.cat((torch.full_like(batch["question_ids"], -100), fx["labels"].to(cuda)), dim=1)
        m3 = qa_attention_mask(batch["question_mask"], batch["answer_mask"])
        full = sum(m.multimodal_encoder(input_ids=ids, attention_mask=m3, encoder_hidden_states=m._condition_feats(enc, st[1:]),
                                        labels=labels).loss for st in subtasks) / len(subtasks)
        full.backward()
    er = Errs("qa/answer rows")
    er.add("loss", abs(loss.item() - full.item()) / abs(full.item()), 1e-3)
    want = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert set(got) == set(want)
    worst = ("", 0.0)
    for n, g in want.items():
        e = ((got[n].float() - g.float()).abs().max() / g.float().abs().max().clamp_min(1e-20)).item()
        if e > worst[1]:
            worst = (n, e)
    er.add(f"worst gradient ({worst[0]})", worst[1], 5e-2)
    er.check()


# ---------------------------------------------------------------------------------------------------------------------
# forward_qa, evaluation
# ---------------------------------------------------------------------------------------------------------------------
EVAL_SEED = 77         # tests/qa_oracle.py:eval_case; chosen among seeds 0 .. 119 on the recomputing path's own logits: margin 5 x the bound, two distinct answers
NUM_QUESTIONS = [2, 1, 3]


def test_forward_qa_answers_with_and_without_the_cache(cuda):
    """b = 3 with 2, 1 and 3 questions, Lq = 8, max_answer_len 5: the answers of the recomputing decode (condition tokens copied per question)
    and of the ragged cached decode (each sample's tokens projected once) are the same - after the recomputing path's own logits have shown
    that no answer hangs on a near-tie (qa_oracle.beam_search_with_margins: every margin above 4 x 2e-3 of the largest logit, 2e-3 being
    the bound on the two paths' logit difference)."""
    torch.set_num_threads(16)
    m, _ = build_model("evaclip02_base", 2, device=cuda, max_answer_len=5)
    me = m.multimodal_encoder
    q, qm, toks, boost = qa_oracle.eval_case(EVAL_SEED)
    named = dict(m.named_parameters())
    with torch.no_grad():      # the test model: see qa_oracle.sharpen_keys / cross_value_keys / eval_case for what is changed and why
        for key in qa_oracle.sharpen_keys():
            named[key].mul_(qa_oracle.SHARPEN)
        for key in qa_oracle.cross_value_keys():
            named[key].mul_(qa_oracle.CROSS_GAIN)
        me.cls.predictions.bias[toks.to(cuda)] += boost.to(cuda)
    inp = synth_inputs(dict(b=3, vision=2, S=0), seed=8)
    batch = {k: v.to(cuda) for k, v in inp.items()}
    batch.update(question_ids=q.to(cuda), question_mask=qm.to(cuda), num_questions=NUM_QUESTIONS)
    nb = m.beam_size
    assert nb == 3 and m.max_answer_len == 5
    own = torch.arange(3).repeat_interleave(torch.tensor(NUM_QUESTIONS))
    with runtime.precision(torch.float16), torch.no_grad():
        cond = m._condition_feats(m.encode_batch(dict(batch)), "v")
        E = cond.shape[1]
        condx = cond[own.to(cuda)].repeat_interleave(nb, dim=0).contiguous()
        ids0, mask0 = qa_oracle.qa_prompt(q, qm)
        step = lambda ids, mask: me.next_token_logits(ids.to(cuda), mask.to(cuda), condx, None)
        ref_ids, margin, top = qa_oracle.beam_search_with_margins(step, ids0, mask0, nb, 5)
        print("beam-selection margin", margin, "largest logit", top, "required", 4 * 2e-3 * top)
        assert margin > 4 * 2e-3 * top, (margin, top)
        ref = me.tokenizer.batch_decode(ref_ids[:, 9:], skip_special_tokens=True)
        caches = []
        make = me._decode_cache
        me._decode_cache = lambda *a: caches.append(make(*a)) or caches[-1]
        Fn.BertDecodeCache.passes = []
        try:
            outs = []
            for cached in (False, True):
                m.config["decode_use_cache"] = cached
                outs.append(m.forward_qa(dict(batch), "qa%tv", compute_loss=False))
            passes = Fn.BertDecodeCache.passes
        finally:
            Fn.BertDecodeCache.passes = None
            del me._decode_cache
    print(outs, ref)
    assert outs[0] == outs[1] == {"generated_answers_tv": ref}
    assert len(ref) == 6 and len(set(ref)) > 1                 # flat in question order; the answers depend on question and sample
    assert passes[0] == (18, 10)                               # 6 questions x 3 beams: [question | [CLS]] + [MASK]
    assert len(passes) > 1 and passes[1:] == [(18, 2)] * (len(passes) - 1)
    (dec,) = caches
    assert dec.kvx.shape[0] == 3 * E and dec.sets == 3 and dec.set_row0.tolist() == [0, 6, 9, 18]


def test_demo_answers_with_cache(cuda, tmp_path):
    import inference_demo as demo
    from mico_amd.model import MiCo
    pdir = str(tmp_path / "MiCo-synth")
    demo.write_synthetic_pretrain_dir(pdir, "evaclip02_base", steps=(3,), vision_layers=1, max_vision_sample_num=8)
    ckpt, opts = demo.load_from_pretrained_dir(pdir)
    model = MiCo.from_pretrained(opts, ckpt).to(cuda).eval()
    x = torch.rand(1, 3, 224, 224, generator=torch.Generator().manual_seed(0))
    questions = ["what is the man doing?", "is it snowing?"]
    with runtime.precision(torch.float16):
        plain = demo.run_demo(model, x, ["a dog"], cuda)
        a = demo.run_demo(model, x, ["a dog"], cuda, questions=questions)
        b = demo.run_demo(model, x, ["a dog"], cuda, questions=questions, use_cache=True)
    assert "answers" not in plain and len(a["answers"]) == 2
    assert a["answers"] == b["answers"] and a["captions"] == b["captions"] == plain["captions"]
