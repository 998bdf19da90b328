"""Incremental caption decoding (BertForMaskedLM.generate(use_cache=True), functional.BertDecodeCache, mico_attn_decode):
the decode attention kernel against fp32 torch attention; the cached step's logits against the recomputing path under teacher forcing
(with beam re-gathers, and a padded bidirectional prompt); token ids against the oracle; MiCo.forward / demo captions with the cache
on and off; one prompt pass, then 2 positions per row and step."""
import pytest
import torch

from common import build_model
from mico_amd import functional as Fn
from mico_amd import ops, runtime
from oracle import mico_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def tol(dtype, k=1.0):
    return (2e-3 if dtype == torch.float16 else 1.6e-2) * k


def _decode_case(dev, dtype, sets, R, Qp, Sk, H=3, masked=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    D = H * 64
    q = torch.randn(sets * R * Qp, D, generator=g).to(dev, dtype)
    kv = torch.randn(sets, Sk, 2 * D, generator=g).to(dev, dtype)      # [K | V] per key, as the caches hold them
    mask = None
    if masked:
        mask = torch.where(torch.rand(sets * R, Qp, Sk, generator=g) < 0.3, -10000.0, 0.0).to(dev)
    return q, kv, mask


def _run(q, kv, mask, sets, R, Qp, Sk, H, splits=None):
    D = H * 64
    o = torch.empty_like(q)
    ops.attn_decode(q, kv, kv[:, :, D:], o, sets=sets, rows_per_set=R, q_per_row=Qp, H=H, Sk=Sk, hd=64, scale=0.125, q_rs=D,
                    kv_strides=(kv.stride(0), kv.stride(1)), o_rs=D, mask=mask,
                    mask_strides=(mask.stride(0), mask.stride(1)) if mask is not None else (0, 0), splits=splits)
    return o


def _ref(q, kv, mask, sets, R, Qp, Sk, H):
    D = H * 64
    qf = q.float().view(sets, R * Qp, H, 64).permute(0, 2, 1, 3)                 # [sets, H, QR, 64]
    k = kv[:, :, :D].float().view(sets, Sk, H, 64).permute(0, 2, 1, 3)
    v = kv[:, :, D:].float().view(sets, Sk, H, 64).permute(0, 2, 1, 3)
    s = qf @ k.transpose(-1, -2) * 0.125
    if mask is not None:
        s = s + mask.view(sets, 1, R * Qp, Sk)
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(sets * R * Qp, D)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Sk", [1, 7, 63, 64, 65, 257, 2056])
@pytest.mark.parametrize("R,Qp", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (5, 1), (5, 2)])
def test_attn_decode_matches_torch(cuda, dtype, Sk, R, Qp):
    for masked in (False, True):
        sets, H = 3, 3
        q, kv, mask = _decode_case(cuda, dtype, sets, R, Qp, Sk, H, masked, seed=Sk * 10 + R)
        o = _run(q, kv, mask, sets, R, Qp, Sk, H)
        ref = _ref(q, kv, mask, sets, R, Qp, Sk, H)
        err = ((o.float() - ref).abs().max() / ref.abs().max()).item()
        assert err < tol(dtype, 1.5), (masked, err)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attn_decode_key_split_and_determinism(cuda, dtype):
    """One set x one head cannot fill the chip: the keys are split (forced here at several widths, and the default choice); every
    split agrees with the reference, and a launch repeated is bit-identical (fixed-order combine, no atomics)."""
    sets, R, Qp, Sk, H = 1, 3, 2, 1000, 1
    q, kv, mask = _decode_case(cuda, dtype, sets, R, Qp, Sk, H, True, seed=5)
    assert ops.attn_decode_splits(sets, H, R * Qp, Sk) > 1
    ref = _ref(q, kv, mask, sets, R, Qp, Sk, H)
    for splits in (None, 1, 2, 3, 7, 16):
        a = _run(q, kv, mask, sets, R, Qp, Sk, H, splits)
        b = _run(q, kv, mask, sets, R, Qp, Sk, H, splits)
        assert torch.equal(a, b), splits
        err = ((a.float() - ref).abs().max() / ref.abs().max()).item()
        assert err < tol(dtype, 1.5), (splits, err)


def test_attn_decode_refuses_other_head_sizes(cuda):
    q = torch.zeros(2, 64, dtype=torch.float16, device=cuda)
    with pytest.raises(ops.MicoHipError, match="hd 64 only"):
        ops.attn_decode(q, q, q, q, sets=1, rows_per_set=1, q_per_row=2, H=2, Sk=2, hd=32, scale=1.0, q_rs=64, kv_strides=(128, 64), o_rs=64)


def _bert(cuda, sep_bias=0.0):
    m, sd = build_model("evaclip02_base", 1, device=cuda)
    sdo = dict(sd)
    sdo["multimodal_encoder.cls.predictions.decoder.weight"] = sdo["multimodal_encoder.bert.embeddings.word_embeddings.weight"]
    bias = sdo["multimodal_encoder.cls.predictions.bias"].clone()
    bias[102] += sep_bias
    sdo["multimodal_encoder.cls.predictions.bias"] = bias
    with torch.no_grad():
        m.multimodal_encoder.cls.predictions.bias.copy_(bias.to(cuda))
    return m, sdo


def _teacher_forced(me, ids0, mask0, cond, R, steps, permute, seed):
    """Decode a fixed random token sequence step by step with the cache and, at every step, recompute the same prefix without it."""
    g = torch.Generator().manual_seed(seed)
    rows = ids0.shape[0]
    dec = me._decode_cache(ids0, mask0, cond, R, ids0.shape[1] + steps)
    enc = cond.repeat_interleave(R, dim=0).contiguous()
    ids, mask, parent = ids0, mask0, None
    worst = 0.0
    for _ in range(steps):
        a = dec.next_token_logits(ids, parent).float()
        b = me.next_token_logits(ids, mask, enc, None).float()
        diff = ((a - b).abs().max() / b.abs().max()).item()
        worst = max(worst, diff)
        assert diff <= 2e-3, diff
        top2 = b.topk(2, dim=-1).values
        sure = (top2[:, 0] - top2[:, 1]) > (a - b).abs().max(dim=-1).values * 2
        assert torch.equal(a.argmax(-1)[sure], b.argmax(-1)[sure])
        tok = torch.randint(1000, 30000, (rows, 1), generator=g).to(ids.device)
        if permute:     # beam search: a row continues a parent row of its own set
            parent = torch.cat([s * R + torch.randperm(R, generator=g) for s in range(rows // R)])
            ids = ids[parent.to(ids.device)]
        ids = torch.cat([ids, tok], 1)
        mask = me.update_attention_mask(mask)
    return worst


def test_teacher_forced_logits_bos_beams(cuda):
    m, _ = _bert(cuda)
    me = m.multimodal_encoder
    g = torch.Generator().manual_seed(11)
    cond = torch.randn(2, 7, 768, generator=g).to(cuda)
    with runtime.precision(torch.float16), torch.no_grad():
        ids = torch.full((6, 1), 101, dtype=torch.long, device=cuda)
        worst = _teacher_forced(me, ids, ids.new_ones(6, 1, 1), cond, 3, 10, True, 1)
    print("max relative logit difference", worst)


def test_teacher_forced_logits_padded_question_prompt(cuda):
    """vast.py:618-623: a padded question prefix + [BOS], its key-padding mask expanded to [b, Q, Q] and grown once."""
    m, _ = _bert(cuda)
    me = m.multimodal_encoder
    g = torch.Generator().manual_seed(12)
    cond = torch.randn(2, 9, 768, generator=g).to(cuda)
    q = torch.randint(1000, 30000, (2, 6), generator=g)
    kp = torch.ones(2, 6, dtype=torch.long)
    kp[1, 4:] = 0
    q[1, 4:] = 0
    with runtime.precision(torch.float16), torch.no_grad():
        ids = torch.cat([q, torch.full((2, 1), 101)], 1).to(cuda)
        mask = me.update_attention_mask(kp[:, None, :].expand(2, 6, 6).contiguous()).to(cuda)
        worst = _teacher_forced(me, ids, mask, cond, 1, 8, False, 2)
    print("max relative logit difference", worst)


@pytest.mark.parametrize("num_beams,sep_bias,max_new", [(1, 0.0, 6), (3, 0.0, 6), (3, 1.2, 8), (3, 1.5, 8), (3, 1.7, 8), (2, 1.6, 8), (2, 1.8, 8)])
def test_cached_generate_matches_oracle(cuda, num_beams, sep_bias, max_new):
    torch.set_num_threads(16)
    m, sdo = _bert(cuda, sep_bias)
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(3, 7, 768, generator=g)
    with torch.no_grad():
        ref = O.generate_beam(sdo, cond, max_new, num_beams, 0.6)
    tk = m.multimodal_encoder.tokenizer
    with runtime.precision(torch.float16):
        init = torch.full((3, 1), tk.bos_token_id, dtype=torch.long, device=cuda)
        out = m.multimodal_encoder.generate(input_ids=init, attention_mask=init.new_ones(3, 1, 1), encoder_hidden_states=cond.to(cuda),
                                            max_new_tokens=max_new, num_beams=num_beams, eos_token_id=tk.sep_token_id,
                                            pad_token_id=tk.pad_token_id, length_penalty=0.6, use_cache=True)
    print(num_beams, sep_bias, out.tolist(), ref.tolist())
    assert out.cpu().tolist() == ref.tolist()


@pytest.mark.parametrize("sep_bias,max_new,nrs", [(0.0, 6, 1), (2.5, 8, 1), (4.0, 8, 1), (2.5, 8, 3)])
def test_cached_sampling_matches_oracle(cuda, sep_bias, max_new, nrs):
    torch.set_num_threads(16)
    m, sdo = _bert(cuda, sep_bias)
    g = torch.Generator().manual_seed(4)
    cond = torch.randn(4, 7, 768, generator=g)
    noise = torch.rand(4 * nrs, max_new, generator=g)
    tk = m.multimodal_encoder.tokenizer
    me = m.multimodal_encoder
    with runtime.precision(torch.float16), torch.no_grad():
        init = torch.full((4, 1), tk.bos_token_id, dtype=torch.long, device=cuda)
        out = me.generate(input_ids=init, attention_mask=init.new_ones(4, 1, 1), encoder_hidden_states=cond.to(cuda),
                          max_new_tokens=max_new, do_sample=True, top_k=10, eos_token_id=tk.sep_token_id,
                          pad_token_id=tk.pad_token_id, sample_noise=noise, use_cache=True, num_return_sequences=nrs)
        # the oracle's sampling loop (on the expanded, sample-major condition) over the product's CACHED step: the search must agree token
        # for token.  (Against the recomputing step's logits the draws can differ: with random-init weights the ten kept logits of 30522
        # nearly flat ones reorder within 16-bit rounding - the case (2.5, 8, 1) does at its first step; the logits themselves are gated
        # by the teacher-forced tests above.)
        condx = cond.repeat_interleave(nrs, dim=0)
        init_x = init.repeat_interleave(nrs, dim=0)
        dec = me._decode_cache(init_x, init_x.new_ones(4 * nrs, 1, 1), cond.to(cuda), nrs, 1 + max_new)
        step = lambda ids, mask: dec.next_token_logits(ids.to(cuda)).float().cpu()
        ref = O.generate_sample(sdo, condx, max_new, 10, noise, step_logits=step)
    print(sep_bias, nrs, out.tolist(), ref.tolist())
    assert out.cpu().tolist() == ref.tolist()


def test_forward_cap_with_decode_cache(cuda):
    """MiCo.forward(batch, "cap%tv", compute_loss=False): config decode_use_cache returns the captions of the recomputing path, for the
    beam search and for captioner_mode (unexpanded condition + num_return_sequences)."""
    from mico_amd.weights import synth_inputs
    torch.set_num_threads(16)
    inp = synth_inputs(dict(b=2, vision=2, S=8), seed=8)
    batch = {k: v.to(cuda) for k, v in inp.items()}
    for over in (dict(max_caption_len=6), dict(max_caption_len=5, captioner_mode=True, generate_nums=3)):
        m, sd = build_model("evaclip02_base", 1, device=cuda, **over)
        noise = torch.rand(6, 5, generator=torch.Generator().manual_seed(1))
        outs = []
        for cached in (False, True):
            m.config["decode_use_cache"] = cached
            b = dict(batch)
            if over.get("captioner_mode"):
                b["_injected"] = {"sample_noise": noise}
            with runtime.precision(torch.float16), torch.no_grad():
                outs.append(m(b, "cap%tv", compute_loss=False))
        print(over, outs)
        if not over.get("captioner_mode"):
            assert outs[0] == outs[1]
            continue
        # captioner_mode: the oracle's sampling loop over the cached step on the unexpanded condition (3 rows per set, sample-major
        # noise).  The recomputing path's draws may differ where the ten kept random-init logits nearly tie (see the sampling test).
        sdo = dict(sd)
        sdo["multimodal_encoder.cls.predictions.decoder.weight"] = sdo["multimodal_encoder.bert.embeddings.word_embeddings.weight"]
        me = m.multimodal_encoder
        with runtime.precision(torch.float16), torch.no_grad():
            cond = m._condition_feats(m.encode_batch(dict(batch)), "v")
            init = torch.full((6, 1), 101, dtype=torch.long, device=cuda)
            dec = me._decode_cache(init, init.new_ones(6, 1, 1), cond, 3, 6)
            step = lambda ids, mask: dec.next_token_logits(ids.to(cuda)).float().cpu()
            ref = O.generate_sample(sdo, cond.repeat_interleave(3, dim=0).float().cpu(), 5, 10, noise, step_logits=step)
        assert outs[1] == {"generated_captions_tv": me.tokenizer.batch_decode(ref[:, 1:], skip_special_tokens=True)}


def test_demo_caption_with_cache(cuda, tmp_path):
    import inference_demo as demo
    from mico_amd.model import MiCo
    pdir = str(tmp_path / "MiCo-synth")
    demo.write_synthetic_pretrain_dir(pdir, "evaclip02_base", steps=(3,), vision_layers=1, max_vision_sample_num=8)
    ckpt, opts = demo.load_from_pretrained_dir(pdir)
    model = MiCo.from_pretrained(opts, ckpt).to(cuda).eval()
    x = torch.rand(1, 3, 224, 224, generator=torch.Generator().manual_seed(0))
    with runtime.precision(torch.float16):
        a = demo.run_demo(model, x, ["a dog"], cuda)
        b = demo.run_demo(model, x, ["a dog"], cuda, use_cache=True)
    assert a["caption_ids"].tolist() == b["caption_ids"].tolist() and a["captions"] == b["captions"]


def test_one_prompt_pass_then_two_positions_per_step(cuda, monkeypatch):
    m, _ = _bert(cuda)
    me = m.multimodal_encoder
    full = []
    orig = Fn.BertFn.apply
    monkeypatch.setattr(Fn.BertFn, "apply", lambda *a: full.append(1) or orig(*a))
    Fn.BertDecodeCache.passes = []
    try:
        cond = torch.randn(2, 7, 768, generator=torch.Generator().manual_seed(6)).to(cuda)
        with runtime.precision(torch.float16):
            init = torch.full((2, 1), 101, dtype=torch.long, device=cuda)
            out = me.generate(input_ids=init, attention_mask=init.new_ones(2, 1, 1), encoder_hidden_states=cond, max_new_tokens=7,
                              num_beams=3, eos_token_id=None, pad_token_id=0, length_penalty=0.6, use_cache=True)
        passes = Fn.BertDecodeCache.passes
    finally:
        Fn.BertDecodeCache.passes = None
    assert out.shape == (2, 8)
    assert not full                                   # no recomputing BERT forward
    assert passes[0] == (6, 2)                        # prompt ([BOS]) + [MASK] of 2 x 3 rows
    assert passes[1:] == [(6, 2)] * 6                 # then the chosen token and the new [MASK] per row and step
