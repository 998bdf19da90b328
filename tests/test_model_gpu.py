"""Parity of the HIP product path (mico_amd.model on libmico_hip.so) against (a) golden fixtures produced by the reference
itself and (b) the CPU oracle on the same seeded inputs.  Bar (BASELINE.json north_star): embeddings / logits within 1e-3
(max-abs error over max-abs reference) in the fp16 configuration, integer outputs bit-exact; the bf16 throughput
configuration is checked against a looser, stated bound.  Gradients: 2e-2 (fp16, carried with a 4096x internal scale)."""
import pytest
import torch
import torch.nn.functional as F

from common import golden, rel_err, build_model, grad_digest_check, precision_config, Errs, PRECISION_CONFIGS
from mico_amd import runtime
from mico_amd.weights import synth_inputs
from oracle import mico_oracle as O

pytestmark = pytest.mark.gpu

FWD_TOL = {torch.float16: 1e-3, torch.bfloat16: 1.2e-2}
GRAD_TOL = {torch.float16: 2e-2, torch.bfloat16: 6e-2}


@pytest.fixture(scope="module", params=[("evaclip02_base", "b16_d2"), ("evaclip01_giant", "g14_d2")])
def setup(request, cuda):
    vtype, tag = request.param
    m, sd = build_model(vtype, 2, device=cuda)
    return vtype, tag, m, sd


def err_vs(a, b, scale):
    return ((a.detach().float().cpu() - b.float()).abs().max() / float(scale)).item()


def to_dev(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_vit_tower(setup, cuda, dtype):
    vtype, tag, m, sd = setup
    fx = golden(f"vit_{tag}.pt")
    g = torch.Generator().manual_seed(fx["meta"]["input_seed"])
    x = torch.randn((2, 3, 224, 224), generator=g)
    w = torch.randn(fx["out"].shape, generator=g) / fx["out"].numel() ** 0.5
    m.zero_grad(set_to_none=True)
    with runtime.precision(dtype):
        out = m.vision_encoder.visual(x.to(cuda), return_all_features=True)
        assert out.shape == fx["out"].shape
        e = rel_err(out, fx["out"])
        print(f"{tag} {dtype} fwd rel err {e:.2e}")
        assert e < FWD_TOL[dtype]
        (out * w.to(cuda)).sum().backward()
    named = dict(m.vision_encoder.visual.named_parameters())
    worst = 0.0
    for n, d in fx["grads"].items():
        ge = grad_digest_check(d, named[n].grad, None)
        worst = max(worst, ge)
        assert ge < GRAD_TOL[dtype], (n, ge)
    print(f"{tag} {dtype} worst grad err {worst:.2e}")


@pytest.mark.parametrize("chunk", [None, 1])
def test_vit_tower_head_split(setup, cuda, chunk):
    """bench.py's timed precision: plain fp16 with the first blocks' forward GEMMs weights-split (runtime.CFG.head_split_blocks; here block 0
    split, block 1 plain) - forward and parameter gradients against the reference goldens, also through the chunked-recompute path (the
    recomputed forward and the backward must pick the same per-block weight layouts)."""
    vtype, tag, m, sd = setup
    fx = golden(f"vit_{tag}.pt")
    g = torch.Generator().manual_seed(fx["meta"]["input_seed"])
    x = torch.randn((2, 3, 224, 224), generator=g)
    w = torch.randn(fx["out"].shape, generator=g) / fx["out"].numel() ** 0.5
    m.zero_grad(set_to_none=True)
    old = runtime.snapshot()
    try:
        runtime.CFG.split_fp16, runtime.CFG.head_split_blocks = False, 1
        runtime.set_tower_chunk(chunk)
        with runtime.precision(torch.float16):
            out = m.vision_encoder.visual(x.to(cuda), return_all_features=True)
            assert runtime.snapshot()[1:] == (False, old[2], old[3], 1, old[5])      # the per-block state does not leak out of the tower
            e = rel_err(out, fx["out"])
            (out * w.to(cuda)).sum().backward()
    finally:
        runtime.set_tower_chunk(None)
        runtime.restore(old)
    named = dict(m.vision_encoder.visual.named_parameters())
    worst = max(grad_digest_check(d, named[n].grad, None) for n, d in fx["grads"].items())
    print(f"{tag} head-split fwd rel err {e:.2e} worst grad err {worst:.2e}")
    assert e < FWD_TOL[torch.float16] and worst < GRAD_TOL[torch.float16]      # the gate itself (measured: B/16 6.1e-4, g/14 4.6e-4)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_vit_tower_large(cuda, dtype):
    """EVA02-CLIP-L/14 (mico.py:336-340): RoPE + sub-LN + SwiGLU with hidden = int(1024 * 2.6667) = 2730, which is not a multiple of 8 -
    the engine runs it in 2752-wide zero-padded buffers (functional.TowerSpec.hidden_pad; LayerNorm statistics over the 2730 valid
    columns).  Same gates as the other towers, against the reference's own outputs (tests/golden/vit_l14_d2.pt)."""
    m, sd = build_model("evaclip02_large", 2, device=cuda)
    fx = golden("vit_l14_d2.pt")
    g = torch.Generator().manual_seed(fx["meta"]["input_seed"])
    x = torch.randn((2, 3, 224, 224), generator=g)
    w = torch.randn(fx["out"].shape, generator=g) / fx["out"].numel() ** 0.5
    m.zero_grad(set_to_none=True)
    with runtime.precision(dtype):
        out = m.vision_encoder.visual(x.to(cuda), return_all_features=True)
        assert out.shape == fx["out"].shape
        e = rel_err(out, fx["out"])
        print(f"l14_d2 {dtype} fwd rel err {e:.2e}")
        assert e < FWD_TOL[dtype]
        (out * w.to(cuda)).sum().backward()
    named = dict(m.vision_encoder.visual.named_parameters())
    worst = 0.0
    for n, d in fx["grads"].items():
        ge = grad_digest_check(d, named[n].grad, None)
        worst = max(worst, ge)
        assert ge < GRAD_TOL[dtype], (n, ge)
    print(f"l14_d2 {dtype} worst grad err {worst:.2e}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("drop_path", [False, True])
def test_vit_tower_bige_postnorm(cuda, dtype, drop_path):
    """EVA02-CLIP-bigE-14-plus (mico.py:341-344): the POST-norm block order x + drop_path(norm(branch(x))) (eva_vit_model.py:411-413), width
    1792, head dim 112, hidden 15360 - forward and every parameter-gradient digest against the reference's own EVAVisionTransformer
    (tests/golden/vit_bige_d2.pt); with injected stochastic-depth scales against the oracle (pinned to that golden by
    tests/test_oracle_vs_golden.py::test_vit_tower_bige_postnorm)."""
    from oracle import mico_oracle as O
    m, sd = build_model("evaclip02_bige", 2, device=cuda)
    fx = golden("vit_bige_d2.pt")
    g = torch.Generator().manual_seed(fx["meta"]["input_seed"])
    x = torch.randn((2, 3, 224, 224), generator=g)
    w = torch.randn(fx["out"].shape, generator=g) / fx["out"].numel() ** 0.5
    vis = m.vision_encoder.visual
    m.zero_grad(set_to_none=True)
    dps = None
    if drop_path:
        dps = torch.tensor([[[1.25, 0.0], [1.25, 1.25]], [[0.0, 1.6], [1.6, 0.0]]])     # [depth, branch, frame]: 0 or 1 / keep
    with runtime.precision(dtype):
        out = vis.forward_groups([x.to(cuda)], drop_path_scale=dps)
        (out * w.to(cuda)).sum().backward()
    named = dict(vis.named_parameters())
    if not drop_path:
        e = rel_err(out, fx["out"])
        worst = max(grad_digest_check(d, named[n].grad, None) for n, d in fx["grads"].items())
    else:
        sdo = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
        ref = O.eva_vit_forward(sdo, x, O.ARCHS["evaclip02_bige"], drop_path_scale=dps)
        (ref * w).sum().backward()
        e = rel_err(out, ref)
        worst = 0.0
        for n, p in named.items():
            if n.startswith("head."):
                continue
            gr = sdo["vision_encoder.visual." + n].grad
            worst = max(worst, ((p.grad.cpu() - gr).abs().max() / gr.abs().max().clamp_min(1e-20)).item())
    print(f"bige_d2 {dtype} drop_path={drop_path}: fwd rel err {e:.2e}, worst grad err {worst:.2e}")
    assert e < FWD_TOL[dtype] and worst < GRAD_TOL[dtype]
    if not drop_path:   # the no-grad pass (nothing saved) and the facade's vision branch produce the same tokens / a [b, n, 1792] feature
        with torch.no_grad(), runtime.precision(dtype):
            assert torch.equal(vis.forward_groups([x.to(cuda)]), out)
            fv = m.forward_vision_encoder(x.to(cuda).unsqueeze(1))
        assert fv.shape[0] == 2 and fv.shape[-1] == 1792 and torch.isfinite(fv).all()


@pytest.mark.parametrize("pc", PRECISION_CONFIGS)
def test_bert(setup, cuda, pc):
    """BERT (self-only, cross-attention with a 2-D mask, causal cross-attention + LM head + CE) against the reference's own outputs, in
    the parity configuration AND in the precision bench.py times (plain fp16: common.precision_config): sequence outputs and the loss at
    the 1e-3 gate of SURVEY section 8d, argmax ids bit-exact where the reference decides, gradients at the 2e-2 gradient gate."""
    vtype, tag, m, sd = setup
    if tag != "b16_d2":
        pytest.skip("tower independent")
    fx = golden("bert.pt")
    g = torch.Generator().manual_seed(fx["meta"]["seed"])
    b, S, E = fx["meta"]["b"], fx["meta"]["S"], fx["meta"]["E"]
    ids = torch.randint(1000, 30000, (b, S), generator=g)
    ids[:, 0] = 101
    mask = (torch.arange(S)[None] < fx["meta"]["lens"][:, None]).long()
    ids = ids * mask
    cond = torch.randn((b, E, 768), generator=g)
    ids, mask, cond = ids.to(cuda), mask.to(cuda), cond.to(cuda)
    me = m.multimodal_encoder
    er = Errs(f"bert/{pc}")
    with precision_config(pc):
        def ids_exact(tag, logits):
            """argmax token ids bit-exact wherever the reference itself decides: its gap between the two largest
            logits of the position exceeds 2e-3 of max|logit|, twice the 1e-3 gate on the logits.  The other positions (6 + 1 + 1 of
            3 x 48 with these random-init weights; the fixture records them) are ties at that resolution: there the product must
            still name one of the reference's two candidates."""
            got = logits.argmax(-1).cpu()
            decided = fx[tag + "_top2_gap"] > 2e-3
            assert decided.float().mean() > 0.85
            assert torch.equal(got[decided], fx[tag + "_argmax"][decided]), (tag, (got != fx[tag + "_argmax"]).nonzero())
            assert (got[..., None] == fx[tag + "_top2_ids"]).any(-1).all(), tag

        o = me(input_ids=ids, attention_mask=mask)
        er.add("self_seq", rel_err(o.sequence_output, fx["self_seq"]), 1e-3)
        ids_exact("self", o.logits)
        o = me(input_ids=ids, attention_mask=mask, encoder_hidden_states=cond)
        er.add("cross_seq", rel_err(o.sequence_output, fx["cross_seq"]), 1e-3)
        ids_exact("cross", o.logits)
        m3 = torch.tril(mask.unsqueeze(1).expand(-1, S, -1)).contiguous()
        m.zero_grad(set_to_none=True)
        cr = cond.clone().requires_grad_(True)
        o = me(input_ids=ids, attention_mask=m3, encoder_hidden_states=cr, labels=fx["labels"].to(cuda))
        er.add("causal_seq", rel_err(o.sequence_output, fx["causal_seq"]), 1e-3)
        er.add("causal_loss", abs(o.loss.item() - fx["causal_loss"].item()) / fx["causal_loss"].item(), 1e-3)
        o.loss.backward()
    er.add("causal_dcond", rel_err(cr.grad, fx["causal_dcond"]), GRAD_TOL[torch.float16])
    named = dict(me.named_parameters())
    worst = max(grad_digest_check(d, named[n].grad, None) for n, d in fx["causal_grads"].items())
    er.add("causal_param_grads(worst)", worst, GRAD_TOL[torch.float16])
    er.check()


@pytest.mark.parametrize("pc", PRECISION_CONFIGS)
def test_facade(setup, cuda, pc):
    """The MiCo facade against the reference's own outputs, in the parity configuration and in bench.py's timed precision: every tensor
    SURVEY section 8d names at 1e-3 (max|out - ref| / max|ref|)."""
    vtype, tag, m, sd = setup
    fx = golden(f"facade_{tag}.pt")
    cfgs = {"n1": dict(b=2, vision=1, audio=1, depth=1, S=20), "n4": dict(b=2, vision=4, audio=4, depth=1, S=20),
            "n3": dict(b=2, vision=3, audio=2, depth=1, S=20)}
    tol = 1e-3
    er = Errs(f"facade/{tag}/{pc}")
    with precision_config(pc), torch.no_grad():
        for name, c in cfgs.items():
            r = fx[name]
            inp = to_dev(synth_inputs(c, seed=100), cuda)
            vo = m.forward_vision_encoder(inp["vision_pixels"])
            ao = m.forward_audio_encoder(inp["audio_spectrograms"])
            do = m.forward_depth_encoder(inp["depth_pixels"])
            # metric of SURVEY.md section 8d: max|out - ref| / max|ref| over the feature tensor (the fixture keeps 3 token
            # rows per frame; the tensor-wide max is taken from the product output)
            er.add(f"{name} vision rows", err_vs(vo[:, :, [0, 1, 50]], r["vision_out_rows"], vo.abs().max()), tol)
            er.add(f"{name} audio rows", err_vs(ao[:, :, [0, 1, 50]], r["audio_out_rows"], ao.abs().max()), tol)
            from mico_amd.functional import l2_normalize
            pv_, pa_, pd_ = m.pool_vision_for_contra(vo), m.pool_audio_for_contra(ao), m.pool_depth_for_contra(do)
            fv = l2_normalize(m.contra_head_v(pv_))
            er.add(f"{name} feat_v", rel_err(fv, r["feat_v"]), tol)
            er.add(f"{name} feat_a", rel_err(l2_normalize(m.contra_head_a(pa_)), r["feat_a"]), tol)
            er.add(f"{name} feat_d", rel_err(l2_normalize(m.contra_head_d(pd_)), r["feat_d"]), tol)
            er.add(f"{name} feat_va", rel_err(l2_normalize(m.contra_head_va(torch.cat((pv_, pa_), 1))), r["feat_va"]), tol)
            er.add(f"{name} feat_vd", rel_err(l2_normalize(m.contra_head_id(torch.cat((pv_, pd_), 1))), r["feat_vd"]), tol)
            to = m.forward_multimodal_encoder(inp["input_ids"], inp["attention_mask"]).sequence_output
            ft = l2_normalize(m.contra_head_t(m.pool_text_for_contra(to)))
            er.add(f"{name} feat_t", rel_err(ft, r["feat_t"]), tol)
            # cosine-similarity logits live in [-1, 1]: error measured against that range (random features are near
            # orthogonal, so max|sim| itself is ~0.02 here)
            er.add(f"{name} sim_t2v", (ft @ fv.t() - r["sim_t2v"].to(cuda)).abs().max().item(), tol)
            for pv, k in ((False, "full"), (True, "pv")):
                m.config.pool_video = pv
                cv = m.get_multimodal_forward_input_vision(vo)
                ca = m.get_multimodal_forward_input_audio(ao)
                cd = m.get_multimodal_forward_input_depth(do)
                er.add(f"{name} cond_v_{k} rows", err_vs(cv[:, [0, 1, cv.shape[1] - 1]], r[f"cond_v_{k}_rows"], cv.abs().max()), tol)
                er.add(f"{name} cond_v_{k} sum", rel_err(cv.sum((1, 2)), r[f"cond_v_{k}_sum"]), tol)
                er.add(f"{name} cond_a_{k} rows", err_vs(ca[:, [0, 1, ca.shape[1] - 1]], r[f"cond_a_{k}_rows"], ca.abs().max()), tol)
                er.add(f"{name} cond_d_{k} rows", err_vs(cd[:, [0, 1, cd.shape[1] - 1]], r[f"cond_d_{k}_rows"], cd.abs().max()), tol)
                out = m.forward_multimodal_encoder(inp["input_ids"], inp["attention_mask"], cv).sequence_output
                score = F.softmax(m.itm_head(out[:, 0]), dim=1)[:, 1]
                er.add(f"{name} itm_score_{k}", rel_err(score, r[f"itm_score_{k}"]), tol)
            m.config.pool_video = False
    er.check()


@pytest.mark.parametrize("pc", PRECISION_CONFIGS)
@pytest.mark.parametrize("W", [1, 2, 4])
def test_alignment_loss(setup, cuda, W, pc):
    """ITC + ITM + CAP of vast.py against the reference's own losses and gradient digests (W = 1 and simulated 2 / 4 ranks), in the parity
    configuration and in bench.py's timed precision: scalar losses at 1e-3 relative."""
    vtype, tag, m, sd = setup
    fx = golden(f"loss_{tag}.pt")
    r = fx[f"W{W}"]
    b = fx["meta"]["b"]
    inputs = [to_dev(synth_inputs(dict(b=b, vision=2, audio=1, S=12), seed=1234 + k), cuda) for k in range(W)]
    batch = dict(inputs[0])
    batch["_injected"] = {st: {k: r["inj"][st][k] for k in ("neg_cond_idx", "neg_text_idx")} for st in ("tva", "tv")}
    batch["_injected"]["cap"] = r["inj"]["cap"]
    er = Errs(f"loss/{tag}/W{W}/{pc}")
    with precision_config(pc):
        if W >= 2:
            with torch.no_grad():
                encs = [m.encode_batch(dict(i)) for i in inputs[1:]]
                remote = {c: torch.cat([m._condition_feats(e, c).detach() for e in encs]) for c in ("v", "va")}
            world = dict(rank=0, feat_t_all=r["world"]["feat_t_all"].to(cuda), ids_all=r["world"]["ids_all"].to(cuda),
                         mask_all=r["world"]["mask_all"].to(cuda))
            for c in ("v", "va"):
                world[f"feat_{c}_all"] = r["world"][f"feat_{c}_all"].to(cuda)
                world[f"cond_{c}_fetch"] = (lambda rc: (lambda cond, idx: torch.cat((cond, rc))[idx]))(remote[c])
            batch["_world"] = world
        m.zero_grad(set_to_none=True)
        out = m(batch, fx["meta"]["task"], compute_loss=True)
        for k, v in r["losses"].items():
            er.add(k, abs(out[k].item() - v.item()) / max(abs(v.item()), 1e-6), 1e-3)
        sum(out.values()).backward()
    named = dict(m.named_parameters())
    worst = ("", 0.0)
    for n, d in r["grads"].items():
        ge = grad_digest_check(d, named[n].grad, None)
        if ge > worst[1]:
            worst = (n, ge)
    er.add(f"worst grad digest ({worst[0]})", worst[1], 5e-2)
    er.check()


def test_shared_cross_kv_equals_per_pass_projection(setup, cuda):
    """runtime.CFG.share_cross_kv (the step's condition tokens projected to cross-attention K/V once, read by the ITM triplet through
    kv_batch_mod and again by the captioning pass) against the reference's per-pass projection: same losses, same gradients -
    in particular of the key / value projections, whose gradient now arrives through functional.CrossKVFn."""
    vtype, tag, m, sd = setup
    fx = golden(f"loss_{tag}.pt")
    r = fx["W1"]
    b = fx["meta"]["b"]
    batch0 = to_dev(synth_inputs(dict(b=b, vision=2, audio=1, S=12), seed=1234), cuda)
    from mico_amd import functional as Fn
    res, concat, accum = {}, {}, {}
    # per-pass projection; the shared memory (one projection GEMM, one K = L * 2 D product for the token gradient)
    # (second field: functional.DkvSession - the captioning pass and the ITM triplet keep ONE gradient buffer for the own set they both read;
    # off = a buffer per pass, summed by autograd)
    for share, inplace in ((False, True), (True, True), (True, False)):
        batch = dict(batch0)
        batch["_injected"] = {st: {k: r["inj"][st][k] for k in ("neg_cond_idx", "neg_text_idx")} for st in ("tva", "tv")}
        batch["_injected"]["cap"] = r["inj"]["cap"]
        old = runtime.CFG.share_cross_kv, runtime.CFG.dkv_inplace
        runtime.CFG.share_cross_kv, runtime.CFG.dkv_inplace = share, inplace
        c0, a0 = Fn.CrossKVFn.concat_backwards, Fn.DkvSession.accumulated
        try:
            with runtime.precision(torch.float16):
                m.zero_grad(set_to_none=True)
                out = m(batch, fx["meta"]["task"], compute_loss=True)
                sum(out.values()).backward()
        finally:
            runtime.CFG.share_cross_kv, runtime.CFG.dkv_inplace = old
        concat[(share, inplace)] = Fn.CrossKVFn.concat_backwards - c0
        accum[(share, inplace)] = Fn.DkvSession.accumulated - a0
        res[(share, inplace)] = ({k: v.item() for k, v in out.items()},
                                 {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    assert concat[(True, True)] > 0 and concat[(True, False)] > 0 and concat[(False, True)] == 0, concat
    # the task's captioning pass shares the tva memory with the tva triplet: exactly one of the two adds to the other's buffer - and only
    # with the session on
    assert accum == {(False, True): 0, (True, True): 1, (True, False): 0}, accum
    ref_l, ref_g = res[(False, True)]
    for key in ((True, True), (True, False)):
        for k in ref_l:
            assert abs(res[key][0][k] - ref_l[k]) <= 2e-4 * max(1.0, abs(ref_l[k])), (key, k)
        assert set(res[key][1]) == set(ref_g)
        worst = ("", 0.0)
        for n, g0 in ref_g.items():
            if n.endswith("self.key.bias"):   # analytically zero (a constant added to every score of a softmax row): rounding noise only
                continue
            e = rel_err(res[key][1][n], g0) if g0.abs().max() > 0 else float(res[key][1][n].abs().max())
            if e > worst[1]:
                worst = (n, e)
        print(tag, "shared", "one dK/dV buffer" if key[1] else "a buffer per pass", "vs per-pass K/V: worst gradient difference", worst)
        assert worst[1] < 5e-3, (key, worst)
        assert any("crossattention.self.key.weight" in n for n in res[key][1])


def test_staged_backward_equals_direct(setup, cuda):
    """MiCo.forward(backward_scale=...) (round 6: the BERT passes differentiated one condition set at a time inside the forward, the condition-token
    gradients handed to the towers by one _StagedLoss node) against the direct form: same losses, same gradients for every parameter - towers, BERT,
    heads - also with a loss scale other than 1 (the caller's backward of scale * sum)."""
    vtype, tag, m, sd = setup
    fx = golden(f"loss_{tag}.pt")
    r = fx["W1"]
    b = fx["meta"]["b"]
    batch0 = to_dev(synth_inputs(dict(b=b, vision=2, audio=1, S=12), seed=1234), cuda)
    res = {}
    for name, scale in (("direct", None), ("staged", 1.0), ("staged-x8", 8.0)):
        batch = dict(batch0)
        batch["_injected"] = {st: {k: r["inj"][st][k] for k in ("neg_cond_idx", "neg_text_idx")} for st in ("tva", "tv")}
        batch["_injected"]["cap"] = r["inj"]["cap"]
        with runtime.precision(torch.float16):
            m.zero_grad(set_to_none=True)
            out = m(batch, fx["meta"]["task"], compute_loss=True, backward_scale=scale)
            if scale is not None:      # the BERT side is already differentiated: its cross-attention projections have their gradients now
                assert any(p.grad is not None for n, p in m.named_parameters() if "crossattention.self.key.weight" in n)
                assert all(p.grad is None for n, p in m.named_parameters() if n.startswith("vision_encoder."))
            (sum(out.values()) * (scale or 1.0)).backward()
        res[name] = ({k: v.item() for k, v in out.items()},
                     {n: p.grad.clone() / (scale or 1.0) for n, p in m.named_parameters() if p.grad is not None})
    ref_l, ref_g = res["direct"]
    assert set(ref_l) == {"loss_itc", "loss_itm", "loss_cap"}
    for key in ("staged", "staged-x8"):
        for k in ref_l:
            assert abs(res[key][0][k] - ref_l[k]) <= 2e-4 * max(1.0, abs(ref_l[k])), (key, k, res[key][0][k], ref_l[k])
        assert set(res[key][1]) == set(ref_g)
        worst = ("", 0.0)
        for n, g0 in ref_g.items():
            if n.endswith("self.key.bias"):   # analytically zero: rounding noise only
                continue
            e = rel_err(res[key][1][n], g0) if g0.abs().max() > 0 else float(res[key][1][n].abs().max())
            if e > worst[1]:
                worst = (n, e)
        print(tag, key, "vs direct: worst gradient difference", worst)
        assert worst[1] < 2e-3, (key, worst)


def _step_pass_events(b, task, staged):
    """What test_step_pass_order expects of one training step: the caption's text pass of encode_batch, then the ITM triplets (3 b rows, each after
    the projection of its [own | hard negative] K/V memory) and the captioning passes (b rows, labels) - in task order in the direct form, per
    condition set in the staged one.  Every pass asks for its dropout seed as it starts."""
    text, seed = ("bert", b, "text", False), ("seed",)
    itm = [("kv", True), ("bert", 3 * b, "cross_kv", False), seed]
    cap_shared, cap_own = [("bert", b, "cross_kv", True), seed], [("bert", b, "cond", True), seed]
    return [text, seed] + {
        # direct: tva triplet, tv triplet, the captioning pass reads tva's memory; staged: set "va" (triplet + captioning), then set "v"
        ("ret%tva%tv_cap%tva", False): itm + itm + cap_shared,
        ("ret%tva%tv_cap%tva", True): itm + cap_shared + itm,
        # direct: the captioning passes come first and project their own K/V; staged: set "va" (cap%tva reads the triplet's memory), then "v"
        ("cap%tv%tva_ret%tva", False): cap_own + cap_own + itm,
        ("cap%tv%tva_ret%tva", True): itm + cap_shared + cap_own,
        # no triplet at all: the captioning pass projects its own K/V in both forms
        ("itc%tv_cap%tv", False): cap_own,
        ("itc%tv_cap%tv", True): cap_own,
    }[(task, staged)]


def test_step_pass_order(setup, cuda):
    """The order of the BERT passes of a training step, which of them read a shared cross-attention K/V memory and which project their own
    condition tokens, and the order in which they draw their dropout seeds - direct and staged form, as literal lists."""
    vtype, tag, m, sd = setup
    if tag != "b16_d2":
        pytest.skip("tower independent")
    fx = golden(f"loss_{tag}.pt")
    r = fx["W1"]
    b = fx["meta"]["b"]
    batch0 = to_dev(synth_inputs(dict(b=b, vision=2, audio=1, S=12), seed=1234), cuda)
    me = m.multimodal_encoder
    bert = me.bert
    events, labelled, seeds = [], [False], iter(range(1, 1 << 20))
    bert_forward, project, lm_forward = bert.forward, bert.project_cross_kv, me.forward

    def rec_lm(*a, **kw):
        labelled[0] = kw.get("labels") is not None
        try:
            return lm_forward(*a, **kw)
        finally:
            labelled[0] = False

    def rec_bert(input_ids=None, attention_mask=None, encoder_hidden_states=None, **kw):
        mode = "cross_kv" if kw.get("cross_kv") is not None else "cond" if encoder_hidden_states is not None else "text"
        events.append(("bert", input_ids.shape[0], mode, labelled[0]))
        return bert_forward(input_ids, attention_mask, encoder_hidden_states, **kw)

    def rec_kv(cond_own, cond_neg=None):
        events.append(("kv", cond_neg is not None))
        return project(cond_own, cond_neg)

    def rec_seed():
        events.append(("seed",))
        return next(seeds)

    was_training = m.training
    me.forward, bert.forward, bert.project_cross_kv, bert.dropout_seed_source = rec_lm, rec_bert, rec_kv, rec_seed
    m.train()
    try:
        for task in ("ret%tva%tv_cap%tva", "cap%tv%tva_ret%tva", "itc%tv_cap%tv"):
            for scale in (None, 1.0):
                batch = dict(batch0)
                batch["_injected"] = {st: {k: r["inj"][st][k] for k in ("neg_cond_idx", "neg_text_idx")} for st in ("tva", "tv")}
                batch["_injected"]["cap"] = r["inj"]["cap"]
                del events[:]
                with runtime.precision(torch.float16):
                    m.zero_grad(set_to_none=True)
                    m(batch, task, compute_loss=True, backward_scale=scale)
                print(task, "staged" if scale else "direct", events)
                assert events == _step_pass_events(b, task, scale is not None), (task, scale)
    finally:
        del me.forward, bert.forward, bert.project_cross_kv
        bert.dropout_seed_source = None
        m.train(was_training)
        m.zero_grad(set_to_none=True)


def test_dkv_session_both_reader_orders(setup, cuda):
    """functional.DkvSession at the BertModel level, in BOTH orders of arrival: a triplet pass [own | neg | own] and an own-only pass read one shared
    K/V memory (BertModel.project_cross_kv); whichever is created last is differentiated first and writes the own set's gradient buffer, the other adds to
    it - the triplet in three short-query launches (own / negative / own), the own-only pass with dkv_accumulate in its one launch, into the own half of
    the triplet's [own | neg] pair.  Against a buffer per pass summed by autograd (dkv_inplace off): same parameter and condition-token gradients."""
    vtype, tag, m, sd = setup
    if tag != "b16_d2":
        pytest.skip("tower independent")
    from mico_amd import functional as Fn
    bert = m.multimodal_encoder.bert
    g = torch.Generator().manual_seed(7)
    n, S, E = 3, 16, 40
    ids = torch.randint(1000, 30000, (3 * n, S), generator=g).to(cuda)
    ids[:, 0] = 101
    am = torch.ones_like(ids)
    cond0, neg0 = torch.randn((n, E, 768), generator=g).to(cuda), torch.randn((n, E, 768), generator=g).to(cuda)
    wt = torch.randn((3 * n, S, 768), generator=g).to(cuda)        # a fixed cotangent per output element
    was_training = bert.training
    bert.eval()                                                    # (no dropout: the two runs of an order must see the same function)
    res = {}
    try:
        for order in ("triplet_first", "own_first"):
            for inplace in (False, True):
                old = runtime.CFG.dkv_inplace
                runtime.CFG.dkv_inplace = inplace
                a0 = Fn.DkvSession.accumulated
                try:
                    with runtime.precision(torch.float16):
                        m.zero_grad(set_to_none=True)
                        cond, neg = cond0.clone().requires_grad_(True), neg0.clone().requires_grad_(True)
                        kv = bert.project_cross_kv(cond, neg)
                        passes = {"triplet": lambda: (bert(input_ids=ids, attention_mask=am, cross_kv=kv).last_hidden_state * wt).sum(),
                                  "own": lambda: (bert(input_ids=ids[:n], attention_mask=am[:n], cross_kv=(kv[0], None)).last_hidden_state * wt[:n]).sum() * 0.5}
                        terms = [passes[k]() for k in (("triplet", "own") if order == "triplet_first" else ("own", "triplet"))]
                        sum(terms).backward()
                finally:
                    runtime.CFG.dkv_inplace = old
                assert Fn.DkvSession.accumulated - a0 == (1 if inplace else 0), (order, inplace)
                grads = {k: p.grad.clone() for k, p in bert.named_parameters() if p.grad is not None}
                grads["cond"], grads["neg"] = cond.grad.clone(), neg.grad.clone()
                res[(order, inplace)] = grads
            ref, got = res[(order, False)], res[(order, True)]
            assert set(ref) == set(got) and any("crossattention.self.value.weight" in k for k in got)
            worst = ("", 0.0)
            for k, g0 in ref.items():
                if k.endswith("self.key.bias"):       # analytically zero: rounding noise only
                    continue
                e = rel_err(got[k], g0) if g0.abs().max() > 0 else float(got[k].abs().max())
                if e > worst[1]:
                    worst = (k, e)
            print("DkvSession", order, "vs a buffer per pass: worst gradient difference", worst)
            assert worst[1] < 2e-3, (order, worst)
    finally:
        bert.train(was_training)


def test_cap_subtask_without_retrieval_twin_keeps_cross_kv_gradients(setup, cuda):
    """task "cap%tv%tva_ret%tva" - cap%tv has no retrieval twin, so its BERT pass projects its own condition tokens and produces
    cross-attention key / value weight gradients itself, while ret%tva / cap%tva go through functional.CrossKVFn, a second producer of the same
    gradients.  With those parameters as part of the shared gradient arena the engine's out-of-place sum dropped later in-place additions; they
    are private in such a pass now.  Against the step with share_grad_arena off (per-node arenas, autograd sums everything): same gradients."""
    vtype, tag, m, sd = setup
    fx = golden(f"loss_{tag}.pt")
    r = fx["W1"]
    b = fx["meta"]["b"]
    batch0 = to_dev(synth_inputs(dict(b=b, vision=2, audio=1, S=12), seed=1234), cuda)
    res = {}
    for task in ("cap%tv%tva_ret%tva", "ret%tva_cap%tva%tv"):
        for share in (False, True):
            batch = dict(batch0)
            batch["_injected"] = {st: {k: r["inj"][st][k] for k in ("neg_cond_idx", "neg_text_idx")} for st in ("tva", "tv")}
            batch["_injected"]["cap"] = r["inj"]["cap"]
            old = runtime.CFG.share_grad_arena
            runtime.CFG.share_grad_arena = share
            try:
                with runtime.precision(torch.float16):
                    m.zero_grad(set_to_none=True)
                    out = m(batch, task, compute_loss=True)
                    sum(out.values()).backward()
            finally:
                runtime.CFG.share_grad_arena = old
            res[share] = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        assert set(res[True]) == set(res[False])
        worst = ("", 0.0)
        for n, g0 in res[False].items():
            if n.endswith("self.key.bias"):
                continue
            e = rel_err(res[True][n], g0) if g0.abs().max() > 0 else float(res[True][n].abs().max())
            if e > worst[1]:
                worst = (n, e)
        print(tag, task, "shared arena vs per-node arenas: worst gradient difference", worst)
        assert worst[1] < 2e-3, (task, worst)      # (summation order of fp32 atomics / split-K slabs only)


def test_no_cpu_fallback():
    """The product path must fail loudly on CPU tensors - it never routes through PyTorch/oracle math."""
    from mico_amd._lib import MicoHipError
    m, _ = build_model("evaclip02_base", 1, device="cpu")
    with pytest.raises((MicoHipError, RuntimeError)):
        m.forward_vision_encoder(torch.zeros(1, 1, 3, 224, 224))


def test_full_depth_vit_g(cuda):
    """Full 40-block EVA01-g/14 on one image against the reference's own output (tests/golden/vit_g14_full.pt): the parity configuration,
    bench.py's timed precision (both at the 1e-3 gate, token rows AND feat_v) and bf16 (reported bound)."""
    fx = golden("vit_g14_full.pt")
    m, sd = build_model("evaclip01_giant", None, device=cuda)
    g = torch.Generator().manual_seed(fx["meta"]["input_seed"])
    x = torch.randn((1, 1, 3, 224, 224), generator=g).to(cuda)
    from mico_amd.functional import l2_normalize
    import contextlib
    er = Errs("full g/14")
    for name, ctx, tol in (("parity", precision_config("parity"), 1e-3), ("timed", precision_config("timed"), 1e-3),
                           ("bf16", runtime.precision(torch.bfloat16), 2e-2)):
        with ctx, torch.no_grad():
            out = m.forward_vision_encoder(x)
            feat = l2_normalize(m.contra_head_v(m.pool_vision_for_contra(out)))
        er.add(f"{name} token rows", err_vs(out[0, 0, [0, 1, 128, 256]], fx["rows"], fx["amax"]), tol)
        er.add(f"{name} feat_v", rel_err(feat, fx["feat_v"]), tol)
    er.check()


def test_subtitle_branch_and_heads(cuda):
    """get_multimodal_forward_input_subtitle (16-bit MFMA projection: the 1e-3 gate in the fp16 parity configuration) and the
    subtitle-bearing contrastive heads (exact-fp32 kernels) against the reference (golden subtitle_b16.pt)."""
    fx = golden("subtitle_b16.pt")
    m, _ = build_model("evaclip02_base", 1, device=cuda)
    with runtime.precision(torch.float16), torch.no_grad():
        cond = m.get_multimodal_forward_input_subtitle(fx["sub_in"].to(cuda))
        assert cond.shape == fx["cond_s"].shape and rel_err(cond, fx["cond_s"]) < 1e-3
        for k, x in fx["pooled"].items():
            y = getattr(m, "contra_head_" + k)(x.to(cuda))
            assert rel_err(y, fx["head_" + k]) < 1e-5, k


def test_subtitle_subtasks(cuda):
    """vast.py's subtitle sub-tasks (ts / tvs / tvas): subtitles through the text BERT, CLS-pooled for the contrastive heads
    (contra_head_s / _vs / _vas) and projected + type-embedded as cross-attention condition tokens, concatenated after the vision
    and audio tokens.  Features and the ITC / ITM / CAP losses against the oracle (fp16 parity configuration)."""
    import random
    torch.set_num_threads(16)
    m, sd = build_model("evaclip02_base", 2, device=cuda)
    sdo = dict(sd)
    sdo["multimodal_encoder.cls.predictions.decoder.weight"] = sdo["multimodal_encoder.bert.embeddings.word_embeddings.weight"]
    b = 3
    inp = synth_inputs(dict(b=b, vision=2, audio=1, S=10), seed=21)
    sub = synth_inputs(dict(b=b, S=7), seed=22)
    inp["subtitle_ids"], inp["subtitle_mask"] = sub["input_ids"], sub["attention_mask"]
    idx = torch.arange(b).roll(1)
    mi, lab = O.token_masker(inp["input_ids"], 0.6, random.Random(1))
    task = "ret%tvas%tvs%ts_cap%tvas"
    inj = {st: dict(neg_cond_idx=idx, neg_text_idx=idx.roll(1)) for st in ("tvas", "tvs", "ts")}
    inj["cap"] = dict(masked_ids=mi, labels=lab)
    with torch.no_grad():
        ref, ref_enc = O.mico_forward(sdo, O.ARCHS["evaclip02_base"], inp, task, dict(itm_ratio=0.1), injected=inj)
    batch = to_dev(inp, cuda)
    batch["_injected"] = inj
    with runtime.precision(torch.float16), torch.no_grad():
        enc = m.encode_batch(dict(batch))
        for c in ("s", "vs", "vas"):
            assert rel_err(m._feat_cond(enc, c), O.feat_cond(sdo, ref_enc, c)) < 1e-3, c
            assert rel_err(m._condition_feats(enc, c), O.condition_feats(ref_enc, c)) < 1e-3, c
        out = m(batch, task)
    for k, v in ref.items():
        e = abs(out[k].item() - v.item()) / max(abs(v.item()), 1e-6)
        assert e < 1e-3, (k, out[k].item(), v.item())
    # raw subtitles are tokenised to max_subtitle_len
    raw = dict(to_dev(synth_inputs(dict(b=2, vision=1, S=10), seed=5), cuda), raw_subtitles=["a dog barks", "people talking loudly"])
    with runtime.precision(torch.float16), torch.no_grad():
        e2 = m.encode_batch(raw)
    assert e2["condition_feats_s"].shape == (2, m.max_subtitle_len, 768)


def test_fp8_tower_tolerance(cuda):
    """BASELINE configs[4] precision ("fp8 MFMA"): the towers' forward and input-gradient GEMMs on the block-scaled fp8 MFMA
    (runtime.fp8_mode).  The reference has no fp8 path - the bound is this build's, measured against the same reference goldens as the
    16-bit configurations: final-LN tokens of the depth-2 towers within 6e-2 of max|ref| (measured 1.5-3e-2; e4m3 carries 3 mantissa
    bits: ~3 % per product, averaged over the reduction), gradient digests within 0.2.  Also: the fp8 kernels actually ran."""
    from mico_amd import ops
    for vtype, tag in (("evaclip02_base", "b16_d2"), ("evaclip01_giant", "g14_d2")):
        m, sd = build_model(vtype, 2, device=cuda)
        fx = golden(f"vit_{tag}.pt")
        g = torch.Generator().manual_seed(fx["meta"]["input_seed"])
        x = torch.randn((2, 3, 224, 224), generator=g)
        w = torch.randn(fx["out"].shape, generator=g) / fx["out"].numel() ** 0.5
        calls = []
        orig = ops.gemm_mx8
        ops.gemm_mx8 = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        try:
            import mico_amd.functional as Fm
            Fm._mx8_worthwhile, keep = (lambda mm, nn: True), Fm._mx8_worthwhile     # 2 images are a small problem: force the fp8 path
            with runtime.precision(torch.bfloat16), runtime.fp8_mode():
                m.zero_grad(set_to_none=True)
                out = m.vision_encoder.visual(x.to(cuda), return_all_features=True)
                e = rel_err(out, fx["out"])
                (out * w.to(cuda)).sum().backward()
        finally:
            ops.gemm_mx8 = orig
            Fm._mx8_worthwhile = keep
        named = dict(m.vision_encoder.visual.named_parameters())
        worst = max(grad_digest_check(d, named[n].grad, None) for n, d in fx["grads"].items())
        print(f"{tag} fp8: fwd rel err {e:.2e}, worst grad digest err {worst:.2e}, {len(calls)} fp8 GEMM launches")
        assert len(calls) >= 2 * 4 * 2 - 2      # 4 forward + 4 input-gradient GEMMs per block (B/16 has more), 2 blocks
        assert e < 0.15 and worst < 0.35
