"""Global-norm gradient clipping on the GPU (mico_grad_sumsq, mico_grad_clip_coef, mico_adamw_step_dev, mico_grads_scale behind
mico_amd.optim.AdamW(max_grad_norm=...), GradScaler and clip_grad_norm_) against torch.nn.utils.clip_grad_norm_ and the reference AdamW
arithmetic in float64 on the CPU (clip_common.OracleAdamW).

The norm's gate, |total_norm - ref| <= 1e-5 ref, comes from the kernel's own summation: every term is >= 0, so the relative error of the sum is
at most (longest chain of roundings) x 2^-24; the kernel's chain is 31 (stated at grad_sumsq_kernel), the gate allows 270 x 6e-8 = 1.6e-5 on
the sum, half of that on the root.  The gates of the clipped update add that delta to the ones of tests/test_optim_gpu.py."""
import pytest
import torch
import torch.nn as nn

from clip_common import GROUP_HYPER, BETAS, NORM_GATE, OracleAdamW, fixture_grads
from common import build_model, golden, rel_err

pytestmark = pytest.mark.gpu

CHUNK = 65536
NUMELS = [1, 3, 5, CHUNK, CHUNK + 1, 2 * CHUNK + 7]     # below a vector, ragged, one chunk exactly, one element into a second chunk, 3 chunks + tail
MISALIGNED = 4                                          # this tensor's gradient starts one element into its storage: the scalar path, two chunks


@pytest.fixture(scope="module")
def table():
    """CPU gradients of the shape list (seeded) and their float64 norm; never modified"""
    g = torch.Generator().manual_seed(11)
    grads = [torch.randn(n, generator=g) for n in NUMELS]
    ref = torch.cat([t.double() for t in grads]).norm().item()
    return dict(grads=grads, ref=ref)


def _params(cuda, grads, scale=1.0):
    """parameters with these gradients on the device, in two param groups, plus one parameter without a gradient; the gradient of tensor
    MISALIGNED is a view one element into its storage"""
    params = []
    for i, g in enumerate(grads):
        p = nn.Parameter(torch.zeros(g.numel(), device=cuda))
        if i == MISALIGNED:
            store = torch.empty(g.numel() + 1, device=cuda)
            p.grad = store[1:]
            p.grad.copy_(g * scale)
            assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
        else:
            p.grad = (g * scale).to(cuda)
        params.append(p)
    nograd = nn.Parameter(torch.zeros(9, device=cuda))
    groups = [dict(params=params[:3] + [nograd], weight_decay=0.01, lr=1e-3), dict(params=params[3:], weight_decay=0.0, lr=5e-4)]
    return params, groups


def test_norm_against_float64(cuda, table):
    from mico_amd.optim import AdamW
    params, groups = _params(cuda, table["grads"])
    opt = AdamW(groups, lr=1e-3, max_grad_norm=1.0)
    assert opt.last_grad_norm is None
    coef = opt.grad_clip_stats(1.0)
    norm = opt.last_grad_norm
    assert norm.dtype == torch.float32 and norm.is_cuda and norm.numel() == 1
    got, ref = norm.item(), table["ref"]
    print(f"norm {got!r} ref {ref!r} rel {abs(got - ref) / ref:.3e}")
    assert abs(got - ref) <= NORM_GATE * ref
    want_coef = 1.0 / (ref + 1e-6)
    assert abs(coef.item() - want_coef) <= (NORM_GATE + 2e-7) * want_coef
    coef2 = opt.grad_clip_stats(1.0)                       # fixed summation order, plain stores: the same bits on every run
    assert opt.last_grad_norm.item() == got and coef2.item() == coef.item()
    assert len(opt.state) == 0                             # the read-only pass creates no optimizer state


def test_multiply_comes_before_the_square(cuda, table):
    """fp32 gradients of magnitude 3e20 (a loss-scaled backward) cannot be squared in fp32; times 1 / 2^16 first they can"""
    from mico_amd.optim import AdamW
    params, groups = _params(cuda, table["grads"], scale=3e20)
    opt = AdamW(groups, lr=1e-3, max_grad_norm=1.0)
    flag = torch.zeros(1, device=cuda)
    opt.grad_clip_stats(1.0, grad_mult=2.0 ** -16, flag=flag)
    ref = torch.cat([(t * 3e20).double() * 2.0 ** -16 for t in table["grads"]]).norm().item()
    got = opt.last_grad_norm.item()
    print(f"norm {got!r} ref {ref!r} rel {abs(got - ref) / ref:.3e}")
    assert abs(got - ref) <= NORM_GATE * ref
    assert flag.item() == 0.0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_sets_the_flag_and_skips_the_step(cuda, table, bad):
    from mico_amd.optim import AdamW, GradScaler
    params, groups = _params(cuda, table["grads"])
    opt = AdamW(groups, lr=1e-3, max_grad_norm=1.0)
    sc = GradScaler(init_scale=4.0)
    sc.step(opt)                                           # a clean step first: the moments exist
    sc.update()
    assert all(opt.state[p]["step"] == 1 for p in params) and torch.isfinite(opt.last_grad_norm).item()
    before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
    params[-1].grad[-1] = bad                              # the last element of the ragged tail of the last tensor
    flag = torch.zeros(1, device=cuda)
    opt.grad_clip_stats(1.0, grad_mult=0.25, flag=flag)
    assert flag.item() == 1.0 and not torch.isfinite(opt.last_grad_norm).item()
    opt.last_grad_norm = None
    assert sc.step(opt) is None
    assert opt.last_grad_norm is not None and not torch.isfinite(opt.last_grad_norm).item()     # a skipped step still records its norm
    sc.update()
    assert sc.get_scale() == 2.0
    for p, (p0, m0, v0) in zip(params, before):
        assert opt.state[p]["step"] == 1
        assert torch.equal(p.detach(), p0) and torch.equal(opt.state[p]["exp_avg"], m0) and torch.equal(opt.state[p]["exp_avg_sq"], v0)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_coef_one_is_bit_identical_to_the_unclipped_step(cuda, dt):
    """norm 0 (all-zero gradients) and a max_grad_norm far above the norm both give coef == 1.0f, and grad_mult * 1.0f is grad_mult: parameters,
    moments and the 16-bit weight mirrors (plain bf16, split fp16) equal those of a twin stepped through mico_adamw_step"""
    from mico_amd import runtime
    from mico_amd.optim import AdamW
    g = torch.Generator().manual_seed(3)
    shapes = [(40, 64), (40,), (7,)]
    init = [torch.randn(*s, generator=g) for s in shapes]
    grads = [torch.randn(*s, generator=g) for s in shapes]
    runtime.clear_weight_cache()
    try:
        with runtime.precision(dt):
            twins, mirrors = [], []
            for max_norm in (1e9, None):
                ps = [nn.Parameter(t.clone().to(cuda)) for t in init]
                runtime.gemm_weight([ps[0]])
                assert runtime.weight_mirror(ps[0]) is not None
                mirrors.append(runtime._live_copies(ps[0])[0][1][0])
                opt = AdamW([dict(params=ps[:1], weight_decay=0.01), dict(params=ps[1:], weight_decay=0.0)], lr=1e-2, betas=BETAS,
                            max_grad_norm=max_norm)
                for step in range(2):
                    for p, gr in zip(ps, grads):
                        p.grad = torch.zeros_like(p) if step == 0 else gr.to(cuda) * 512.0
                    opt.step(grad_mult=1.0 / 512.0)
                    if max_norm is not None:
                        coef = opt.grad_clip_stats(max_norm, grad_mult=1.0 / 512.0)
                        assert coef.item() == 1.0 and (opt.last_grad_norm.item() == 0.0) == (step == 0)
                assert runtime._live_copies(ps[0])[0][1][0] is mirrors[-1]          # the cached copy survived both steps
                twins.append((ps, opt))
            (pa, oa), (pb, ob) = twins
            for a, b in zip(pa, pb):
                assert torch.equal(a.detach(), b.detach())
                assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) and torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
            assert torch.equal(mirrors[0], mirrors[1])
            w = pa[0].detach()
            hi = w.to(dt)
            assert torch.equal(mirrors[0][:40, :64], hi) and not torch.equal(w.cpu(), init[0])
            if dt == torch.float16:
                assert getattr(mirrors[0], "_mico_split", False)
                assert torch.equal(mirrors[0][:40, 64:128], (w - hi.float()).to(dt))
    finally:
        runtime.clear_weight_cache()


@pytest.mark.parametrize("through_scaler", [False, True])
@pytest.mark.parametrize("correct_bias", [True, False])
def test_clipped_update_matches_the_oracle(cuda, correct_bias, through_scaler):
    """optimizer.pt's initial values and gradients, 4 steps, parameter [0][1] skipping step 1, max_grad_norm 3.2 (coef ~ 0.3): torch's
    clip_grad_norm_ in float64, then the reference update; directly and through GradScaler(init_scale=1024) with scaled gradients."""
    from mico_amd.optim import AdamW, GradScaler
    fx = golden("optimizer.pt")[f"correct_bias_{correct_bias}"]
    max_norm, d = 3.2, NORM_GATE
    params = [[nn.Parameter(t.clone().to(cuda)) for t in grp] for grp in fx["init"]]
    opt = AdamW([dict(params=params[gi], **GROUP_HYPER[gi]) for gi in range(2)], lr=1e-3, betas=BETAS, correct_bias=correct_bias,
                max_grad_norm=max_norm)
    sc = GradScaler(init_scale=1024.0)
    oracle = OracleAdamW(fx["init"], correct_bias)
    for step in range(4):
        gs = fixture_grads(fx, step)
        for gi, grp in enumerate(params):
            for pi, p in enumerate(grp):
                g = gs[gi][pi]
                p.grad = None if g is None else (g * 1024.0 if through_scaler else g.clone()).to(cuda)
        before = [[t.clone() for t in grp] for grp in oracle.p]
        norm, coef = oracle.step(gs, max_grad_norm=max_norm)
        assert 0.25 < coef < 0.4
        if through_scaler:
            sc.step(opt)
            sc.update()
        else:
            opt.step()
        got_norm = opt.last_grad_norm.item()               # of the UN-scaled gradients
        print(f"step {step} norm {got_norm!r} ref {norm!r} rel {abs(got_norm - norm) / norm:.3e}")
        assert abs(got_norm - norm) <= d * norm
        for gi, grp in enumerate(params):
            for pi, p in enumerate(grp):
                want = oracle.p[gi][pi]
                tol = 2e-7 * max(1.0, want.abs().max().item()) + 2 * d * (want - before[gi][pi]).abs().max().item()
                err = (p.detach().cpu().double() - want).abs().max().item()
                assert err <= tol, (step, gi, pi, err, tol)
    for gi, grp in enumerate(params):
        for pi, p in enumerate(grp):
            s = opt.state[p]
            assert s["step"] == oracle.t[gi][pi]
            assert rel_err(s["exp_avg"], oracle.m[gi][pi]) < 1e-6 + 2 * d and rel_err(s["exp_avg_sq"], oracle.v[gi][pi]) < 1e-6 + 3 * d
    assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert all("max_grad_norm" not in g for g in opt.state_dict()["param_groups"])


def test_weight_mirrors_refreshed_in_a_clipped_step(cuda):
    """tests/test_optim_gpu.py::test_weight_mirrors_refreshed_in_step with a step that clips: after it the cached 16-bit weights equal a fresh
    cast of the updated parameters, in the bf16 and the split fp16 layouts (mico_adamw_step_dev runs the kernel that refreshes them)."""
    from mico_amd import runtime
    from mico_amd.optim import AdamW
    from mico_amd.weights import synth_inputs
    max_norm = 0.01
    for dt in (torch.bfloat16, torch.float16):
        runtime.clear_weight_cache()
        m, sd = build_model("evaclip02_base", 1, device=cuda)
        m.train()
        opt = AdamW([dict(params=[p for p in m.parameters()], weight_decay=0.01, lr=1e-2)], lr=1e-2, max_grad_norm=max_norm)
        batch = {k: v.to(cuda) for k, v in synth_inputs(dict(b=2, vision=1, audio=1, S=8), seed=5).items()}
        with runtime.precision(dt):
            loss = sum(m(dict(batch), "ret%tva_cap%tva").values())
            loss.backward()
            before = {k: v[1].clone() for k, v in runtime._W16.items()}
            opt.step()
            assert opt.last_grad_norm.item() > 2 * max_norm, "the step must clip"
            kept = dict(runtime._W16)
            assert len(kept) > 20, "most weight copies must survive the step through their mirrors"
            changed = 0
            for key, (_, buf) in kept.items():
                src = runtime._ENTRY_SRC[key]
                plist = [p for p in m.parameters() if runtime.param_uid(p) in src]
                plist.sort(key=lambda p: src.index(runtime.param_uid(p)))
                w = torch.cat([p.detach().reshape(p.shape[0], -1) for p in plist], 0)
                n, k = w.shape
                kp = buf.shape[1] // 2 if getattr(buf, "_mico_split", False) else buf.shape[1]
                hi = w.to(dt)
                assert torch.equal(buf[:n, :k], hi), key
                if getattr(buf, "_mico_split", False):
                    assert torch.equal(buf[:n, kp:kp + k], (w - hi.float()).to(dt)), key
                changed += int(not torch.equal(buf, before[key]))
            assert changed > 20
    runtime.clear_weight_cache()


def _within_one_ulp(got, want):
    lo = torch.nextafter(want, torch.full_like(want, float("-inf")))
    hi = torch.nextafter(want, torch.full_like(want, float("inf")))
    return bool(((got >= lo) & (got <= hi)).all())


def test_clip_grad_norm_drop_in(cuda, table):
    from mico_amd.optim import clip_grad_norm_
    ref = table["ref"]
    params, _ = _params(cuda, table["grads"])
    max_norm = 0.5 * ref
    total = clip_grad_norm_(params, max_norm)
    assert total.dtype == torch.float32 and total.is_cuda
    print(f"norm {total.item()!r} ref {ref!r} rel {abs(total.item() - ref) / ref:.3e}")
    assert abs(total.item() - ref) <= NORM_GATE * ref
    coef = torch.tensor(max_norm, dtype=torch.float32) / (total.cpu() + 1e-6)          # the coefficient's fp32 arithmetic, from the returned norm
    assert abs(coef.item() - 0.5) < 1e-5
    for p, g in zip(params, table["grads"]):
        assert _within_one_ulp(p.grad.cpu(), g * coef), p.numel()
    # a norm below max_norm: nothing is rewritten (also through a single tensor argument)
    params, _ = _params(cuda, table["grads"])
    total = clip_grad_norm_(params, 2.0 * ref)
    assert abs(total.item() - ref) <= NORM_GATE * ref
    for p, g in zip(params, table["grads"]):
        assert torch.equal(p.grad.cpu(), g)
    assert clip_grad_norm_(params[-1], 1e9).item() > 0 and torch.equal(params[-1].grad.cpu(), table["grads"][-1])
    assert float(clip_grad_norm_([nn.Parameter(torch.zeros(3, device=cuda))], 1.0)) == 0.0      # no gradients at all


def test_clip_grad_norm_counts_gradients_torch_scales(cuda):
    """an fp16 gradient and a non-contiguous fp32 gradient are scaled by torch (glue), but their squares count in the norm"""
    from mico_amd.optim import clip_grad_norm_
    g = torch.Generator().manual_seed(5)
    a, b, c = torch.randn(300, generator=g), torch.randn(8, 6, generator=g), torch.randn(50, generator=g).half()
    pa, pb, pc = nn.Parameter(torch.zeros(300, device=cuda)), nn.Parameter(torch.zeros(6, 8, device=cuda)), \
        nn.Parameter(torch.zeros(50, device=cuda, dtype=torch.float16))
    pa.grad, pb.grad, pc.grad = a.to(cuda), b.to(cuda).t(), c.to(cuda)
    assert not pb.grad.is_contiguous()
    ref = torch.cat([a.double(), b.double().flatten(), c.double()]).norm().item()
    total = clip_grad_norm_([pa, pb, pc], 0.25 * ref)
    assert abs(total.item() - ref) <= NORM_GATE * ref
    coef = torch.tensor(0.25 * ref, dtype=torch.float32) / (total.cpu() + 1e-6)
    assert _within_one_ulp(pa.grad.cpu(), a * coef) and _within_one_ulp(pb.grad.cpu(), b.t() * coef)
    assert torch.equal(pc.grad.cpu(), c * coef.half())
