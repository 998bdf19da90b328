"""Global-norm gradient clipping, host side (no GPU): the C-ABI of its four entry points, build_optimizer's key, GradScaler's single
read-only pass over a stub optimizer, argument errors raised before any library call, and the float64 oracle the GPU tests use."""
import os
import re
import types

import pytest
import torch
import torch.nn as nn

from clip_common import OracleAdamW, fixture_grads
from common import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mico_grad_sumsq": 10, "mico_grad_clip_coef": 6, "mico_adamw_step_dev": 15, "mico_grads_scale": 8}


def test_abi_of_the_clip_entry_points():
    import ctypes
    from mico_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mico_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW.items():
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, hdr, re.S)
        assert decl, f"{name} is not declared in include/mico_hip.h"
        assert len(decl.group(1).split(",")) == nargs, name
        assert len(_lib.PROTOTYPES[name]) == nargs, name
        assert hasattr(raw, name), f"{name} is not exported"
    # mico_adamw_step_dev = mico_adamw_step + one trailing device pointer before the stream; mico_adamw_step itself is unchanged
    assert _lib.PROTOTYPES["mico_adamw_step_dev"] == _lib.PROTOTYPES["mico_adamw_step"][:-1] + [_lib.c_vp, _lib.c_vp]
    assert len(_lib.PROTOTYPES["mico_adamw_step"]) == 14
    assert _lib.lib().mico_version() == _lib.ABI_VERSION >= 120


def _args(**run):
    from mico_amd.model import AttrDict
    return AttrDict(model_cfg=AttrDict(vision_encoder_type="evaclip01_giant"),
                    run_cfg=AttrDict(new_params_name=["fresh"], weight_decay=0.01, learning_rate=1e-4, new_lr=5e-4, clip_lr=5e-7,
                                     betas=[0.9, 0.98], optim="adamw", **run))


def test_build_optimizer_reads_max_grad_norm_only():
    from mico_amd import optim
    tiny = nn.Sequential(nn.Linear(3, 2), nn.LayerNorm(2))
    plain = optim.build_optimizer(tiny, _args(), None)
    assert plain.max_grad_norm is None and plain.last_grad_norm is None
    assert optim.build_optimizer(tiny, _args(max_grad_norm=None), None).max_grad_norm is None
    assert optim.build_optimizer(tiny, _args(max_grad_norm=-1), None).max_grad_norm is None
    assert optim.build_optimizer(tiny, _args(grad_norm=5.0), None).max_grad_norm is None      # the reference's ignored default stays ignored
    clipped = optim.build_optimizer(tiny, _args(max_grad_norm=2.5), None)
    assert clipped.max_grad_norm == 2.5
    a, b = plain.state_dict(), clipped.state_dict()
    assert set(a) == set(b) == {"state", "param_groups"}
    assert [sorted(g) for g in a["param_groups"]] == [sorted(g) for g in b["param_groups"]]
    assert not any("max_grad_norm" in g for g in b["param_groups"]) and "max_grad_norm" not in clipped.defaults
    with pytest.raises(ValueError):
        optim.build_optimizer(tiny, _args(max_grad_norm=0.0), None)


class _StubOptimizer:
    """records what GradScaler.step asks of an optimizer; `bad` is what the overflow check finds"""

    def __init__(self, max_grad_norm, bad):
        self.param_groups = [dict(params=[nn.Parameter(torch.zeros(2))])]
        self.max_grad_norm, self.bad, self.calls = max_grad_norm, bad, []

    def grads_nonfinite(self, flag):
        self.calls.append(("grads_nonfinite",))
        flag.fill_(float(self.bad))
        return flag

    def grad_clip_stats(self, max_grad_norm, grad_mult=1.0, flag=None):
        self.calls.append(("grad_clip_stats", max_grad_norm, grad_mult))
        assert flag is not None, "the scaler's overflow flag must ride on the same pass"
        flag.fill_(float(self.bad))
        return "coef"

    def step(self, **kw):
        self.calls.append(("step", kw))
        return "stepped"


def test_grad_scaler_uses_one_pass_when_the_optimizer_clips():
    from mico_amd.optim import GradScaler
    sc = GradScaler(init_scale=8.0)
    opt = _StubOptimizer(2.0, bad=False)
    assert sc.step(opt) == "stepped"
    sc.update()
    assert opt.calls == [("grad_clip_stats", 2.0, 1.0 / 8.0), ("step", dict(grad_mult=1.0 / 8.0, clip_coef="coef"))]
    assert sc.get_scale() == 8.0
    # found inf: the step is skipped and the scale halves, as without clipping
    opt = _StubOptimizer(2.0, bad=True)
    assert sc.step(opt) is None
    sc.update()
    assert opt.calls == [("grad_clip_stats", 2.0, 1.0 / 8.0)] and sc.get_scale() == 4.0
    # clipping off: the parent's calls exactly
    opt = _StubOptimizer(None, bad=False)
    assert sc.step(opt) == "stepped"
    sc.update()
    assert opt.calls == [("grads_nonfinite",), ("step", dict(grad_mult=1.0 / 4.0))]
    opt = _StubOptimizer(None, bad=True)
    assert sc.step(opt) is None
    sc.update()
    assert opt.calls == [("grads_nonfinite",)] and sc.get_scale() == 2.0
    # per-call override of the attribute
    opt = _StubOptimizer(None, bad=False)
    sc.step(opt, max_grad_norm=3.0)
    assert [c[0] for c in opt.calls] == ["grad_clip_stats", "step"] and opt.calls[0][1] == 3.0


def test_bad_arguments_raise_before_any_library_call(monkeypatch):
    from mico_amd import _lib, optim

    def reached():
        pytest.fail("the library was reached before the argument check")
    monkeypatch.setattr(_lib, "lib", reached)
    p = nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    for bad in (0, -2):
        with pytest.raises(ValueError):
            optim.AdamW([p], max_grad_norm=bad)
        opt = optim.AdamW([p])
        with pytest.raises(ValueError):
            opt.step(max_grad_norm=bad)
        opt.max_grad_norm = bad
        with pytest.raises(ValueError):
            opt.step()
        with pytest.raises(ValueError):
            optim.GradScaler().step(opt)
        with pytest.raises(ValueError):
            optim.clip_grad_norm_([p], bad)
        assert len(opt.state) == 0
    with pytest.raises(ValueError):
        optim.clip_grad_norm_([p], 1.0, norm_type=1)
    with pytest.raises(ValueError):
        optim.clip_grad_norm_([p], 1.0, norm_type=float("inf"))
    assert torch.equal(p.grad, torch.ones(4))


@pytest.mark.parametrize("correct_bias", [True, False])
def test_oracle_restates_the_reference_update(correct_bias):
    """clip_common.OracleAdamW without clipping against the reference optimizer's own outputs: the float64 restatement differs from the
    reference's fp32 run by fp32 rounding only (the gate of tests/test_optim_gpu.py); with clipping, its coefficient is torch's."""
    fx = golden("optimizer.pt")[f"correct_bias_{correct_bias}"]
    o = OracleAdamW(fx["init"], correct_bias)
    for step in range(4):
        assert o.step(fixture_grads(fx, step)) == (None, 1.0)
        for gi, grp in enumerate(fx["after"][step]):
            for pi, want in enumerate(grp):
                assert (o.p[gi][pi].float() - want).abs().max() <= 2e-7 * want.abs().max().clamp_min(1.0), (step, gi, pi)
    for gi, grp in enumerate(fx["moments"]):
        for pi, (m, v, st) in enumerate(grp):
            assert o.t[gi][pi] == st
            assert (o.m[gi][pi].float() - m).abs().max() < 1e-6 * m.abs().max() and (o.v[gi][pi].float() - v).abs().max() < 1e-6 * v.abs().max()
    o = OracleAdamW(fx["init"], correct_bias)
    grads = fixture_grads(fx, 0)
    ref = torch.cat([g.double().flatten() for grp in grads for g in grp]).norm().item()
    norm, coef = o.step(grads, max_grad_norm=0.3 * ref)
    assert abs(norm - ref) <= 1e-12 * ref and abs(coef - 0.3) < 1e-6
