"""Shared by tests/test_clip_cpu.py and tests/test_clip_gpu.py: the oracle of a clipped optimizer step on the CPU - torch.nn.utils.clip_grad_norm_
on float64 gradients, then the reference AdamW's arithmetic (data/utils/build_optimizer.py:105-197) restated in float64.  The restatement is
checked against the reference's own outputs (tests/golden/optimizer.pt) in test_clip_cpu.py."""
import math

import torch
import torch.nn as nn

GROUP_HYPER = [dict(weight_decay=0.01, lr=1e-3), dict(weight_decay=0.0, lr=5e-4)]      # the groups optimizer.pt was recorded with
BETAS, EPS = (0.9, 0.98), 1e-6
NORM_GATE = 1e-5       # relative gate of the norm (all terms >= 0: summation chain length x 2^-24 on the sum, half of it on the root)


class OracleAdamW:
    """float64 state of the reference update over [group][param] tensors; step(grads) takes None for a parameter without a gradient."""

    def __init__(self, init, correct_bias):
        self.p = [[t.double().clone() for t in grp] for grp in init]
        self.m = [[torch.zeros_like(t) for t in grp] for grp in self.p]
        self.v = [[torch.zeros_like(t) for t in grp] for grp in self.p]
        self.t = [[0 for _ in grp] for grp in self.p]
        self.correct_bias = correct_bias

    def step(self, grads, max_grad_norm=None):
        """grads [group][param] (float64 or None) -> (total_norm, coef) of torch's clip_grad_norm_ (None, 1.0 without clipping)"""
        norm, coef = None, 1.0
        if max_grad_norm is not None:
            holders = [nn.Parameter(torch.zeros_like(g, dtype=torch.float64)) for grp in grads for g in grp if g is not None]
            for h, g in zip(holders, [g for grp in grads for g in grp if g is not None]):
                h.grad = g.double().clone()
            norm = float(torch.nn.utils.clip_grad_norm_(holders, max_grad_norm, norm_type=2.0))
            it = iter(holders)
            grads = [[None if g is None else next(it).grad for g in grp] for grp in grads]
            coef = min(1.0, max_grad_norm / (norm + 1e-6))
        b1, b2 = BETAS
        for gi, grp in enumerate(grads):
            lr, wd = GROUP_HYPER[gi]["lr"], GROUP_HYPER[gi]["weight_decay"]
            for pi, g in enumerate(grp):
                if g is None:
                    continue
                g = g.double()
                self.t[gi][pi] += 1
                t = self.t[gi][pi]
                self.m[gi][pi] = self.m[gi][pi] * b1 + (1.0 - b1) * g
                self.v[gi][pi] = self.v[gi][pi] * b2 + (1.0 - b2) * g * g
                step_size = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t) if self.correct_bias else lr
                p = self.p[gi][pi] - step_size * (self.m[gi][pi] / (self.v[gi][pi].sqrt() + EPS))
                if wd > 0.0:
                    p = p - lr * wd * p
                self.p[gi][pi] = p
        return norm, coef


def fixture_grads(fx, step):
    """the gradients of optimizer.pt's step `step` as the fixture applied them: parameter [0][1] has none at step 1"""
    return [[None if (step == 1 and gi == 0 and pi == 1) else g for pi, g in enumerate(grp)] for gi, grp in enumerate(fx["grads"][step])]
