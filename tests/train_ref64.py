"""Float64 restatement of torch.optim.Adam's single-tensor step (torch/optim/adam.py
_single_tensor_adam, the non-capturable path the reference's optimizer takes), with a learning rate
and a step count per element, and the error bounds an fp32 Adam is held to against it.

Test infrastructure only (not collected: no test_ prefix). The inputs are the fp32 values of one
step (parameters, gradient, exp_avg, exp_avg_sq before the step) promoted to float64; the outputs are
what that one step gives in float64. A sequence of steps is checked one step at a time, each from the
fp32 state the code under test itself held before it, so no rounding is carried from step to step.

Bounds (tests/test_train_ref64.py checks that the fp32 numpy oracle oracle/train_oracle.adam_step
stays inside them on the inputs of tests/_train_cases.py; csrc/optim.hip is held to the same ones):

  exp_avg_sq  |v - v64| <= V_REL * v64                       no absolute term: every term is
                                                             non-negative, at most four roundings
                                                             (beta2, 1 - beta2, g * g, the sum)
  exp_avg     |m - m64| <= M_REL * max(|g|, |m_prev|)        the lerp m + w (g - m) cancels
  param       |p - p64| <= P_ULPS * ulp32(p64) + P_STEP * |p64 - p_prev|
                                                             one rounding of p and a relative error
                                                             of the step

Measured worst ratios error / bound of the oracle against this reference, over the 14-group layout
at P in {1, 3, 37}, three steps each (tests/test_train_ref64.py::test_oracle_adam_within_bounds
prints them): exp_avg_sq 0.174, exp_avg 0.058, param 0.249 (P = 37; P = 1 and 3 are within 0.06 of
these). The oracle breaks none of the bounds, so they stand as first written.
"""
from __future__ import annotations

import numpy as np

V_REL = 1e-6
M_REL = 1e-6
P_ULPS = 2.0
P_STEP = 1e-5


def adam64(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-15):
    """One Adam step in float64. p, g, m, v: arrays of one shape; lr and step: scalars or arrays
    that broadcast to it. Elements whose step count is <= 0 have no gradient this step (torch skips
    a parameter whose .grad is None): their p, m and v come back untouched."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    lr = np.broadcast_to(np.asarray(lr, np.float64), p.shape)
    step = np.broadcast_to(np.asarray(step, np.int64), p.shape)
    live = step > 0
    t = np.where(live, step, 1).astype(np.float64)
    m1 = m + (g - m) * (1.0 - beta1)                           # exp_avg.lerp_(grad, 1 - beta1)
    v1 = v * beta2 + (1.0 - beta2) * g * g                     # mul_(beta2).addcmul_(g, g, 1 - beta2)
    step_size = lr / (1.0 - beta1 ** t)
    denom = np.sqrt(v1) / np.sqrt(1.0 - beta2 ** t) + eps
    p1 = p - step_size * (m1 / denom)                          # addcdiv_(exp_avg, denom, -step_size)
    return np.where(live, p1, p), np.where(live, m1, m), np.where(live, v1, v)


def ulp32(x):
    """Spacing of float32 at |x|, as float64."""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def worst_ratio(err, bound):
    # 0 / 0 is inside the bound; anything / 0 is outside it
    with np.errstate(divide="ignore", invalid="ignore"):
        r = err / bound
    r = np.where((err == 0) & (bound == 0), 0.0, r)
    return float(np.max(r)) if r.size else 0.0


def bound_ratios(p, m, v, p_prev, g, m_prev, v_prev, lr, step, **adam):
    """Worst error / bound of one fp32 step (p, m, v after it) from the fp32 state before it, for
    each of the three quantities. A ratio <= 1 is inside the bound."""
    p64, m64, v64 = adam64(p_prev, g, m_prev, v_prev, lr, step, **adam)
    g64, mp64, pp64 = (np.asarray(x, np.float64) for x in (g, m_prev, p_prev))
    return {
        "v": worst_ratio(np.abs(np.asarray(v, np.float64) - v64), V_REL * v64),
        "m": worst_ratio(np.abs(np.asarray(m, np.float64) - m64), M_REL * np.maximum(np.abs(g64), np.abs(mp64))),
        "p": worst_ratio(np.abs(np.asarray(p, np.float64) - p64), P_ULPS * ulp32(p64) + P_STEP * np.abs(p64 - pp64)),
    }


def assert_adam_bounds(what, p, m, v, p_prev, g, m_prev, v_prev, lr, step, **adam):
    """Hold one fp32 step to the three bounds; elements with step <= 0 must be bit-identical."""
    step_e = np.broadcast_to(np.asarray(step, np.int64), np.shape(p))
    skip = step_e <= 0
    for name, a, b in (("param", p, p_prev), ("exp_avg", m, m_prev), ("exp_avg_sq", v, v_prev)):
        a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
        assert np.array_equal(a[skip].view(np.uint32), b[skip].view(np.uint32)), f"{what}: skipped {name} changed"
    r = bound_ratios(p, m, v, p_prev, g, m_prev, v_prev, lr, step, **adam)
    for k, x in r.items():
        assert x <= 1.0, f"{what}: {k} is {x:.3g} x its bound ({r})"
    return r
