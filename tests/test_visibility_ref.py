"""CPU tests of the visibility-baking test infrastructure and bindings: tests/visibility_ref64.py against the
reference's own float32 results (tests/golden/visibility.npz), the share of undecided rays of every seeded
case the GPU tests use, ref64's Fibonacci directions against tests/golden/fib.npz, and the bindings' refusal
of CPU tensors (the product has no CPU path)."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from tests import relight_ref64
from tests import visibility_ref64 as v64

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_visibility as mgv  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "visibility.npz"))


def test_ref64_reproduces_golden_within_floors(golden):
    worst = mgv.measure(golden)
    for k, floor in v64.FLOORS.items():
        print(f"{k}: golden vs ref64 {worst[k]:.3e} (floor {floor:.1e})")
        assert worst[k] <= floor, (k, worst[k])
        assert worst[k] > floor / 4, (k, worst[k], "the floor is not the measurement any more")


def test_golden_cases_cover_the_clamp_and_the_traced_values(golden):
    for name in mgv.CASES:
        _, _, first = mgv.golden_fit(golden, name)
        u = first["basis"] @ np.concatenate([golden[f"{name}_dc"].reshape(mgv.P, 1),
                                             golden[f"{name}_rest"].reshape(mgv.P, -1)], 1).astype(np.float64).T
        u = np.diag(u) + 0.5
        assert (u < 0).mean() > 0.05 and (u > 1).mean() > 0.05 and ((u >= 0) & (u <= 1)).mean() > 0.3
        t = golden[f"{name}_traced_step1"]
        assert 0.2 < (t == 0).mean() < 0.4 and 0.1 < (t == 1).mean() < 0.3 and ((t > 0.9) & (t < 1)).mean() > 0.4
        assert len(np.unique(golden[f"{name}_idx"])) == mgv.N_INDEX


def test_undecided_share_of_golden_cases(golden):
    for name in mgv.CASES:
        fit, _, first = mgv.golden_fit(golden, name)
        for e in (first, mgv.golden_index(golden, name)):
            assert e["undecided"].mean() <= v64.UNDECIDED_MAX, name
        assert fit.undecided.mean() <= v64.UNDECIDED_MAX, name  # over the three steps


def test_undecided_share_of_every_gpu_seed():
    for P in v64.SHAPE_PS:
        for K in v64.KS:
            draws = v64.fit_draws(P, K, v64.shape_seed(P, K), v64.SHAPE_STEPS)
            fit, _, evals = v64.run_fit(draws)
            assert fit.undecided.mean() <= v64.UNDECIDED_MAX, (P, K)
            assert v64.fit32_error(draws) <= v64.BARS["params"], (P, K)  # the specification's own float32 error
    # the draw that SHAPE_SEEDS steps over: below Adam's eps a gradient entry's rounding reaches the parameter
    assert v64.fit32_error(v64.fit_draws(1000, 25, 0, 1)) > v64.BARS["params"]
    for K in v64.KS:
        c = v64.index_draw(v64.INDEX_P, K, v64.INDEX_SEED, v64.INDEX_N)
        e = v64.evaluate(c["dc"], c["rest"], c["dirs"], c["traced"], c["normals"], c["index"])
        assert e["undecided"].mean() <= v64.UNDECIDED_MAX, K
        assert np.abs(e["grad_rest"]).sum() > 0 or K == 1


def test_ref64_gradient_is_the_finite_difference_of_its_loss():
    c = v64.draw_case(40, 9, 3)
    e = v64.evaluate(c["dc"], c["rest"], c["dirs"], c["traced"], c["normals"])
    ok = mgv.decided_rows(e, 40)
    h = 1e-6
    for g in np.nonzero(ok)[0][:10]:
        for k in (0, 3, 7):
            rest = c["rest"].astype(np.float64)
            rest[g, k, 0] += h
            up = v64.evaluate(c["dc"], rest, c["dirs"], c["traced"], c["normals"])["loss"]
            rest[g, k, 0] -= 2 * h
            dn = v64.evaluate(c["dc"], rest, c["dirs"], c["traced"], c["normals"])["loss"]
            assert abs((up - dn) / (2 * h) - e["grad_rest"][g, k, 0]) < 1e-7


def test_float32_flip_and_basis():
    d = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [1e-30, -1e-30, 0]], np.float32)
    n = np.array([[-1, 0, 0], [-1, 0, 0], [1, 0, 0], [1, 1, 0]], np.float32)
    f = v64.flip32(d, n)
    assert np.array_equal(f[0], -d[0]) and np.array_equal(f[1], d[1])
    assert np.array_equal(f[2], d[2])  # a dot product of 0 does not flip
    assert np.array_equal(f[3], d[3])  # (1e-30 - 1e-30) + 0 == 0
    b32 = v64.basis(np.random.default_rng(0).normal(size=(50, 3)).astype(np.float32), 25, np.float32)
    assert b32.dtype == np.float32 and b32.shape == (50, 25)
    b64 = v64.basis(np.random.default_rng(0).normal(size=(50, 3)).astype(np.float32).astype(np.float64), 25)
    assert relight_ref64.rel_err(b32, b64) < 1e-6
    # the basis is the degree-4 basis of the relighting restatement
    import torch

    dd = np.random.default_rng(1).normal(size=(20, 3))
    np.testing.assert_allclose(v64.basis(dd, 25), relight_ref64.sh_basis25(torch.from_numpy(dd)).numpy(), rtol=1e-14)


def test_ref64_fibonacci_dirs_agree_with_fib_golden_and_relight_ref64():
    f = np.load(os.path.join(HERE, "golden", "fib.npz"))
    ours = v64.fibonacci_dirs(f["normals"], f["dirs"].shape[1])
    e = v64.rel_err(f["dirs"], ours)
    print(f"fib.npz vs ref64: {e:.3e} (floor {v64.FIB_FLOOR:.1e})")
    assert v64.FIB_FLOOR / 4 < e <= v64.FIB_FLOOR
    assert np.array_equal(ours, relight_ref64.fibonacci_dirs(f["normals"].astype(np.float64), f["dirs"].shape[1]).numpy())
    np.testing.assert_allclose(np.linalg.norm(ours, axis=-1), 1.0, rtol=1e-14)


def test_bindings_refuse_cpu_tensors():
    import torch

    import relightable3dgaussian_amd as r
    from relightable3dgaussian_amd import visibility

    P = 4
    dc, rest = torch.zeros(P, 1, 1), torch.zeros(P, 15, 1)
    d, t, n = torch.randn(P, 3), torch.rand(P), torch.randn(P, 3)
    with pytest.raises(RuntimeError):
        visibility.visibility_sh_loss(dc, rest, d, t, n)
    with pytest.raises(RuntimeError):
        r._C.visibility_sh_loss_backward(dc, rest, d, t, n, None, torch.ones(()))
    with pytest.raises(RuntimeError):
        r._C.visibility_sh_fit_step(dc, rest, d, t, n, dc.clone(), rest.clone(), dc.clone(), rest.clone(), 1, 1e-2,
                                    0.9, 0.999, 1e-8, torch.zeros(1), 0)
    with pytest.raises(RuntimeError):
        visibility.fibonacci_dirs(n, 24)
    with pytest.raises(RuntimeError):
        r._C.trace_bvh_opacity_centres(torch.zeros(2 * P - 1, 5, dtype=torch.int32), torch.zeros(2 * P - 1, 6), d,
                                       torch.zeros(P, 3), torch.zeros(P, 6), torch.ones(P), n)


def test_loss_refuses_a_direction_that_requires_grad():
    import torch

    from relightable3dgaussian_amd import visibility

    d = torch.randn(4, 3, requires_grad=True)
    with pytest.raises(ValueError):
        visibility.visibility_sh_loss(torch.zeros(4, 1, 1), torch.zeros(4, 15, 1), d, torch.rand(4))
    with pytest.raises(ValueError):
        visibility.visibility_sh_loss(torch.zeros(4, 1, 1), torch.zeros(4, 15, 1), torch.randn(4, 3),
                                      torch.rand(4, requires_grad=True))
