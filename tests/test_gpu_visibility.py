"""Visibility baking on the GPU (csrc/visibility.hip, the centre-ray trace of csrc/bvh.hip,
relightable3dgaussian_amd/visibility.py) against tests/visibility_ref64.py, the reference's own float32
results (tests/golden/visibility.npz), the array trace `_C.trace_bvh_opacity` (bit for bit with one lane per
ray) and the BVH oracle. Bars and the undecided-ray rule: tests/visibility_ref64.py."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

import oracle
from tests import visibility_ref64 as v64
from tests._helpers import lib_options
from tests.test_bvh import near_cut, scene, tt

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_visibility as mgv  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def vis():
    from relightable3dgaussian_amd import visibility

    return visibility


def cat(dc, rest):
    dc, rest = np.asarray(dc), np.asarray(rest)
    return np.concatenate([dc.reshape(dc.shape[0], -1), rest.reshape(dc.shape[0], -1)], 1)


def hip_loss(c, index=None, upstream=None, normals=True):
    """visibility_sh_loss + backward through autograd -> (loss, grad_dc, grad_rest) as numpy."""
    import torch

    dc, rest = tt(c["dc"]).requires_grad_(True), tt(c["rest"]).requires_grad_(True)
    loss = vis().visibility_sh_loss(dc, rest, tt(c["dirs"]), tt(c["traced"]), tt(c["normals"]) if normals else None,
                                    None if index is None else tt(index))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss if upstream is None else loss * upstream).backward()
    return float(loss.detach()), dc.grad.cpu().numpy(), rest.grad.cpu().numpy()


def hip_fit(hip_ext, draws, lr=1e-2):
    """The fused fit step over the per-step draws -> ([loss], [(dc, rest) after each step])."""
    import torch

    dc, rest, n = tt(draws[0]["dc"]), tt(draws[0]["rest"]), tt(draws[0]["normals"])
    st = [torch.zeros_like(dc), torch.zeros_like(rest), torch.zeros_like(dc), torch.zeros_like(rest)]
    losses = torch.zeros(len(draws), device="cuda")
    after = []
    for s, c in enumerate(draws):
        hip_ext.visibility_sh_fit_step(dc, rest, tt(c["dirs"]), tt(c["traced"]), n, *st, s + 1, lr, 0.9, 0.999, 1e-8,
                                       losses, s)
        after.append((dc.cpu().numpy(), rest.cpu().numpy()))
    return losses.cpu().numpy(), after


def check_loss(got, ref):
    e = abs(got - ref) / abs(ref) if ref else abs(got)
    print(f"loss {got:.9g} ref64 {ref:.9g} rel {e:.2e} (bar {v64.BARS['loss']:.1e})")
    assert e <= v64.BARS["loss"]


def check_grad(gdc, grest, e, scale=1.0):
    P = gdc.shape[0]
    ok = mgv.decided_rows(e, P)
    assert ok.mean() >= 1 - v64.UNDECIDED_MAX
    ref = cat(e["grad_dc"], e["grad_rest"]) * scale
    err = v64.rel_err(cat(gdc, grest)[ok], ref[ok])
    print(f"grad rel {err:.2e} (bar {v64.BARS['grad']:.1e}), {int((~ok).sum())} rows left out")
    assert err <= v64.BARS["grad"]


def check_fit(losses, after, draws, golden_params=None):
    fit = v64.Fit(draws[0]["dc"], draws[0]["rest"], draws[0]["normals"])
    refs = []
    for c in draws:
        refs.append((fit.step(c["dirs"], c["traced"]), fit.dc.copy(), fit.rest.copy()))
    ok = ~fit.undecided
    assert ok.mean() >= 1 - v64.UNDECIDED_MAX
    for s, (rl, rdc, rrest) in enumerate(refs):
        check_loss(float(losses[s]), rl)
        got, ref = cat(*after[s])[ok], cat(rdc, rrest)[ok]
        err = v64.rel_err(got, ref)
        print(f"step {s + 1}: params rel {err:.2e} (bar {v64.BARS['params']:.1e})")
        assert err <= v64.BARS["params"]
        np.testing.assert_allclose(got, ref, rtol=v64.ADAM_RTOL, atol=v64.ADAM_ATOL)
        if golden_params is not None:
            np.testing.assert_allclose(got, cat(*golden_params[s])[ok], rtol=v64.ADAM_RTOL, atol=v64.ADAM_ATOL)
    return fit


# ---- golden cases ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(mgv.CASES))
def test_golden_loss_gradient_and_fit(hip_ext, name):
    g = np.load(os.path.join(HERE, "golden", "visibility.npz"))
    draws = [dict(dc=g[f"{name}_dc"], rest=g[f"{name}_rest"], normals=g[f"{name}_normals"],
                  dirs=g[f"{name}_dirs_step{s + 1}"], traced=g[f"{name}_traced_step{s + 1}"]) for s in range(mgv.STEPS)]
    loss, gdc, grest = hip_loss(draws[0])
    e = v64.evaluate(**draws[0])
    check_loss(loss, e["loss"])
    check_grad(gdc, grest, e)
    ci = dict(draws[0], dirs=g[f"{name}_idx_dirs"], traced=g[f"{name}_idx_traced"])
    loss, gdc, grest = hip_loss(ci, index=g[f"{name}_idx"])
    ei = mgv.golden_index(g, name)
    check_loss(loss, ei["loss"])
    check_grad(gdc, grest, ei)
    named = np.zeros(mgv.P, bool)
    named[g[f"{name}_idx"]] = True
    assert not cat(gdc, grest)[~named].any()  # rows the index does not name are exactly zero
    losses, after = hip_fit(hip_ext, draws)
    check_fit(losses, after, draws,
              [(g[f"{name}_dc_step{s + 1}"], g[f"{name}_rest_step{s + 1}"]) for s in range(mgv.STEPS)])


# ---- shapes against ref64 -------------------------------------------------------------------------

@pytest.mark.parametrize("K", v64.KS)
@pytest.mark.parametrize("P", v64.SHAPE_PS)
def test_shapes_loss_gradient_and_fit(hip_ext, P, K):
    draws = v64.fit_draws(P, K, v64.shape_seed(P, K), v64.SHAPE_STEPS)
    loss, gdc, grest = hip_loss(draws[0])
    assert gdc.shape == (P, 1, 1) and grest.shape == (P, K - 1, 1)
    e = v64.evaluate(**draws[0])
    check_loss(loss, e["loss"])
    check_grad(gdc, grest, e)
    losses, after = hip_fit(hip_ext, draws)
    check_fit(losses, after, draws)


@pytest.mark.parametrize("K", v64.KS)
def test_indexed_loss(hip_ext, K):
    c = v64.index_draw(v64.INDEX_P, K, v64.INDEX_SEED, v64.INDEX_N)
    idx = c.pop("index")
    loss, gdc, grest = hip_loss(c, index=idx)
    e = v64.evaluate(c["dc"], c["rest"], c["dirs"], c["traced"], c["normals"], idx)
    check_loss(loss, e["loss"])
    check_grad(gdc, grest, e)
    loss32, gdc32, grest32 = hip_loss(c, index=idx.astype(np.int32))
    assert loss32 == loss and np.array_equal(gdc32, gdc) and np.array_equal(grest32, grest)


def test_repeated_index_rows_accumulate(hip_ext):
    c = v64.draw_case(10, 4, 5, R=6)
    idx = np.array([3, 3, 3, 7, 0, 7])
    loss, gdc, grest = hip_loss(c, index=idx)
    e = v64.evaluate(c["dc"], c["rest"], c["dirs"], c["traced"], c["normals"], idx)
    assert not e["undecided"].any()
    check_loss(loss, e["loss"])
    check_grad(gdc, grest, e)


# ---- exact cases ----------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [4, 25])
def test_zero_coefficients_give_exact_results(hip_ext, K):
    P = 70
    c = v64.draw_case(P, K, 9)
    c["dc"][:], c["rest"][:] = 0, 0
    c["traced"][:] = 0.5
    loss, gdc, grest = hip_loss(c)
    assert loss == 0.0 and not gdc.any() and not grest.any()  # s is exactly 0.5
    b32 = v64.basis(v64.flip32(c["dirs"], c["normals"]), K, F)  # float32, the kernel's operation order
    for traced, sign in ((0.0, 1.0), (1.0, -1.0)):
        c["traced"][:] = traced
        loss, gdc, grest = hip_loss(c)
        assert loss == 0.5
        want = (F(sign) * b32) / F(P)
        assert np.array_equal(cat(gdc, grest).view(np.uint32), want.view(np.uint32))


def test_zero_dot_product_is_not_flipped(hip_ext):
    """Rows 0 / 1: d . n == 0 exactly (kept); row 2: negative (flipped); row 3: positive (kept). The z
    coefficient alone is non-zero, so the gradient's sign shows which way d pointed."""
    d = np.array([[1, 0, 0.5], [2, -2, 0.25], [0, 0, 0.5], [0, 0, 0.5]], F)
    n = np.array([[0, 1, 0], [1, 1, 0], [0, 0, -1], [0, 0, 1]], F)
    c = dict(dc=np.zeros((4, 1, 1), F), rest=np.zeros((4, 3, 1), F), dirs=d, normals=n, traced=np.zeros(4, F))
    _, gdc, grest = hip_loss(c)
    want = v64.basis(v64.flip32(d, n), 4, F) / F(4)
    assert np.array_equal(cat(gdc, grest), want)
    assert (grest[[0, 1, 3], 1, 0] > 0).all() and grest[2, 1, 0] < 0  # basis_2 = C1 * z
    _, _, unflipped = hip_loss(c, normals=False)
    assert unflipped[2, 1, 0] > 0


# ---- Adam behaviour -------------------------------------------------------------------------------

def test_zero_gradient_still_takes_its_adam_step(hip_ext):
    """Step 1: raw + 0.5 inside (0, 1) and traced 0, a gradient. Step 2: a direction 20 times as long pushes
    raw + 0.5 above 1, the clamp closes and the gradient is exactly zero; the moments decay and the
    coefficients still move, as torch.optim.Adam moves zero entries of a present gradient."""
    P = 3
    base = dict(dc=np.zeros((P, 1, 1), F), rest=np.tile(np.array([0, 1, 0], F)[None, :, None], (P, 1, 1)),
                normals=np.tile(np.array([[0, 0, 1]], F), (P, 1)))
    draws = [dict(base, dirs=np.tile(np.array([[0, 0, 0.5]], F), (P, 1)), traced=np.zeros(P, F)),
             dict(base, dirs=np.tile(np.array([[0, 0, 10.0]], F), (P, 1)), traced=np.ones(P, F))]
    losses, after = hip_fit(hip_ext, draws)
    fit = check_fit(losses, after, draws)
    assert not fit.last["sgn"].any()  # step 2's gradient is zero
    assert (after[1][1][:, 1, 0] < after[0][1][:, 1, 0]).all() and (after[0][1][:, 1, 0] < 1).all()
    assert losses[1] == 0.0


# ---- the loss as an autograd function -------------------------------------------------------------

def test_autograd_upstream_factor_and_reproducibility(hip_ext):
    import torch

    c = v64.draw_case(1000, 16, v64.SHAPE_SEED)
    e = v64.evaluate(**c)
    up = torch.tensor(0.01, device="cuda")
    loss, gdc, grest = hip_loss(c, upstream=up)
    check_loss(loss, e["loss"])
    check_grad(gdc, grest, e, scale=float(np.float32(0.01)))
    loss2, gdc2, grest2 = hip_loss(c, upstream=up)
    assert loss2 == loss and np.array_equal(gdc2, gdc) and np.array_equal(grest2, grest)
    with pytest.raises(ValueError):
        vis().visibility_sh_loss(tt(c["dc"]), tt(c["rest"]), tt(c["dirs"]).requires_grad_(True), tt(c["traced"]))


# ---- fibonacci_dirs -------------------------------------------------------------------------------

@pytest.mark.parametrize("Ns", [1, 7, 24, 384])
def test_fibonacci_dirs(hip_ext, Ns):
    """Held to ref64 at FIB_BAR = 4 x the floor measured from tests/golden/fib.npz (Ns = 24, random normals).
    The reference's float32 formula (csrc/sh_dirs.h relight_fib_dir, which the render equation keeps) misses
    that bar at Ns = 384: its sample angle float(delta) * r is one rounded product, 3e-5 rad at r = 383
    (2.8e-05 of the direction over these random normals), and for the near-pole normal (eps, 0, -1 + eps^2)
    the rotation divides by 1 + n_z = 1.0e-6, which amplifies that to 1.06e-03. fibonacci_dirs and the centre
    trace therefore evaluate the sample in double and round once (fib_dir)."""
    rng = np.random.default_rng(Ns)
    n = rng.normal(size=(67, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    eps = 1e-3
    n[0] = (0, 0, -1)
    n[1] = (eps, 0, -1 + eps * eps)
    n[2] = (0, 0, 1)
    n = n.astype(F)
    got = vis().fibonacci_dirs(tt(n), Ns).cpu().numpy()
    assert got.shape == (67, Ns, 3)
    err = v64.rel_err(got, v64.fibonacci_dirs(n, Ns))
    print(f"Ns {Ns}: fibonacci_dirs vs ref64 {err:.3e} (bar {v64.FIB_BAR:.1e})")
    assert err <= v64.FIB_BAR


# ---- centre trace ---------------------------------------------------------------------------------

def trace_inputs(sc):
    return tt(sc["means"]), tt(sc["cov_inv"]), tt(sc["opacity"]), tt(sc["normals"])


def hold_to_oracle(sc, nodes, aabbs, o, d, c, v, min_ok=0.999):
    """tests/test_bvh.py compare_opacity for results that are already there."""
    rc, rv, t_last, nt = oracle.bvh_trace_opacity(nodes.cpu().numpy(), aabbs.cpu().numpy(), o, d, sc["means"],
                                                  sc["cov_inv"], sc["opacity"], sc["normals"], with_terms=True)
    ok = ~near_cut(t_last, nt)
    assert ok.mean() >= min_ok
    np.testing.assert_array_equal(c[ok], rc[ok])
    np.testing.assert_allclose(v[ok], rv[ok], rtol=0, atol=2e-5)


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("P", [1, 2, 3000])
def test_centre_trace_given_directions(hip_ext, P, indexed, flip):
    from relightable3dgaussian_amd.bvh import RayTracer

    sc = scene(P, seed=P + 3, spread=0.5)
    rt = RayTracer(tt(sc["means"]), tt(sc["scales"]), tt(sc["rots"]))
    rng = np.random.default_rng(P + 2 * indexed + flip)
    idx = rng.integers(0, P, 700) if indexed else np.arange(P)
    Ns = 2
    d = rng.normal(size=(len(idx), Ns, 3)).astype(F)
    d[0, 0] = (1, 0, 0)
    sc["normals"][idx[0]] = (0, 1, 0)  # a dot product of exactly 0: not flipped
    rows = np.repeat(idx, Ns)
    o = np.ascontiguousarray(sc["means"][rows])
    dd = d.reshape(-1, 3)
    df = np.ascontiguousarray(v64.flip32(dd, sc["normals"][rows]) if flip else dd)
    assert np.array_equal(df[0], dd[0]) and (not flip or P < 3 or (df != dd).any())
    args = trace_inputs(sc)

    def centres():
        res = rt.trace_from_centres(tt(d), *args, index=tt(idx) if indexed else None, flip=flip, sample_num=Ns)
        assert tuple(res["visibility"].shape) == (len(idx), Ns, 1) == tuple(res["contribute"].shape)
        return res["contribute"].cpu().numpy().reshape(-1), res["visibility"].cpu().numpy().reshape(-1)

    with lib_options(test_bvh_lanes=1):  # the reference's order: bit-equal to the array trace, flip included
        c, v = centres()
        ac, av = hip_ext.trace_bvh_opacity(rt.tree, rt.aabb, tt(o), tt(df), *args)
        assert np.array_equal(c, ac.cpu().numpy()) and np.array_equal(v.view(np.uint32), av.cpu().numpy().view(np.uint32))
    hold_to_oracle(sc, rt.tree, rt.aabb, o, df, *centres())
    with lib_options(test_bvh_sort=2):
        hold_to_oracle(sc, rt.tree, rt.aabb, o, df, *centres())


@pytest.mark.parametrize("Ns", [1, 7, 24])
def test_centre_trace_fibonacci_and_precompute(hip_ext, Ns):
    import torch

    from relightable3dgaussian_amd import relight
    from relightable3dgaussian_amd.bvh import RayTracer

    P = 2000
    sc = scene(P, seed=Ns + 40, spread=0.5)
    rt = RayTracer(tt(sc["means"]), tt(sc["scales"]), tt(sc["rots"]))
    args = trace_inputs(sc)
    dirs = vis().fibonacci_dirs(args[3], Ns)
    o = tt(sc["means"])[:, None].expand(P, Ns, 3).contiguous()
    with lib_options(test_bvh_lanes=1):
        res = rt.trace_from_centres(None, *args, sample_num=Ns)
        ac, av = hip_ext.trace_bvh_opacity(rt.tree, rt.aabb, o, dirs, *args)
        assert tuple(res["visibility"].shape) == (P, Ns, 1)
        assert torch.equal(res["contribute"][..., 0], ac)
        assert np.array_equal(res["visibility"][..., 0].cpu().numpy().view(np.uint32), av.cpu().numpy().view(np.uint32))
    on, dn = o.cpu().numpy().reshape(-1, 3), dirs.cpu().numpy().reshape(-1, 3)
    for opts in ({}, {"test_bvh_sort": 2}):
        with lib_options(**opts):
            res = rt.trace_from_centres(None, *args, sample_num=Ns)
            hold_to_oracle(sc, rt.tree, rt.aabb, on, dn, res["contribute"].cpu().numpy().reshape(-1),
                           res["visibility"].cpu().numpy().reshape(-1))
            pre = vis().precompute_visibility(rt, *args, Ns)
            assert tuple(pre.shape) == (P, Ns, 1) and torch.equal(pre, res["visibility"])
    assert (pre == 0).any() and ((pre > 0) & (pre < 1)).any()
    rng = np.random.default_rng(0)
    view = rng.normal(size=(P, 3))
    view /= np.linalg.norm(view, axis=1, keepdims=True)
    _, extra, feats = relight.render_equation_relight(
        tt(rng.uniform(0, 1, (P, 3)).astype(F)), tt(rng.uniform(0.05, 1, (P, 1)).astype(F)),
        tt(rng.uniform(0, 1, (P, 1)).astype(F)), args[3], tt(view.astype(F)),
        tt(rng.normal(0, 0.1, (P, 16, 3)).astype(F)), None, None, Ns, False, visibility_precompute=pre)
    assert tuple(feats.shape) == (P, 21) and bool(torch.isfinite(feats).all())
    np.testing.assert_allclose(extra["incident_visibility"][:, 0].cpu().numpy(),
                               pre[..., 0].double().mean(1).cpu().numpy(), rtol=0, atol=1e-6)


def test_precompute_allocates_nothing_proportional_to_the_rays(hip_ext):
    import torch

    from relightable3dgaussian_amd.bvh import RayTracer

    P, Ns = 20000, 24
    R = P * Ns
    sc = scene(P, seed=77, spread=0.6)
    rt = RayTracer(tt(sc["means"]), tt(sc["scales"]), tt(sc["rots"]))
    args = trace_inputs(sc)
    with lib_options(test_bvh_sort=2):
        vis().precompute_visibility(rt, *args, Ns)  # warm the allocator's pools and rocPRIM
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        pre = vis().precompute_visibility(rt, *args, Ns)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - before - pre.numel() * 4
        res = rt.trace_from_centres(None, *args, sample_num=Ns)
    print(f"peak beyond the output: {extra} B = {extra / R:.2f} B per ray (bound 12)")
    assert extra < 12 * R  # one materialised [R, 3] ray array, of which the array path needs two
    assert torch.equal(res["visibility"], pre)
    # the sorted order (slot -> perm[slot / Ns], slot % Ns) traces the right rays: a sample against the oracle
    sel = np.random.default_rng(1).choice(R, 3000, replace=False)
    dirs = vis().fibonacci_dirs(args[3], Ns).cpu().numpy().reshape(-1, 3)[sel]
    hold_to_oracle(sc, rt.tree, rt.aabb, np.ascontiguousarray(sc["means"][sel // Ns]), np.ascontiguousarray(dirs),
                   res["contribute"].cpu().numpy().reshape(-1)[sel], pre.cpu().numpy().reshape(-1)[sel])


# ---- finetune_visibility --------------------------------------------------------------------------

def test_finetune_visibility_matches_a_host_loop(hip_ext):
    import torch

    from relightable3dgaussian_amd.bvh import RayTracer

    P, K, iters = 500, 16, 5
    sc = scene(P, seed=13, spread=0.4)
    rt = RayTracer(tt(sc["means"]), tt(sc["scales"]), tt(sc["rots"]))
    args = trace_inputs(sc)
    c = v64.draw_case(P, K, 21)

    def run():
        dc, rest = tt(c["dc"]), tt(c["rest"])
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1234)
        losses = vis().finetune_visibility(dc, rest, rt, *args, iterations=iters, generator=gen)
        return losses.cpu().numpy(), dc.cpu().numpy(), rest.cpu().numpy()

    losses, dc, rest = run()
    assert losses.shape == (iters,)
    # the host loop: the same draws, the array trace on explicit (flipped) arrays, ref64's step
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    fit = v64.Fit(c["dc"], c["rest"], sc["normals"])
    ref_losses = []
    for _ in range(iters):
        d = torch.randn((P, 3), dtype=torch.float32, device="cuda", generator=gen).cpu().numpy()
        df = v64.flip32(d, sc["normals"])
        _, traced = hip_ext.trace_bvh_opacity(rt.tree, rt.aabb, args[0], tt(df), *args)
        ref_losses.append(fit.step(d, traced.cpu().numpy()))
    ok = ~fit.undecided
    print(f"{int((~ok).sum())} of {P} Gaussians undecided in some step")
    assert ok.mean() >= 1 - v64.UNDECIDED_MAX  # the draws are the GPU generator's, so this is checked here
    for s in range(iters):
        check_loss(float(losses[s]), ref_losses[s])
    got, ref = cat(dc, rest)[ok], cat(fit.dc, fit.rest)[ok]
    err = v64.rel_err(got, ref)
    print(f"params after {iters} steps: rel {err:.2e} (bar {v64.BARS['params']:.1e})")
    assert err <= v64.BARS["params"]
    np.testing.assert_allclose(got, ref, rtol=v64.ADAM_RTOL, atol=v64.ADAM_ATOL)
    losses2, dc2, rest2 = run()
    assert np.array_equal(losses2, losses) and np.array_equal(dc2, dc) and np.array_equal(rest2, rest)


# ---- argument errors ------------------------------------------------------------------------------

def test_argument_errors(hip_ext):
    import torch

    from relightable3dgaussian_amd.bvh import RayTracer

    P = 8
    c = v64.draw_case(P, 16, 1)
    dc, rest, d, t, n = tt(c["dc"]), tt(c["rest"]), tt(c["dirs"]), tt(c["traced"]), tt(c["normals"])
    with pytest.raises(RuntimeError, match="K must be"):
        vis().visibility_sh_loss(dc, tt(np.zeros((P, 4, 1), F)), d, t, n)  # K = 5
    with pytest.raises(RuntimeError):
        vis().visibility_sh_loss(dc, rest, d[:0], t[:0], n, torch.zeros(0, dtype=torch.int64, device="cuda"))  # R = 0
    with pytest.raises(RuntimeError):
        vis().visibility_sh_loss(dc, rest[:P - 1], d, t, n)  # mismatched P
    with pytest.raises(RuntimeError):
        vis().visibility_sh_loss(dc, rest, d[:5], t[:5], n)  # R != P without index
    with pytest.raises(RuntimeError):
        vis().visibility_sh_loss(dc, rest, d, t[:5], n)
    sc = scene(P, seed=1, spread=0.5)
    rt = RayTracer(tt(sc["means"]), tt(sc["scales"]), tt(sc["rots"]))
    args = trace_inputs(sc)
    with pytest.raises(RuntimeError):
        rt.trace_from_centres(tt(np.zeros((P * 3 + 1, 3), F)), *args, sample_num=3)  # R no multiple of Ns
    with pytest.raises(RuntimeError):
        rt.trace_from_centres(tt(np.zeros((P - 1, 3), F)), *args)  # R != P without index
    with pytest.raises(ValueError):
        rt.trace_from_centres(None, *args)  # Fibonacci mode needs sample_num
    # an index entry outside [0, P) is the caller's contract (the array is on the device: checking it would
    # read it back); it is documented in include/r3dg_hip.h and not exercised here
