"""Inputs of the training-step edge tests (tests/test_train_ref64.py on the CPU,
tests/test_gpu_train_edges.py on the GPU): Adam over the 14-group layout at sizes where the group
boundaries fall at every residue mod 4, and densify / prune models in which every class of
Gaussian is present and every mask is unambiguous.

Test infrastructure only (not collected: no test_ prefix)."""
from __future__ import annotations

import types

import numpy as np

from oracle import train_oracle as T

F = np.float32
NAMES = [n for n, _ in T.GROUPS]
WIDTHS = [w for _, w in T.GROUPS]
ADAM_P = (1, 3, 37)
MARGIN = 1e-3  # relative distance every compared value keeps from its threshold


# ---- Adam ---------------------------------------------------------------------------------------

def adam_case(P, seed=0, widths=WIDTHS):
    """Flat fp32 buffers of a P-Gaussian model: a distinct learning rate 1e-3 (g + 1) and a distinct
    step count g + 1 per group, three fresh gradients whose magnitude per group is 10 ** U(-4, -1)
    (nothing denormal) with some exact zeros, and a non-zero Adam state for every group that has
    stepped before. Parameters are +-U(0.05, 2): the parameter bound has ulp32(p) as its absolute
    term, so p stays well above the step (lr <= 1.4e-2)."""
    rng = np.random.default_rng(1000 * P + seed)
    G = len(widths)
    bounds = np.cumsum([0] + [P * w for w in widths])
    total = int(bounds[-1])
    gid = np.repeat(np.arange(G), [P * w for w in widths])
    c = types.SimpleNamespace(P=P, widths=list(widths), bounds=bounds, total=total, gid=gid)
    c.lrs = [1e-3 * (g + 1) for g in range(G)]
    c.steps0 = [g + 1 for g in range(G)]
    c.p0 = (rng.choice([-1.0, 1.0], size=total) * rng.uniform(0.05, 2.0, size=total)).astype(F)
    mag = 10.0 ** rng.uniform(-4, -1, size=G)
    seen = (np.asarray(c.steps0) > 1)[gid]
    c.m0 = np.where(seen, rng.normal(size=total) * mag[gid], 0.0).astype(F)
    c.v0 = np.where(seen, (rng.normal(size=total) * mag[gid]) ** 2, 0.0).astype(F)
    c.grads = []
    for _ in range(3):
        mag = 10.0 ** rng.uniform(-4, -1, size=G)
        g = (rng.normal(size=total) * mag[gid]).astype(F)
        g[rng.random(total) < 0.06] = 0.0
        c.grads.append(g)
    return c


def steps_at(c, k, skip=()):
    """Per-group step counts of step k (0-based); groups in `skip` (indices) get 0 = no gradient."""
    return [0 if g in skip else s + k for g, s in enumerate(c.steps0)]


def per_elem(c, vals, lo=0, hi=None):
    """One value per group -> one per element of [lo, hi)."""
    return np.asarray(vals)[c.gid[lo:c.total if hi is None else hi]]


def oracle_adam(c, p, g, m, v, steps, lo=0, hi=None):
    """oracle/train_oracle.adam_step over the flat range [lo, hi), group by group (one step count
    each; <= 0 skips). p is the whole buffer, g / m / v hold the range. Returns new (p, m, v)."""
    hi = c.total if hi is None else hi
    p, m, v = np.array(p, F), np.array(m, F), np.array(v, F)
    for gi, (a, b) in enumerate(zip(c.bounds[:-1], c.bounds[1:])):
        a, b = max(int(a), lo), min(int(b), hi)
        if a >= b or steps[gi] <= 0:
            continue
        sl = slice(a - lo, b - lo)
        p[a:b], m[sl], v[sl] = T.adam_step(p[a:b], g[sl], m[sl], v[sl], c.lrs[gi], steps[gi])
    return p, m, v


# ---- densify / prune ----------------------------------------------------------------------------

# classes of Gaussian in a synthetic densify model
KEEP, LOW_OPACITY, CLONE, CLONE_PRUNED, SPLIT, SPLIT_BIG_CHILDREN, SPLIT_LOW_OPACITY, BIG_WORLD, \
    NAN_GRAD, INF_GRAD_CLONE, INF_GRAD_SPLIT, NORMAL_ONLY_CLONE, NORMAL_ONLY_SPLIT = range(13)
ALL_CLASSES = tuple(range(13))

LAYOUT14 = list(T.GROUPS)
# roles out of their usual order, and a group that has none
LAYOUT5 = [("opacity", 1), ("rotation", 4), ("extra", 5), ("scaling", 3), ("xyz", 3)]

DENSIFY = dict(max_grad=2e-4, min_opacity=0.005, extent=2.5, max_grad_normal=0.5, percent_dense=0.01)


def roles_of(layout):
    names = [n for n, _ in layout]
    return [names.index("xyz"), names.index("scaling"), names.index("rotation"), names.index("opacity")]


def off_thresholds(x, thresholds):
    """True where x is at least MARGIN (relative) away from every threshold."""
    x = np.asarray(x, np.float64)
    ok = np.ones(x.shape, bool)
    for t in thresholds:
        ok &= np.abs(x - t) >= MARGIN * abs(t)
    return ok


def assert_unambiguous(model, xyz_accum, normal_accum, denom, max_radii, N, max_screen_size=20.0, **d):
    """Every value a mask is made from keeps MARGIN from its threshold: each activated scale and
    each child's scale from percent_dense * extent and 0.1 * extent (the kernel forms these as
    float products, the reference as the double product rounded: they can differ by one ulp),
    sigmoid(opacity) from min_opacity, |grad| from its thresholds, max_radii2D from the screen size."""
    d = {**DENSIFY, **d}
    s = np.exp(model["scaling"].astype(np.float64))
    ths = (d["percent_dense"] * d["extent"], 0.1 * d["extent"])
    assert off_thresholds(s, ths).all() and off_thresholds(s / (0.8 * N), ths).all(), "scale on a threshold"
    sg = 1.0 / (1.0 + np.exp(-model["opacity"].astype(np.float64)))
    assert off_thresholds(sg, (d["min_opacity"],)).all(), "opacity on its threshold"
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.asarray(xyz_accum, np.float64) / np.asarray(denom, np.float64)
        gn = np.asarray(normal_accum, np.float64) / np.asarray(denom, np.float64)
    fin = np.isfinite(g)
    assert off_thresholds(g[fin], (d["max_grad"],)).all(), "gradient on its threshold"
    assert off_thresholds(gn[np.isfinite(gn)], (d["max_grad_normal"],)).all(), "normal gradient on its threshold"
    if max_screen_size:
        assert off_thresholds(max_radii, (max_screen_size,)).all(), "radius on the screen size"


def densify_case(P, classes=ALL_CLASSES, layout=LAYOUT14, N=2, seed=0):
    """A model whose Gaussian i is of class classes[i % len(classes)] (shuffled), with the inputs of
    r3dg_densify_and_prune: model / m / v dicts name -> [P, w], the statistics, and noise for
    every possible child."""
    d = DENSIFY
    rng = np.random.default_rng(77 * P + 13 * N + seed)
    cls = np.asarray([classes[i % len(classes)] for i in range(P)], int) if P else np.zeros(0, int)
    rng.shuffle(cls)
    dense, world, div = d["percent_dense"] * d["extent"], 0.1 * d["extent"], 0.8 * N
    is_in = lambda *cs: np.isin(cls, cs)
    model = {n: (rng.normal(size=(P, w)) * 0.5).astype(F) for n, w in layout}
    # largest activated scale by class; the other two axes are smaller
    smax = rng.uniform(0.08 * dense, min(0.9 * dense, 0.9 * world * div), size=P)           # clone-sized
    split_ok = rng.uniform(1.2 * dense, 0.96 * world * div, size=P)                          # children <= world
    split_big = rng.uniform(1.04 * world * div, 2.0 * world * div, size=P)                   # children > world
    smax = np.where(is_in(SPLIT, SPLIT_LOW_OPACITY, INF_GRAD_SPLIT, NORMAL_ONLY_SPLIT), split_ok, smax)
    smax = np.where(is_in(SPLIT_BIG_CHILDREN), split_big, smax)
    smax = np.where(is_in(BIG_WORLD), rng.uniform(1.04 * world, 3.0 * world, size=P), smax)
    s = smax[:, None] * rng.uniform(0.2, 0.9, size=(P, 3))
    if P:
        s[np.arange(P), rng.integers(0, 3, size=P)] = smax
    for t in (dense, world):  # nudge the few scales (parents' or children's) that fell on a threshold
        for k in (1.0, div):
            near = np.abs(s / k - t) < 4 * MARGIN * t
            s = np.where(near, s * 0.98, s)
    model["scaling"] = np.log(s).astype(F)
    low = is_in(LOW_OPACITY, CLONE_PRUNED, SPLIT_LOW_OPACITY)
    model["opacity"] = np.where(low, rng.uniform(-9.0, -5.6, size=P), rng.uniform(-5.0, 3.0, size=P)).astype(F)[:, None]
    m = {n: (rng.normal(size=(P, w)) * 1e-2).astype(F) for n, w in layout}
    v = {n: (rng.normal(size=(P, w)) ** 2 * 1e-4).astype(F) for n, w in layout}
    den = rng.integers(1, 6, size=P).astype(F)
    by_grad = is_in(CLONE, CLONE_PRUNED, SPLIT, SPLIT_BIG_CHILDREN, SPLIT_LOW_OPACITY)
    by_normal = is_in(NORMAL_ONLY_CLONE, NORMAL_ONLY_SPLIT)
    acc = np.where(by_grad, rng.uniform(1.5, 5.0, size=P), rng.uniform(0.0, 0.7, size=P)) * d["max_grad"] * den
    nacc = np.where(by_normal, rng.uniform(1.2, 2.0, size=P), rng.uniform(0.0, 0.8, size=P)) * d["max_grad_normal"] * den
    zero_den = is_in(NAN_GRAD, INF_GRAD_CLONE, INF_GRAD_SPLIT)
    den = np.where(zero_den, 0.0, den).astype(F)
    acc = np.where(is_in(NAN_GRAD), 0.0, acc)       # 0 / 0 = NaN -> 0: not selected
    nacc = np.where(is_in(NAN_GRAD), 0.0, nacc)
    acc = np.where(is_in(INF_GRAD_CLONE, INF_GRAD_SPLIT), d["max_grad"] * 0.3, acc)  # x / 0 = inf: selected
    c = types.SimpleNamespace(P=P, N=N, layout=list(layout), cls=cls, model=model, m=m, v=v,
                              xyz_accum=acc.astype(F), normal_accum=nacc.astype(F), denom=den,
                              max_radii=np.where(rng.random(P) < 0.3, rng.uniform(21.0, 40.0, size=P),
                                                 rng.uniform(0.0, 19.0, size=P)).astype(F),
                              noise=rng.normal(size=3 * N * max(P, 1)).astype(F))
    assert_unambiguous(model, c.xyz_accum, c.normal_accum, c.denom, c.max_radii, N)
    return c


def oracle_densify(c, max_screen_size, prune_only=False, noise=None, **d):
    d = {**DENSIFY, **d}
    return T.densify_and_prune(c.model, c.m, c.v, c.xyz_accum, c.normal_accum, c.denom, c.max_radii, d["max_grad"],
                               d["min_opacity"], d["extent"], max_screen_size, d["max_grad_normal"],
                               d["percent_dense"], c.noise if noise is None else noise, N=c.N,
                               prune_only=prune_only, return_source=True)


# ---- the reference-made fixture tests/golden/train_edges.npz -------------------------------------

RTOL, ATOL = 2e-5, 1e-6  # tests/test_train.py: child xyz and scaling restate fp32 arithmetic


def edges_case(gold):
    """The inputs of tests/golden/train_edges.npz as a densify case."""
    c = types.SimpleNamespace(P=int(gold["in_xyz"].shape[0]), N=2, layout=list(LAYOUT14))
    c.model = {n: gold[f"in_{n}"].astype(F) for n in NAMES}
    c.m = {n: gold[f"in_m_{n}"].astype(F) for n in NAMES}
    c.v = {n: gold[f"in_v_{n}"].astype(F) for n in NAMES}
    c.xyz_accum, c.normal_accum, c.denom = gold["in_xyz_accum"], gold["in_normal_accum"], gold["in_denom"]
    c.max_radii, c.noise = gold["in_max_radii2D"], gold["noise"]
    return c


def edges_want(gold, tag):
    return tuple({n: gold[f"{tag}_{pre}{n}"] for n in NAMES} for pre in ("", "m_", "v_"))


def assert_densified(what, got, want, n_copied):
    """got / want: (model, exp_avg, exp_avg_sq) dicts name -> [P_new, w]. Rows below n_copied are kept
    originals and clones: exact copies. Child rows are exact too, except xyz and scaling (fp32
    arithmetic: RTOL / ATOL). The Adam state is a copy or zero: exact everywhere."""
    for which, g, w in zip(("param", "exp_avg", "exp_avg_sq"), got, want):
        assert list(g) == list(w), what
        for n in g:
            a, b = np.asarray(g[n]), np.asarray(w[n])
            assert a.shape == b.shape, f"{what}: {which} {n} {a.shape} != {b.shape}"
            if which == "param" and n in ("xyz", "scaling"):
                np.testing.assert_array_equal(a[:n_copied], b[:n_copied], err_msg=f"{what}: copied {n}")
                np.testing.assert_allclose(a[n_copied:], b[n_copied:], rtol=RTOL, atol=ATOL, err_msg=f"{what}: child {n}")
            else:
                np.testing.assert_array_equal(a, b, err_msg=f"{what}: {which} {n}")
