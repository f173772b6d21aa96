"""The backward blend's per-visit record fetch (render_bwd.hip, the `while (bits)` pair loop) on the shapes
where an instance-indexed fetch can go wrong, against the C oracle (never HIP against HIP).

One 16 x 16 image = one tile = one workgroup, four 8 x 8 quadrants = four waves; a batch is 64 instances.
  low-N    N instances stacked on the tile centre, N in {1, 2, 63, 64, 65, 127, 128, 129}, opacities so low
           that every pixel blends all N: every wave visits every instance -- the batch tail (cnt < 64, lanes
           past the batch), exact batch boundaries, the double buffer (batch b's records against batch b + 1's
           DMA), odd and even visit counts (the last pair's j1 = j0).
  high-N   the same stacks with opacities at which every pixel saturates before the range ends: batches are
           counted from max n_contrib, not from the range end (from 127 on, still more than one batch).
  quadrants  136 small Gaussians, each inside one quadrant (6 / 70 / 40 / 20 of them), the first quadrant's
           nearest: the visit masks differ per wave, and a wave's trimming of the instances behind its own
           last contributor (lo = hi - wmax) takes whole batches from one wave and part of a batch from others.
Each scene's coverage is asserted on the oracle's forward (CPU test below, and again before every GPU
comparison), so a scene that stops exercising its case fails loudly.

Written for the lane-held batch records (lane l keeps instance l's record, a visit takes it by v_readlane at its
instance index), which passed these tests and measured slower; the tests stay for whatever
replaces the fetch next. They run each scene on both reductions (rows twice, bit-identical) and on every SMAX
instantiation launch_bwd_s dispatches.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import oracle
from relightable3dgaussian_amd import synthetic
from tests._helpers import hip_backward, hip_forward, lib_options, upstream_grads
from tests.test_gpu_parity import GRAD_BARS, _check_forward, grad_check

W = H = 16
NB = 64  # instances per staged batch (render_bwd.hip kBwdNB)
STACK_N = [1, 2, 63, 64, 65, 127, 128, 129]
QUAD_COUNTS = (6, 70, 40, 20)
NAMES = [f"low-{n}" for n in STACK_N] + [f"high-{n}" for n in STACK_N] + ["quadrants"]
S_MAIN = [0, 11, 12]            # SMAX 0, the flagship's 11 (no pad channel), 12
S_REST = [3, 6, 16, 21, 32]     # launch_bwd_s's other instantiations (SMAX 4, 8, 16, 24, 32)
CASES = [(n, s) for n in NAMES for s in S_MAIN] + [(n, s) for n in ("low-129", "quadrants") for s in S_REST]


def _camera():
    """At the origin, looking down +z: pixel u <-> x = (u - 7.5) / fx * z. A 4 degree field of view (fx = 229 px),
    so that a splat with a screen sigma of 8 px is 0.035 z across, as trained splats are: at m1_camera's 60
    degrees on 16 px it would be 0.9 z, and the projection's Jacobian terms in dL_dmeans3D cancel to 1e-5 of
    themselves (the oracle's own f32 rounding then exceeds GRAD_BARS; test_scene_is_well_conditioned)."""
    fov = math.radians(4.0)
    return synthetic.make_camera(np.eye(3), np.zeros(3), fov, fov, W, H)


def _scene(u, v, z, sigma_px, opacity, seed):
    cam = _camera()
    fx, fy = cam.focal
    P = len(z)
    rng = np.random.default_rng(seed)
    means = np.stack([(u - (W - 1) / 2) / fx * z, (v - (H - 1) / 2) / fy * z, z], 1)
    scales = np.repeat((sigma_px * z / fx)[:, None], 3, 1)
    q = rng.normal(size=(P, 4))
    sh = np.empty((P, 16, 3))
    sh[:, 0] = (rng.uniform(0, 1, (P, 3)) - 0.5) / 0.28209479
    sh[:, 1:] = rng.normal(0, 0.1, (P, 15, 3))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return synthetic.Scene(f32(means), f32(scales), f32(q / np.linalg.norm(q, axis=1, keepdims=True)),
                           f32(opacity).reshape(P, 1), f32(sh), f32(rng.uniform(0, 1, (P, 32)))), cam


@functools.lru_cache(maxsize=None)
def scene(name):
    kind, _, arg = name.partition("-")
    if kind == "quadrants":
        rng = np.random.default_rng(500)
        quad = np.repeat(np.arange(4), QUAD_COUNTS)
        P = len(quad)
        u = 3.5 + 8 * (quad & 1) + rng.uniform(-1, 1, P)
        v = 3.5 + 8 * (quad >> 1) + rng.uniform(-1, 1, P)
        # depth: quadrant 0's few instances nearest, quadrant 3's within the nearer part of the range
        key = np.where(quad == 0, rng.uniform(0.0, 0.04, P),
                       np.where(quad == 3, rng.uniform(0.05, 0.4, P), rng.uniform(0.05, 1.0, P)))
        return _scene(u, v, 3.0 + key, rng.uniform(0.8, 1.2, P), rng.uniform(0.02, 0.05, P), 501)
    N = int(arg)
    rng = np.random.default_rng(100 + N + (1000 if kind == "high" else 0))
    u, v = 7.5 + rng.uniform(-1.5, 1.5, N), 7.5 + rng.uniform(-1.5, 1.5, N)
    z = 3.0 + 0.02 * np.arange(N) + rng.uniform(0, 0.01, N)
    sigma = rng.uniform(7.5, 9, N)  # G on the corner pixels ~ 0.44, no lower than ~0.24
    if kind == "low":
        # alpha >= 0.02 * 0.24 > 1 / 255 on every pixel; (1 - 0.03)^129 = 0.02: T stays far above the 1e-4 stop
        op = rng.uniform(0.02, 0.03, N)
    else:
        # T < 1e-4 after about 0.7 N instances on the faintest pixel (coverage asserted below)
        a = 1.0 - np.exp(np.log(1e-4) / max(0.68 * N, 1.0))
        op = np.minimum(a / 0.44, 0.9) * rng.uniform(0.95, 1.05, N)
    return _scene(u, v, z, sigma, op, 200 + N)


@functools.lru_cache(maxsize=None)
def oracle_run(name, S):
    """(forward, upstream gradients, backward) of the oracle: shared, read-only."""
    sc, cam = scene(name)
    o = oracle.rasterize_forward(cam, sc.means3D, sc.opacity, sc.features[:, :S], sh=sc.sh, scales=sc.scales,
                                 rotations=sc.rotations)
    up = upstream(S)
    return o, up, oracle.rasterize_backward(o, *up)


def upstream(S):
    """Upstream gradients of one sign per channel (signs alternating over the channels), magnitudes 0.5e-3 +
    |N(0, 1e-3)| per pixel. These stacks are 127 alike splats of 256 pixels each: under white-noise upstream
    gradients (tests/_helpers.py upstream_grads as it stands) a splat's colour / feature / depth sums cancel to
    ~1/16 of their terms, and the backward's documented 16-bit w = alpha T (two bf16 terms, 2^-16 per product,
    render_bwd.hip kBwdSplit) then shows at ~2e-4 of the sum -- outside GRAD_BARS' 1e-4 with no kernel at
    fault. test_scene_is_well_conditioned asserts from the oracle that 2^-16 of each sum's absolute terms lies
    within half the bar."""
    dc, do, dd, df = upstream_grads(H, W, S, seed=7)
    sign = lambda n: np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)[:, None, None]  # noqa: E731
    pos = lambda a: np.abs(a) + np.float32(0.5e-3)  # noqa: E731
    return pos(dc) * sign(3), pos(do), -pos(dd), pos(df) * sign(S) if S else df


def quadrant_hits(o):
    """[instance of the tile in sorted order, quadrant]: some pixel of the quadrant blends it (float64)."""
    a, b = (int(x) for x in o["ranges"][0])
    ids = o["point_list"][a:b].astype(np.int64)
    co = o["conic_opacity"][ids].astype(np.float64)
    xy = o["means2D"][ids].astype(np.float64)
    py, px = np.mgrid[0:H, 0:W]
    dx = xy[:, 0, None, None] - px
    dy = xy[:, 1, None, None] - py
    power = -0.5 * (co[:, 0, None, None] * dx * dx + co[:, 2, None, None] * dy * dy) - co[:, 1, None, None] * dx * dy
    hit = (power <= 0) & (np.minimum(0.99, co[:, 3, None, None] * np.exp(power)) >= 1.0 / 255.0)
    return np.stack([hit[:, 8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8].any((1, 2))
                     for q in range(4)], 1)


def covers(name, o):
    kind, _, arg = name.partition("-")
    sc, _ = scene(name)
    assert o["ranges"].shape[0] == 1 and int(o["ranges"][0][1]) - int(o["ranges"][0][0]) == sc.P, o["ranges"]
    nc = np.asarray(o["n_contrib"]).reshape(H, W).astype(np.int64)
    hits = quadrant_hits(o)
    wmax = np.array([nc[8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8].max() for q in range(4)])
    max_last = int(nc.max())
    print(f"{name}: {sc.P} instances, n_contrib {int(nc.min())}..{max_last}, per quadrant {wmax.tolist()}, "
          f"visits per quadrant {hits.sum(0).tolist()}")
    if kind == "low":
        assert hits.all(), hits.sum(0)             # every wave visits every instance
        assert int(nc.min()) == sc.P, nc.min()     # and no pixel stops early
    elif kind == "high":
        N = int(arg)
        if N >= 63:
            assert max_last < N, (max_last, N)     # batches counted from max n_contrib, not the range end
            assert int(nc.min()) >= 8, nc.min()
        if N >= 127:
            assert max_last > NB, max_last         # and still more than one batch
    else:
        assert (hits.sum(1) == 1).all(), hits.sum(1)
        assert sorted(hits.sum(0).tolist()) == sorted(QUAD_COUNTS), hits.sum(0)
        assert len(set(wmax.tolist())) == 4 and max_last > 2 * NB, wmax
        lo = [hi - wq for hi in range(max_last, 0, -NB) for wq in wmax]  # per (batch, wave)
        assert any(x >= NB for x in lo) and any(0 < x < NB for x in lo) and any(x <= 0 for x in lo), lo


@pytest.mark.parametrize("name", NAMES)
def test_scene_covers_its_case(name):
    """CPU: the oracle alone meets each scene's coverage assertions."""
    covers(name, oracle_run(name, 11)[0])


@pytest.mark.parametrize("name", NAMES)
def test_scene_is_well_conditioned(name):
    """CPU: on each scene two float32 evaluations of the backward -- the oracle and tests/ref64.py's restatement
    run in float32 -- each lie within half of GRAD_BARS of the float64 restatement. A third float32 evaluation
    that is as accurate (the HIP path: the same operations summed in another order) then lies within the full
    bar of the oracle, so the bars pin the kernel on these scenes and not the scenes' own cancellation. (At
    m1_camera's 60 degrees the oracle's dL_dmeans3D missed this by 20x.)"""
    import torch

    from tests import _edge_scenes as es
    from tests import ref64
    from tests import test_ref64 as t64

    sc, cam = scene(name)
    c = es.Case(name, sc, cam, 11)
    o, up, go = oracle_run(name, 11)
    near = ref64.tile_blend(**t64._blend_inputs(c, o))["near"]
    assert near.mean() <= 0.01, near.mean()
    if near.any():  # a pair within 1e-5 of a skip threshold: left out on both sides, as in test_ref64
        keep = (~near).astype(np.float32)
        up = (up[0] * keep[None], up[1] * keep.reshape(-1), up[2] * keep.reshape(-1), up[3] * keep[None])
        go = oracle.rasterize_backward(o, *up)
    b64 = ref64.tile_blend(**t64._blend_inputs(c, o), upstream=up)
    b32 = ref64.tile_blend(**t64._blend_inputs(c, o), upstream=up, dtype=torch.float32)
    g64 = ref64.per_gaussian_backward(**t64._gauss_inputs(c, o, go))
    g32 = ref64.per_gaussian_backward(**t64._gauss_inputs(c, o, go), dtype=torch.float32)
    worst = {}
    for keys, r32, r64 in ((t64.BLEND_KEYS, b32, b64), (t64.GAUSS_KEYS, g32, g64)):
        for k in keys:
            if np.any(r64[k]) or np.any(go[k]):
                worst[k] = (t64.excess(r32[k], r64[k], t64.CAPS[k]), t64.excess(go[k], r64[k], t64.CAPS[k]))
    # the w-derived sums (colours, features, the depth term in dL_dmeans2D[:, 2]) at 16 significant bits of w:
    # 2^-16 of the sums of their absolute terms (w >= 0: the oracle's backward of the absolute upstream)
    ga = oracle.rasterize_backward(o, *(np.abs(a) for a in up))
    for k, got, ref in (("dL_dcolors", ga["dL_dcolors"], go["dL_dcolors"]),
                        ("dL_dfeatures", ga["dL_dfeatures"], go["dL_dfeatures"]),
                        ("dL_dmeans2D", ga["dL_dmeans2D"][:, 2], go["dL_dmeans2D"][:, 2])):
        rel, frac = GRAD_BARS[k]
        bar = rel * np.abs(ref) + frac * float(np.abs(go[k]).max())
        split = float((2.0 ** -16 * np.abs(got) / bar).max())
        print(f"{name}: {k} 2^-16 of the absolute terms / bar {split:.2f}")
        assert split <= 0.5, (k, split)
    print(f"{name}: worst |d| / GRAD_BARS against float64 (float32 restatement, oracle): "
          + ", ".join(f"{k} {a:.2f} {b:.2f}" for k, (a, b) in worst.items()))
    assert all(max(v) <= 0.5 for v in worst.values()), worst


@pytest.mark.gpu
@pytest.mark.parametrize("reduce", ["atomic", "rows"])
@pytest.mark.parametrize("name,S", CASES)
def test_backward_matches_oracle(hip_ext, name, S, reduce):
    sc, cam = scene(name)
    o, up, go = oracle_run(name, S)
    covers(name, o)
    with lib_options(bwd_reduce=int(reduce == "rows")):
        h = hip_forward(hip_ext, sc, cam, S=S)
        _check_forward(h, o, S)  # n_contrib and final_T bit-exact: the backward replays the same lists
        gh = hip_backward(hip_ext, h, *up)
        if reduce == "rows":  # the deterministic reduction: bitwise the same run to run
            g2 = hip_backward(hip_ext, h, *up)
            for k in gh:
                np.testing.assert_array_equal(gh[k], g2[k], err_msg=k)
    grad_check(f"{name} S={S} {reduce}", gh, go)
