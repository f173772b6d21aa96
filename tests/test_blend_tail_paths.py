"""The blend loops' two bodies -- the pair of live instances and the one-visit tail an odd live count ends on
(render_fwd.hip, render_bwd.hip: `while (j1 >= 0)` and the `if (j0 >= 0)` after it) -- against the C oracle,
forward and backward (never HIP against HIP).

One 16 x 16 image = one tile = one workgroup, four 8 x 8 quadrants = four waves, 64 instances per staged batch
(the scene and camera helpers of tests/test_bwd_lane_records.py). A wave walks the live instances of a batch two
at a time; a batch whose live count is odd ends on the tail body.
  low-N    N in {1, 2, 3, 63, 64, 65, 127, 128, 129} stacked on the tile centre at opacities so low that every
           wave visits all N: a tail after 0, 1 and 31 pairs, no tail at 2 / 64 / 128, a tail of one instance
           alone in its batch right after one and two full batches (65, 129).
  quads    136 small Gaussians, each inside one quadrant (5 / 70 / 41 / 20 of them), depths interleaved: in one
           batch some waves end on the tail body while their neighbours end on a pair.
  sat-*    62 or 63 faint fillers centred on quadrant 0 and one opaque Gaussian: every pixel of wave 0 stops at
           the opaque instance while pixels of the other waves go on (the workgroup stays, wave 0 leaves):
           sat-first   the opaque instance is the first of wave 0's last pair of batch 0,
           sat-second  the second of that pair,
           sat-tail    wave 0's one-visit tail of batch 0 (one more small Gaussian in quadrant 3 makes wave 0's
                       live count 63); nine more instances follow in batch 1 in each.
Each scene's case is asserted on the oracle's forward (CPU test below, and again before every GPU comparison):
the live count per wave and batch and its parity, in the forward's batches (from the range start) and in the
backward's (back from the largest n_contrib), and the position at which wave 0 saturates. The forward visits
the instances its quadrant cull keeps, a superset of those a pixel blends: the coverage also asserts that every
(instance, quadrant) pair that no pixel blends lies far outside the cull's margin (alpha at the quadrant's nearest
point below half the 1/255 threshold), so that both lists are the same.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle
from tests._helpers import hip_backward, hip_forward, lib_options
from tests.test_bwd_lane_records import NB, H, W, _scene, covers as stack_covers, quadrant_hits, upstream
from tests.test_bwd_lane_records import scene as stack_scene
from tests.test_gpu_parity import _check_forward, grad_check

STACK_N = [1, 2, 3, 63, 64, 65, 127, 128, 129]
QUAD_COUNTS = (5, 70, 41, 20)
SAT = {"sat-first": (False, 62), "sat-second": (False, 63), "sat-tail": (True, 63)}  # small one?, opaque position
SAT_N = 73
NAMES = [f"low-{n}" for n in STACK_N] + ["quads"] + list(SAT)
S_MAIN = [0, 11, 12]            # SMAX 0, the flagship's 11 (no pad channel), 12
S_REST = [3, 6, 16, 21, 32]     # the other instantiations (SMAX 4, 8, 16, 24, 32)
CASES = [(n, s) for n in NAMES for s in S_MAIN] + [(n, s) for n in ("low-129", "quads") for s in S_REST]


@functools.lru_cache(maxsize=None)
def scene(name):
    if name.startswith("low-"):
        return stack_scene(name)
    if name == "quads":
        rng = np.random.default_rng(900)
        quad = np.repeat(np.arange(4), QUAD_COUNTS)
        P = len(quad)
        u = 3.5 + 8 * (quad & 1) + rng.uniform(-1, 1, P)
        v = 3.5 + 8 * (quad >> 1) + rng.uniform(-1, 1, P)
        return _scene(u, v, 3.0 + rng.uniform(0.0, 1.0, P), rng.uniform(0.8, 1.2, P), rng.uniform(0.02, 0.05, P), 901)
    small, kpos = SAT[name]
    # fillers on quadrant 0's centre, sigma 8 px, opacity 0.1: after 62 of them T is 1.5e-3 on the centre and
    # 4.8e-3 on the quadrant's corners (no stop: T (1 - alpha) stays above 1e-4), and above 0.2 at pixel (15, 15).
    # The opaque one (opacity 1, sigma 40 px: G >= 0.992 on quadrant 0, alpha clamps to 0.99) then takes every
    # pixel of quadrant 0 below 1e-4 -- they stop -- and leaves pixel (15, 15) at 2e-3: the workgroup goes on
    u, v = np.full(SAT_N, 3.5), np.full(SAT_N, 3.5)
    sigma, op = np.full(SAT_N, 8.0), np.full(SAT_N, 0.1)
    rng = np.random.default_rng(950 + kpos + small)
    u += rng.uniform(-0.2, 0.2, SAT_N)
    v += rng.uniform(-0.2, 0.2, SAT_N)
    op *= rng.uniform(0.97, 1.03, SAT_N)
    sigma[kpos], op[kpos] = 40.0, 1.0
    if small:  # nearest, inside quadrant 3 alone
        u[0], v[0], sigma[0], op[0] = 11.5, 11.5, 1.0, 0.04
    z = 3.0 + 0.02 * np.arange(SAT_N) + rng.uniform(0, 0.01, SAT_N)
    return _scene(u, v, z, sigma, op, 951)


@functools.lru_cache(maxsize=None)
def oracle_run(name, S):
    """(forward, upstream gradients, backward) of the oracle: shared, read-only."""
    sc, cam = scene(name)
    o = oracle.rasterize_forward(cam, sc.means3D, sc.opacity, sc.features[:, :S], sh=sc.sh, scales=sc.scales,
                                 rotations=sc.rotations)
    up = upstream(S)
    return o, up, oracle.rasterize_backward(o, *up)


def cull_is_clear(o, hits):
    """Every (instance, quadrant) pair without a blending pixel: alpha at the point of the quadrant's pixel
    rectangle nearest the mean (float64) is below half the 1/255 threshold."""
    a, b = (int(x) for x in o["ranges"][0])
    ids = o["point_list"][a:b].astype(np.int64)
    co = o["conic_opacity"][ids].astype(np.float64)
    xy = o["means2D"][ids].astype(np.float64)
    for q in range(4):
        x0, y0 = 8.0 * (q & 1), 8.0 * (q >> 1)
        dx = xy[:, 0] - np.clip(xy[:, 0], x0, x0 + 7.0)
        dy = xy[:, 1] - np.clip(xy[:, 1], y0, y0 + 7.0)
        power = -0.5 * (co[:, 0] * dx * dx + co[:, 2] * dy * dy) - co[:, 1] * dx * dy
        alpha = co[:, 3] * np.exp(power)
        miss = ~hits[:, q]
        assert (alpha[miss] < 0.5 / 255.0).all(), (q, alpha[miss].max())


def batch_counts(live, edges):
    """[batch, quadrant]: live instances of each wave in each batch [a, b) of sorted positions."""
    return np.array([[int(live[a:b, q].sum()) for q in range(4)] for a, b in edges])


def covers(name, o):
    if name.startswith("low-"):
        stack_covers(name, o)   # every wave visits all N and no pixel stops early
    sc, _ = scene(name)
    N = sc.P
    assert o["ranges"].shape[0] == 1 and int(o["ranges"][0][1]) - int(o["ranges"][0][0]) == N, o["ranges"]
    nc = np.asarray(o["n_contrib"]).reshape(H, W).astype(np.int64)
    quad_nc = [nc[8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8] for q in range(4)]
    wmax = np.array([int(x.max()) for x in quad_nc])
    max_last = int(nc.max())
    hits = quadrant_hits(o)
    cull_is_clear(o, hits)
    fwd_edges = [(k, min(k + NB, N)) for k in range(0, N, NB)]
    bwd_edges = [(max(hi - NB, 0), hi) for hi in range(max_last, 0, -NB)]
    # the forward walks a wave's culled instances until all its pixels stopped; the backward those a pixel of
    # the wave blended (positions below the wave's largest n_contrib)
    blended = hits & (np.arange(N)[:, None] < wmax[None, :])
    fc, bc = batch_counts(hits, fwd_edges), batch_counts(blended, bwd_edges)
    print(f"{name}: {N} instances, n_contrib per quadrant {wmax.tolist()}, live per (batch, wave): forward "
          f"{fc.tolist()}, backward {bc.tolist()}")
    if name.startswith("low-"):
        n = int(name[4:])
        want = [NB] * (n // NB) + ([n % NB] if n % NB else [])
        assert (fc == np.array(want)[:, None]).all(), fc
        assert (bc == np.array(want)[:, None]).all(), bc   # (the backward's short batch comes last, too)
    elif name == "quads":
        assert (hits.sum(1) == 1).all(), hits.sum(1)
        assert hits.sum(0).tolist() == list(QUAD_COUNTS), hits.sum(0)
        # low opacity: no wave stops early (its largest n_contrib is its last instance's position + 1)
        assert max_last == N and all(wmax[q] == np.flatnonzero(hits[:, q]).max() + 1 for q in range(4)), wmax
        for c in (fc, bc):  # in one batch: a wave on the tail body, another ending on a pair
            assert any((row % 2 == 1).any() and ((row % 2 == 0) & (row >= 2)).any() for row in c), c
        assert (fc % 2 == 1).any(0).sum() >= 2 and (bc % 2 == 1).any(0).sum() >= 2, (fc, bc)
    else:
        small, kpos = SAT[name]
        assert hits[int(small):, 0].all() and (not small or not hits[0, 0]), hits[:, 0]
        # every pixel of wave 0 accumulates the instance before the opaque one and stops at the opaque one
        assert (quad_nc[0] == kpos).all(), quad_nc[0]
        assert max_last == N and min(wmax[1:]) == N, wmax   # the other waves, and so the workgroup, go on
        idx = kpos - int(small)                             # the opaque instance in wave 0's live list of batch 0
        live0 = NB - int(small)
        assert fc[0, 0] == live0 and len(fwd_edges) == 2, fc
        if name == "sat-tail":
            assert live0 % 2 == 1 and idx == live0 - 1      # the one-visit tail
        elif name == "sat-first":
            assert live0 % 2 == 0 and idx % 2 == 0 and idx + 1 < live0
        else:
            assert live0 % 2 == 0 and idx % 2 == 1 and idx == live0 - 1


@pytest.mark.parametrize("name", NAMES)
def test_scene_covers_its_case(name):
    """CPU: the oracle alone meets each scene's coverage assertions."""
    covers(name, oracle_run(name, 11)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("reduce", ["atomic", "rows"])
@pytest.mark.parametrize("name,S", CASES)
def test_blend_matches_oracle(hip_ext, name, S, reduce):
    sc, cam = scene(name)
    o, up, go = oracle_run(name, S)
    covers(name, o)
    with lib_options(bwd_reduce=int(reduce == "rows")):
        h = hip_forward(hip_ext, sc, cam, S=S)
        _check_forward(h, o, S)  # n_contrib and final_T bit-exact, the images within the forward's bars
        gh = hip_backward(hip_ext, h, *up)
        if reduce == "rows":  # the deterministic reduction: bitwise the same run to run
            g2 = hip_backward(hip_ext, h, *up)
            for k in gh:
                np.testing.assert_array_equal(gh[k], g2[k], err_msg=k)
    grad_check(f"{name} S={S} {reduce}", gh, go)
