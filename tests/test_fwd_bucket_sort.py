"""The forward blend's fused per-tile depth sort (r3dg_tilesort.h sort_tile_bucket): a one-pass bucket
sort with an exact rank fix-up, falling back to the radix sort when every depth is equal or a
bucket exceeds its cap.

Scenes: the M1 camera model (origin, identity rotation: the depth key is the float bits of z) at a
32x32 frame, n tiny Gaussians (projected radius 3 px, so tiles_touched = 1) on the centre pixel of one
tile, so that tile's list length is exactly n and its depth pattern is the z array given. Keys, point
list and ranges are compared bit for bit with the oracle's stable sort, n_contrib and final_T with
the oracle's blend. Every case also models the bucket occupancy in numpy with the kernel's constants
and asserts which path (fix-up or fallback) its input takes.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from relightable3dgaussian_amd import synthetic
from tests._helpers import hip_forward
from tests.test_gpu_parity import _final_T, _keys_vs_oracle, _oracle_fwd

pytestmark = pytest.mark.gpu

# mirror relightable3dgaussian_amd/csrc/r3dg_tilesort.h (kBktN, kBktCap) and r3dg_kernels.h (kFusedSortMax)
NBKT = 1024
CAP = 16
FUSED_MAX = 1024
S = 11  # the flagship's feature count (render_fwd_glds_kernel<11, false>)


def _bits(z):
    return np.asarray(z, np.float32).view(np.uint32).astype(np.int64)


def _path(z):
    """(path, shift, fullest bucket) of one tile's depths, by sort_tile_bucket's rules."""
    k = _bits(z)
    if k.size > FUSED_MAX:
        return "long", None, None  # tile_depth_sort_kernel, not the fused sort
    if k.size == 0:
        return "empty", None, None
    span = int(k.max() - k.min())
    if span == 0:
        return "fallback-span0", None, None
    shift = max(0, span.bit_length() - (NBKT.bit_length() - 1))
    b = (k - k.min()) >> shift
    assert b.max() < NBKT
    fullest = int(np.bincount(b, minlength=NBKT).max())
    return ("fixup" if fullest <= CAP else "fallback-cap"), shift, fullest


def _scene(cam, tiles, seed):
    """tiles: [(tile x, tile y, z array)]; the Gaussians of all tiles in one random id order."""
    rng = np.random.default_rng(seed)
    fx, fy = cam.focal
    zs, us, vs = [], [], []
    for tx, ty, z in tiles:
        z = np.asarray(z, np.float32)
        zs.append(z)
        us.append(np.full(z.size, 16 * tx + 8.5))  # pixel 16 tx + 8: the Gaussian's centre on a pixel
        vs.append(np.full(z.size, 16 * ty + 8.5))
    z = np.concatenate(zs)
    u, v = np.concatenate(us), np.concatenate(vs)
    perm = rng.permutation(z.size)
    z, u, v = z[perm], u[perm], v[perm]
    P = z.size
    z64 = z.astype(np.float64)
    means = np.stack([(u - cam.cx) / fx * z64, (v - cam.cy) / fy * z64, z64], 1).astype(np.float32)
    assert np.array_equal(means[:, 2], z)
    scales = np.full((P, 3), 1e-4, np.float32)  # far below a pixel: the 0.3 px^2 low-pass floor, radius 3
    rot = np.zeros((P, 4), np.float32)
    rot[:, 0] = 1.0
    opacity = rng.uniform(0.005, 0.012, (P, 1)).astype(np.float32)  # above 1/255, faint: deep blends
    sh = np.empty((P, 16, 3), np.float32)
    sh[:, 0] = (rng.uniform(0, 1, (P, 3)) - 0.5) / 0.28209479
    sh[:, 1:] = rng.normal(0, 0.05, (P, 15, 3))
    feats = rng.uniform(0, 1, (P, S)).astype(np.float32)
    return synthetic.Scene(means, scales, rot, opacity, sh, feats), perm


def _run(hip_ext, cam, tiles, seed=0):
    import relightable3dgaussian_amd as r

    scene, _ = _scene(cam, tiles, seed)
    h = hip_forward(hip_ext, scene, cam, S=S)
    L = sum(len(z) for _, _, z in tiles)
    assert h["num_rendered"] == L  # tiles_touched = 1 for every Gaussian
    if L == 0:
        return
    assert _keys_vs_oracle(hip_ext, scene, cam, h) == L  # keys, point list, ranges: bit for bit
    gx = (cam.width + 15) // 16
    st = r._C.rasterizer_state(h["geom"], h["binning"], h["image"], scene.P, cam.height, cam.width, L)
    keys = st[0].cpu().numpy().view(np.uint64)
    ranges = st[2].cpu().numpy().astype(np.int64)
    for tx, ty, z in tiles:  # the tile's list is exactly the z pattern given: the modelled path is the real one
        lo, hi = ranges[ty * gx + tx]
        assert hi - lo == len(z)
        np.testing.assert_array_equal((keys[lo:hi] & np.uint64(0xffffffff)).astype(np.int64), np.sort(_bits(z)))
    o = _oracle_fwd(scene, cam, S)
    np.testing.assert_array_equal(h["n_contrib"].cpu().numpy(), o["n_contrib"])
    np.testing.assert_array_equal(_final_T(h, cam), o["final_T"])
    for tx, ty, z in tiles:  # the blend went deep into the sorted list
        if len(z) >= 3:
            assert o["n_contrib"].reshape(cam.height, cam.width)[16 * ty + 8, 16 * tx + 8] > len(z) // 3


@pytest.fixture(scope="module")
def cam32():
    return synthetic.m1_camera(32, 32)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 255, 256, 257, 1023, 1024])
def test_list_lengths(hip_ext, cam32, n):
    z = np.random.default_rng(n).uniform(3, 8, n).astype(np.float32)
    path, _, fullest = _path(z)
    print(f"n {n}: {path}, fullest bucket {fullest}")
    assert path == ("fallback-span0" if n == 1 else "fixup")
    _run(hip_ext, cam32, [(0, 0, z)], seed=n)


def test_longer_than_fused_sort(hip_ext, cam32):
    """n = 1025: one past kFusedSortMax, sorted by tile_depth_sort_kernel; still exact."""
    z = np.random.default_rng(7).uniform(3, 8, 1025).astype(np.float32)
    assert _path(z)[0] == "long"
    _run(hip_ext, cam32, [(1, 0, z)], seed=7)


def test_consecutive_ulps(hip_ext, cam32):
    """700 consecutive float values: span 699 < NBKT, shift 0, one item per bucket."""
    z = (np.float32(5.0).view(np.uint32) + np.arange(700, dtype=np.uint32)).view(np.float32)
    path, shift, fullest = _path(z)
    assert (path, shift, fullest) == ("fixup", 0, 1)
    _run(hip_ext, cam32, [(0, 1, z)], seed=1)


def test_ties_in_pairs_and_triples(hip_ext, cam32):
    """Exact depth ties (120 triples + 120 pairs = 600), ids interleaved by the scene's permutation:
    ordered by Gaussian id inside the fix-up, under the cap."""
    d = np.random.default_rng(2).uniform(3, 8, 240).astype(np.float32)
    assert np.unique(d).size == 240
    z = np.concatenate([np.repeat(d[:120], 3), np.repeat(d[120:], 2)])
    assert z.size == 600
    path, _, fullest = _path(z)
    print(f"ties: {path}, fullest bucket {fullest}")
    assert path == "fixup" and fullest >= 3
    _run(hip_ext, cam32, [(1, 1, z)], seed=2)


def test_all_depths_equal(hip_ext, cam32):
    z = np.full(500, 4.25, np.float32)
    assert _path(z)[0] == "fallback-span0"
    _run(hip_ext, cam32, [(0, 0, z)], seed=3)


def test_two_tight_clusters(hip_ext, cam32):
    """Two clusters a few ulps wide at z = 3 and z = 8: two buckets of 450, far above the cap."""
    rng = np.random.default_rng(4)
    lo = (np.float32(3.0).view(np.uint32) + rng.integers(0, 6, 450).astype(np.uint32)).view(np.float32)
    hi = (np.float32(8.0).view(np.uint32) - rng.integers(0, 6, 450).astype(np.uint32)).view(np.float32)
    z = np.concatenate([lo, hi])
    path, _, fullest = _path(z)
    assert path == "fallback-cap" and fullest == 450
    _run(hip_ext, cam32, [(1, 0, z)], seed=4)


def test_dense_bucket_and_sparse_tail(hip_ext, cam32):
    """z = 3 + 5 u^8: hundreds of items in the first buckets, a sparse tail up to 8."""
    u = np.random.default_rng(5).uniform(0, 1, 1000)
    z = (3.0 + 5.0 * u ** 8).astype(np.float32)
    path, _, fullest = _path(z)
    print(f"dense + tail: {path}, fullest bucket {fullest}")
    assert path == "fallback-cap" and fullest > 100
    _run(hip_ext, cam32, [(0, 1, z)], seed=5)


def test_six_tiles(hip_ext):
    """Six tiles of different lengths in a 48x32 frame, one empty, one on each fallback, one longer
    than the fused sort: every tile's list exact, none disturbs another."""
    cam = synthetic.m1_camera(48, 32)
    rng = np.random.default_rng(6)
    zu = lambda n: rng.uniform(3, 8, n).astype(np.float32)  # noqa: E731
    tiles = [(0, 0, zu(0)), (1, 0, zu(1)), (2, 0, zu(130)), (0, 1, zu(1024)),
             (1, 1, np.full(611, 6.5, np.float32)), (2, 1, zu(1300))]
    paths = [_path(z)[0] for _, _, z in tiles]
    assert paths == ["empty", "fallback-span0", "fixup", "fixup", "fallback-span0", "long"]
    _run(hip_ext, cam, tiles, seed=6)
