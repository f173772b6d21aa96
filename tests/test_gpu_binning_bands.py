"""The binning (preprocess.hip) at every tile-count band and Gaussian-range edge its host code and kernels
branch on: tests/_binning_cases.py builds the scenes and mirrors the plan, tests/test_binning_plan.py checks
on the CPU that every scene reaches the branch it is named for.

Reference: the oracle's preprocess + duplicateWithKeys + stable sort (_keys_vs_oracle); sorted keys, point
list and ranges are compared bit for bit -- the binning is integer work and its result is unique, so there is
no tolerance anywhere. Each case runs under the scatter variants it lists (the default two-pass scatter,
test_bin_one_pass, test_bin_atomic) and asserts through the plan mirror that it lands in its band. The tile
order is not exposed by rasterizer_state; its consumers check it: the backward on the rows reduction must give
the same bits with the LDS path's order (tile_order_block) and the atomic path's (tile_ranges_kernel).
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import _binning_cases as bc
from tests._helpers import hip_backward, hip_forward, lib_options, rows_reduction, upstream_grads
from tests.test_gpu_parity import _keys_vs_oracle, _oracle_fwd, grad_check

pytestmark = pytest.mark.gpu


def _state(h, c):
    import relightable3dgaussian_amd as r

    st = r._C.rasterizer_state(h["geom"], h["binning"], h["image"], c.scene.P, c.cam.height, c.cam.width,
                               h["num_rendered"])
    return [t.cpu().numpy() for t in st[:3]]  # sorted keys, point list, ranges


def _forward(hip_ext, name, variant):
    c = bc.case(name)
    pl = bc.in_band(name, variant)
    with lib_options(**c.options, **bc.VARIANTS[variant]):
        h = hip_forward(hip_ext, c.scene, c.cam, S=c.S)
    L = _keys_vs_oracle(hip_ext, c.scene, c.cam, h)
    print(f"{name} / {variant}: {pl.T} tiles, {c.scene.P} Gaussians, {L} instances, {pl}")
    assert L == h["num_rendered"] and L >= c.expect.get("min_L", 1)
    return c, h


def _pairs(names):
    return [pytest.param(n, v, id=f"{n}-{v}") for n in names for v in bc.variants_of(n)]


@pytest.mark.parametrize("name,variant", _pairs(bc.BAND_NAMES))
def test_tile_count_bands(hip_ext, name, variant):
    """A: the frames either side of every tile-count boundary (tile_ranges_kernel<8|40|0>, dynamic LDS at and
    above 64 KiB, the last LDS frame and the first atomic-fallback frame), 60 000 Gaussians, forward only."""
    _, h = _forward(hip_ext, name, variant)
    assert h["num_rendered"] > 100_000


def test_last_lds_frame_atomic_identical(hip_ext):
    """4096x2304, kBinMaxTiles tiles: the LDS path at its last frame and the atomic path give the same bits."""
    name = "band-4096x2304"
    c, a = _forward(hip_ext, name, "two_pass")
    sa = _state(a, c)
    ia = {k: a[k].cpu().numpy() for k in ("color", "opacity", "depth", "feature", "n_contrib")}
    del a
    _, b = _forward(hip_ext, name, "atomic")
    for x, y, k in zip(sa, _state(b, c), ("keys", "point list", "ranges")):
        np.testing.assert_array_equal(x, y, err_msg=k)
    for k, x in ia.items():
        np.testing.assert_array_equal(x, b[k].cpu().numpy(), err_msg=k)


@pytest.mark.parametrize("name,variant", _pairs(bc.B_NAMES))
def test_small_tile_counts(hip_ext, name, variant):
    """B: frames 16 px high of 1 .. 129 tiles (partial and exact last bucket and column-scan block, the
    padded launch grid), empty buckets, buckets staging 2500 pairs, a tile of LONG_TILE instances."""
    _forward(hip_ext, name, variant)


@pytest.mark.parametrize("name,variant", _pairs(bc.C_NAMES))
def test_gaussian_ranges(hip_ext, name, variant):
    """C: bin_enumerate and the split of the Gaussians over sub-ranges and workgroups: counts either side of
    kBinSub, culled runs, sub-ranges of 0 / 1 / few instances, a rect over the whole grid, clipped rects, and
    the column scan's wave-row split at 1 .. 59 workgroups."""
    _forward(hip_ext, name, variant)


@rows_reduction()
@pytest.mark.parametrize("name", ["long_tile", "tiles-15"])
def test_tile_order_consumers(hip_ext, name):
    """D: the backward (longest tiles first) with the LDS path's order and with the atomic path's: bit-identical
    gradients on the rows reduction. long_tile: a tile in the order's last, capped bucket; tiles-15: a padded
    launch grid (15 tiles on 16 slots). tiles-15 also against the oracle's backward at grad_check's bar."""
    c = bc.case(name)
    dc, do, dd, df = upstream_grads(c.cam.height, c.cam.width, c.S, seed=7)
    g = {}
    for variant in ("two_pass", "atomic"):
        _, h = _forward(hip_ext, name, variant)
        with lib_options(**bc.VARIANTS[variant]):
            g[variant] = hip_backward(hip_ext, h, dc, do, dd, df)
    for k in g["two_pass"]:
        np.testing.assert_array_equal(g["two_pass"][k], g["atomic"][k], err_msg=k)
    assert any(np.abs(v).max() > 0 for v in g["two_pass"].values())
    if name == "tiles-15":
        import oracle

        o = _oracle_fwd(c.scene, c.cam, c.S)
        grad_check(f"binning {name}", g["two_pass"], oracle.rasterize_backward(o, dc, do, dd, df))
