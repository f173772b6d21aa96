"""Scenes for the binning (preprocess.hip: bin_count / bin_colscan / bin_scatter / bin_bucket / bin_atomic,
tile_ranges_kernel<8|40|0>, tile_order_block) and a Python mirror of the host's plan, shared by the CPU
tests (tests/test_binning_plan.py) and the GPU tests (tests/test_gpu_binning_bands.py).

The plan mirror restates which path a (tiles, Gaussians, options) triple takes; test_binning_plan.py
fails when it differs from the constants of r3dg_kernels.h. Every case carries a `covers` check, evaluated on
the CPU from the oracle's preprocess + duplicateWithKeys and the mirror, that the scene really reaches the
branch it is named for. Seeds may change only to satisfy `covers`, never to fit the kernels.
"""
from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass, field

import numpy as np

from relightable3dgaussian_amd import synthetic

# ------------------------------------------------------------------------------------------------
# the plan mirror (r3dg_kernels.h, preprocess.hip launch_bin_prepare / launch_bin_scatter,
# rasterizer.hip binning_args / stage_binning)
# ------------------------------------------------------------------------------------------------
BIN_BUCKET = 16          # kBinBucket: tiles per bucket of the two-pass scatter
BIN_BUCKET_SHIFT = 28    # kBinBucketShift: the two-pass scatter needs P < 2^28
BIN_SUB = 1024           # kBinSub: Gaussians staged in LDS at a time
BIN_BLOCKS_MAX = 256     # kBinBlocksMax
BIN_MATRIX = 1 << 21     # kBinMatrix: the [nblk, T] count matrix's entries
LDS_CU = 163840          # one CU's LDS: the most static + dynamic LDS a workgroup can have
LDS_DEFAULT = 65536      # above it a launch needs hipFuncAttributeMaxDynamicSharedMemorySize
BIN_MAX_TILES = (LDS_CU - 16 * BIN_SUB) // 4  # kBinMaxTiles
ATOMIC_SUB = 256         # bin_atomic_kernel: Gaussians per workgroup
ORDER_BUCKETS = 1024     # tile_order_block: longest-first buckets of count >> 2, capped

VARIANTS = {"two_pass": {}, "one_pass": dict(test_bin_one_pass=1), "atomic": dict(test_bin_atomic=1)}


def bin_blocks_max(T):
    return 0 if T > BIN_MAX_TILES else max(1, min(BIN_BLOCKS_MAX, BIN_MATRIX // max(T, 1)))


def bin_lds_bytes(T):
    return 4 * (T + 4 * BIN_SUB)


def raises_lds_limit(T):
    """allow_lds: the dynamic-LDS attribute is set only above 64 KiB of dynamic LDS."""
    return bin_lds_bytes(T) > LDS_DEFAULT


@dataclass(frozen=True)
class Plan:
    T: int
    P: int
    lds: bool            # LDS counters (bin_count / bin_colscan / bin_scatter), else bin_atomic_kernel
    nblk: int            # binning workgroups (LDS path)
    two_pass: bool       # scatter through 16-tile buckets + bin_bucket_kernel
    ranges_kernel: int   # tile_ranges_kernel<PER>; -1: none (bin_colscan_kernel writes the ranges)
    lds_bytes: int       # dynamic LDS of bin_count_kernel / bin_scatter_kernel
    lds_attr: bool       # the launch raises the dynamic-LDS limit
    sub: int             # Gaussians per enumerated sub-range


def plan(T, P, test_bin_atomic=0, test_bin_blocks=0, test_bin_one_pass=0):
    lds = bin_blocks_max(T) > 0 and not test_bin_atomic and P > 0
    nb = bin_blocks_max(T)
    if test_bin_blocks > 0:
        nb = min(nb, test_bin_blocks)
    nblk = min(nb, (P + BIN_SUB - 1) // BIN_SUB) if lds else 0
    two_pass = lds and not test_bin_one_pass and P < (1 << BIN_BUCKET_SHIFT)
    ranges = -1 if lds else (8 if T <= 8 * 1024 else 40 if T <= 40 * 1024 else 0)
    return Plan(T, P, lds, nblk, two_pass, ranges, bin_lds_bytes(T) if lds else 0, lds and raises_lds_limit(T),
                BIN_SUB if lds else ATOMIC_SUB)


def colscan_rows(nblk):
    """Rows of the count matrix per wave of bin_colscan_kernel: wave w owns [w nblk / 16, (w + 1) nblk / 16)."""
    return [(w + 1) * nblk // 16 - w * nblk // 16 for w in range(16)]


def block_ranges(P, nblk):
    """bin_range: workgroup b's Gaussians, whole sub-ranges split evenly."""
    nsub = (P + BIN_SUB - 1) // BIN_SUB
    return [(b * nsub // nblk * BIN_SUB, min((b + 1) * nsub // nblk * BIN_SUB, P)) for b in range(nblk)]


def order_bucket(count):
    return min(count >> 2, ORDER_BUCKETS - 1)


# ------------------------------------------------------------------------------------------------
# the oracle's binning of a scene
# ------------------------------------------------------------------------------------------------
def oracle_bins(scene, cam):
    """The oracle's preprocess + duplicateWithKeys (rasterizer_impl.cu:72-116): radii, tiles_touched, the
    Gaussian-major instance list (tile, Gaussian), every visible Gaussian's rect and the tiles' counts."""
    import oracle

    lib = oracle.lib()
    P, F = scene.P, np.float32
    radii = np.zeros(P, np.int32); means2D = np.zeros((P, 2), F); depths = np.zeros(P, F)
    cov3D = np.zeros((P, 6), F); rgb = np.zeros((P, 3), F); cl = np.zeros(P, np.uint8)
    conic = np.zeros((P, 4), F); touched = np.zeros(P, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib.oracle_preprocess(ctypes.c_int(P), ctypes.c_int(3), ctypes.c_int(16), p(scene.means3D), p(scene.scales),
                          ctypes.c_float(1.0), p(scene.rotations), p(scene.opacity.reshape(-1)),
                          p(np.ascontiguousarray(scene.sh)), None, None, p(np.ascontiguousarray(cam.view, F)),
                          p(np.ascontiguousarray(cam.proj, F)), p(np.ascontiguousarray(cam.campos, F)),
                          ctypes.c_int(cam.width), ctypes.c_int(cam.height), ctypes.c_float(cam.tanfovx),
                          ctypes.c_float(cam.tanfovy), p(radii), p(means2D), p(depths), p(cov3D), p(rgb), p(cl),
                          p(conic), p(touched))
    offsets = np.cumsum(touched, dtype=np.uint64).astype(np.uint32)
    L = int(offsets[-1]) if P else 0
    keys = np.zeros(max(L, 1), np.uint64); vals = np.zeros(max(L, 1), np.uint32)
    lib.oracle_duplicate_with_keys(ctypes.c_int(P), p(means2D), p(depths), p(offsets), p(radii),
                                   ctypes.c_int(cam.width), ctypes.c_int(cam.height), p(keys), p(vals))
    gx, gy = (cam.width + 15) // 16, (cam.height + 15) // 16
    tiles = (keys[:L] >> np.uint64(32)).astype(np.int64)
    vis = touched > 0
    end = offsets.astype(np.int64)
    first = tiles[(end - touched)[vis]]
    last = tiles[end[vis] - 1]
    rect = np.zeros((P, 4), np.int64)  # x0, y0, w, h in tiles
    rect[vis] = np.stack([first % gx, first // gx, last % gx - first % gx + 1, last // gx - first // gx + 1], 1)
    assert np.array_equal(rect[:, 2] * rect[:, 3], touched)
    return dict(radii=radii, touched=touched.astype(np.int64), offsets=end, L=L, tiles=tiles, gauss=vals[:L],
                rect=rect, counts=np.bincount(tiles, minlength=gx * gy), gx=gx, gy=gy, T=gx * gy)


def sub_totals(touched, sub=BIN_SUB):
    """Instances of every sub-range of `sub` Gaussians (bin_enumerate's `total`)."""
    n = (len(touched) + sub - 1) // sub
    return [int(touched[i * sub:(i + 1) * sub].sum()) for i in range(n)]


def bucket_totals(counts):
    """Staged pairs of every 16-tile bucket (bin_bucket_kernel's s1 - s0)."""
    n = (len(counts) + BIN_BUCKET - 1) // BIN_BUCKET
    return [int(counts[i * BIN_BUCKET:(i + 1) * BIN_BUCKET].sum()) for i in range(n)]


# ------------------------------------------------------------------------------------------------
# scene builders
# ------------------------------------------------------------------------------------------------
S_SMALL = 11  # the flagship's feature count


def placed(cam, u, v, z, sigma_px, visible=None, seed=0, S=S_SMALL, opacity=(0.05, 0.6), oriented=False):
    """Gaussians whose centres project to the pixels (u, v) of an M1 camera (origin, identity rotation) at
    depth z, with a screen-space sigma of sigma_px (0: far below a pixel, i.e. the 0.3 px^2 low-pass floor and
    radius 3). Isotropic with the identity rotation, or `oriented`: axes of 0.4 .. 1 sigma under a random
    rotation (an isotropic Gaussian's rotation gradient is zero, so nothing to compare a backward's with).
    Gaussians not `visible` lie behind the camera (culled, radius 0)."""
    rng = np.random.default_rng(seed)
    fx, fy = cam.focal
    u, v, z = (np.asarray(a, np.float64) for a in (u, v, z))
    P = z.size
    sig = np.broadcast_to(np.asarray(sigma_px, np.float64), (P,))
    means = np.stack([(u - cam.cx) / fx * z, (v - cam.cy) / fy * z, z], 1)
    if visible is not None:
        means[~np.asarray(visible, bool), 2] *= -1.0
    scales = np.repeat(np.maximum(sig * z / fx, 1e-4)[:, None], 3, 1)
    rot = np.zeros((P, 4), np.float32)
    rot[:, 0] = 1.0
    if oriented:
        scales = scales * rng.uniform(0.4, 1.0, (P, 3))
        q = rng.normal(size=(P, 4))
        rot = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    op = rng.uniform(opacity[0], opacity[1], (P, 1)).astype(np.float32)
    sh = np.empty((P, 16, 3), np.float32)
    sh[:, 0] = (rng.uniform(0, 1, (P, 3)) - 0.5) / 0.28209479
    sh[:, 1:] = rng.normal(0, 0.05, (P, 15, 3))
    feats = rng.uniform(0, 1, (P, S)).astype(np.float32)
    return synthetic.Scene(means.astype(np.float32), scales.astype(np.float32), rot, op, sh, feats)


def on_tiles(cam, tiles, seed, visible=None, opacity=(0.05, 0.6)):
    """One tiny Gaussian (one instance) per entry of `tiles` (row-major tile index), within 2 px of the tile's
    centre, in the order given (the caller shuffles)."""
    rng = np.random.default_rng(seed)
    tiles = np.asarray(tiles, np.int64)
    gx = (cam.width + 15) // 16
    u = 16 * (tiles % gx) + 8.5 + rng.uniform(-2, 2, tiles.size)
    v = 16 * (tiles // gx) + 8.5 + rng.uniform(-2, 2, tiles.size)
    return placed(cam, u, v, rng.uniform(3, 8, tiles.size), 0.0, visible, seed + 1, opacity=opacity)


def fill(cam, P, seed, sigma_px=(0.3, 6.0), margin=8.0, visible=None):
    """P Gaussians over the frame and a margin around it, screen-space sigma log-uniform in sigma_px."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-margin, cam.width + margin, P)
    v = rng.uniform(-margin, cam.height + margin, P)
    sig = np.exp(rng.uniform(np.log(sigma_px[0]), np.log(sigma_px[1]), P))
    return placed(cam, u, v, rng.uniform(3, 8, P), sig, visible, seed + 1, oriented=True)


@dataclass
class Case:
    name: str
    scene: synthetic.Scene
    cam: synthetic.Camera
    S: int
    variants: tuple = ("two_pass", "one_pass", "atomic")
    options: dict = field(default_factory=dict)  # besides the variant's (test_bin_blocks)
    expect: dict = field(default_factory=dict)   # what `covers` asserts

    @property
    def T(self):
        return ((self.cam.width + 15) // 16) * ((self.cam.height + 15) // 16)

    def plan(self, variant):
        return plan(self.T, self.scene.P, **{**self.options, **VARIANTS[variant]})


# A. tile-count bands: (width, height) -> (tiles, variants, the band the default path must land in)
BAND_P = 60_000
BANDS = {
    (2048, 1024): (8192, ("two_pass", "one_pass", "atomic"), dict(lds=True, lds_attr=False, atomic_ranges=8)),
    (2064, 1024): (8256, ("two_pass", "one_pass", "atomic"), dict(lds=True, lds_attr=False, atomic_ranges=40)),
    (2048, 1536): (12288, ("two_pass", "one_pass"), dict(lds=True, lds_attr=False, lds_bytes=65536)),
    (2064, 1536): (12384, ("two_pass", "one_pass"), dict(lds=True, lds_attr=True)),
    (4096, 2240): (35840, ("two_pass", "one_pass"), dict(lds=True, lds_attr=True)),
    (4096, 2304): (36864, ("two_pass", "one_pass", "atomic"), dict(lds=True, lds_attr=True, lds_bytes=LDS_CU,
                                                                  atomic_ranges=40)),
    (4096, 2320): (37120, ("two_pass",), dict(lds=False, ranges_kernel=40)),
    (4096, 2560): (40960, ("two_pass",), dict(lds=False, ranges_kernel=40)),
    (4096, 2576): (41216, ("two_pass",), dict(lds=False, ranges_kernel=0)),
}
BAND_NAMES = [f"band-{w}x{h}" for w, h in BANDS]

# B. small tile counts (frames 16 px high): T -> frame width (some with a partial last tile)
SMALL_T = {1: 16, 15: 235, 16: 256, 17: 261, 63: 1003, 64: 1024, 65: 1035, 129: 2059}
TILES_NAMES = [f"tiles-{t}" for t in SMALL_T]
B_NAMES = TILES_NAMES + ["right_half", "bucket_gap", "one_tile_2500", "bucket_spread_2500", "long_tile"]

# C. bin_enumerate and the Gaussian-range split
COUNTS = [1, 1023, 1024, 1025, 2049, 3000]
COUNT_NAMES = [f"count-{p}" for p in COUNTS]
WAVE_ROW_BLOCKS = [1, 2, 15, 16, 17, 0]  # test_bin_blocks (0: uncapped, 59 workgroups)
WAVE_ROW_NAMES = [f"wave_rows-{k}" for k in WAVE_ROW_BLOCKS]
C_NAMES = COUNT_NAMES + ["cull_first_1024", "cull_middle", "cull_last_1500", "cull_alternate", "only_last",
                         "sparse_subranges", "whole_grid", "rects"] + WAVE_ROW_NAMES

NAMES = BAND_NAMES + B_NAMES + C_NAMES
LONG_TILE = 4200  # >= 4092: the last bucket of the longest-first order (count >> 2 capped at 1023)

# One seed per kind of scene; changed only where `covers` asked for another scene.
SEEDS = {"band": 5, "tiles": 100, "right_half": 41, "bucket_gap": 42, "one_tile_2500": 43, "bucket_spread_2500": 44,
         "long_tile": 45, "count": 50, "cull": 60, "only_last": 61, "sparse_subranges": 62, "whole_grid": 63,
         "rects": 64, "wave_rows": 9}


def _build(name):
    kind, _, arg = name.partition("-")
    if kind == "band":
        w, h = (int(x) for x in arg.split("x"))
        tiles, variants, expect = BANDS[(w, h)]
        cam = synthetic.m1_camera(w, h)
        scene = synthetic.m1_scene(P=BAND_P, S=3, seed=SEEDS[kind], cam=cam)
        return Case(name, scene, cam, 3, variants, expect=dict(expect, T=tiles, min_L=100_001))
    if kind == "tiles":
        T = int(arg)
        # (small_scene's tilted camera culls half of so wide a frame: the M1 camera fills every tile)
        cam = synthetic.m1_camera(SMALL_T[T], 16)
        scene = fill(cam, 3000, SEEDS[kind] + T)
        return Case(name, scene, cam, S_SMALL, expect=dict(T=T, min_L=1500, nblk=3, all_tiles=True))
    rng = np.random.default_rng(SEEDS.get(kind, 0))
    if kind == "right_half":  # 64 tiles: buckets 0 and 1 empty, 2 and 3 full
        cam = synthetic.m1_camera(1024, 16)
        return Case(name, on_tiles(cam, rng.integers(32, 64, 3000), SEEDS[kind]), cam, S_SMALL,
                    expect=dict(T=64, empty_buckets=[0, 1], full_buckets=[2, 3]))
    if kind == "bucket_gap":  # 80 tiles: bucket 1 empty between full ones, bucket 3 too
        cam = synthetic.m1_camera(1280, 16)
        tiles = np.concatenate([rng.integers(0, 16, 1200), rng.integers(32, 48, 900), rng.integers(64, 80, 900)])
        return Case(name, on_tiles(cam, rng.permutation(tiles), SEEDS[kind]), cam, S_SMALL,
                    expect=dict(T=80, empty_buckets=[1, 3], full_buckets=[0, 2, 4]))
    if kind == "one_tile_2500":  # bucket 1 stages 2500 pairs, all of tile 21
        cam = synthetic.m1_camera(512, 16)
        tiles = np.concatenate([np.full(2500, 21), rng.integers(0, 16, 200)])
        return Case(name, on_tiles(cam, rng.permutation(tiles), SEEDS[kind], opacity=(0.005, 0.012)), cam, S_SMALL,
                    expect=dict(T=32, bucket=(1, 2500), longest=2500))
    if kind == "bucket_spread_2500":  # bucket 1 stages 2500 pairs over its 16 tiles
        cam = synthetic.m1_camera(512, 16)
        tiles = np.concatenate([rng.integers(16, 32, 2500), rng.integers(0, 16, 200)])
        return Case(name, on_tiles(cam, rng.permutation(tiles), SEEDS[kind]), cam, S_SMALL,
                    expect=dict(T=32, bucket=(1, 2500), all_tiles=True, max_longest=400))
    if kind == "long_tile":  # 17 tiles; tile 9 holds LONG_TILE instances, tile i of the others 3 i + 1
        cam = synthetic.m1_camera(272, 16)
        tiles = np.concatenate([np.full(LONG_TILE, 9)] + [np.full(3 * i + 1, i) for i in range(17) if i != 9])
        return Case(name, on_tiles(cam, rng.permutation(tiles), SEEDS[kind], opacity=(0.005, 0.012)), cam, S_SMALL,
                    expect=dict(T=17, longest=LONG_TILE, all_tiles=True))
    cam = synthetic.m1_camera(96, 64)
    if kind == "count":
        P = int(arg)
        scene = fill(cam, P, SEEDS[kind] + P, margin=8.0 if P > 1 else -8.0)
        return Case(name, scene, cam, S_SMALL, expect=dict(T=24, min_L=max(1, P // 2), nblk=(P + BIN_SUB - 1) // BIN_SUB))
    if kind.startswith("cull_"):
        P = 3000
        vis = np.ones(P, bool)
        options, expect = {}, {}
        if kind == "cull_first_1024":
            vis[:1024] = False
            expect = dict(sub_zero=[0], nblk=3)
        elif kind == "cull_middle":  # one workgroup walks into and out of the empty sub-range
            vis[1024:2048] = False
            options = dict(test_bin_blocks=1)
            expect = dict(sub_zero=[1], nblk=1)
        elif kind == "cull_last_1500":  # a plateau at the end of sub-range 1's offsets; P % 1024 != 0
            vis[1500:] = False
            expect = dict(sub_zero=[2], nblk=3, plateau=(1500, 2048))
        elif kind == "cull_alternate":
            vis[1::2] = False
            expect = dict(sub_zero=[], nblk=3)
        else:
            raise KeyError(name)
        return Case(name, fill(cam, P, SEEDS["cull"], visible=vis), cam, S_SMALL, options=options,
                    expect=dict(expect, T=24, culled=~vis))
    if kind == "only_last":
        P = 3000
        vis = np.zeros(P, bool)
        vis[-1] = True
        scene = fill(cam, P, SEEDS[kind], sigma_px=(3.0, 6.0), margin=-8.0, visible=vis)
        return Case(name, scene, cam, S_SMALL, expect=dict(T=24, sub_zero=[0, 1], nblk=3, culled=~vis))
    if kind == "sparse_subranges":  # sub-range totals 1024, 1 and 300 (fewer instances than threads)
        P = 3072
        vis = np.zeros(P, bool)
        vis[:1024] = True
        vis[1024 + 517] = True
        vis[2048 + rng.choice(1024, 300, replace=False)] = True
        return Case(name, on_tiles(cam, rng.integers(0, 24, P), SEEDS[kind], visible=vis), cam, S_SMALL,
                    expect=dict(T=24, sub_totals=[1024, 1, 300], nblk=3, culled=~vis))
    if kind == "whole_grid":  # Gaussian 700 covers all 40 x 30 tiles, among small ones
        cam = synthetic.m1_camera(640, 480)
        P = 1500
        u = rng.uniform(-8, cam.width + 8, P)
        v = rng.uniform(-8, cam.height + 8, P)
        sig = np.exp(rng.uniform(np.log(0.3), np.log(4.0), P))
        u[700], v[700], sig[700] = 320.0, 240.0, 600.0
        return Case(name, placed(cam, u, v, rng.uniform(3, 8, P), sig, seed=SEEDS[kind]), cam, S_SMALL,
                    expect=dict(T=1200, whole_grid=700, nblk=2))
    if kind == "rects":  # rects one tile wide / tall, clipped at every edge and corner of the 6 x 4 grid
        scene = fill(cam, 600, SEEDS[kind], sigma_px=(0.5, 10.0), margin=30.0)
        return Case(name, scene, cam, S_SMALL, expect=dict(T=24, rects=True, nblk=1))
    if kind == "wave_rows":
        k = int(arg)
        cam = synthetic.m1_camera(480, 272)
        scene = synthetic.m1_scene(P=60_000, S=3, seed=SEEDS[kind], cam=cam)
        return Case(name, scene, cam, 3, ("two_pass", "one_pass"), options=dict(test_bin_blocks=k) if k else {},
                    expect=dict(T=510, nblk=k or 59, min_L=60_000))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _build(name)
    assert c.variants == variants_of(name)
    return c


def variants_of(name):
    """The scatter variants a case runs under, without building its scene (test collection)."""
    kind, _, arg = name.partition("-")
    if kind == "band":
        return BANDS[tuple(int(x) for x in arg.split("x"))][1]
    return ("two_pass", "one_pass") if kind == "wave_rows" else ("two_pass", "one_pass", "atomic")


@functools.lru_cache(maxsize=4)
def bins(name):
    """oracle_bins of the case: shared, read-only."""
    c = case(name)
    return oracle_bins(c.scene, c.cam)


def in_band(name, variant):
    """Assert through the plan mirror that the case, under the variant, takes the path it is named for."""
    c = case(name)
    e = c.expect
    pl = c.plan(variant)
    assert pl.T == e["T"], (name, pl.T)
    if variant == "atomic":
        assert not pl.lds and pl.nblk == 0 and not pl.two_pass and pl.sub == ATOMIC_SUB, (name, pl)
        if "atomic_ranges" in e:
            assert pl.ranges_kernel == e["atomic_ranges"], (name, pl)
        return pl
    assert pl.lds == e.get("lds", True), (name, pl)
    if pl.lds:
        assert pl.two_pass == (variant == "two_pass") and pl.ranges_kernel == -1 and pl.sub == BIN_SUB, (name, pl)
        assert pl.lds_bytes <= LDS_CU, (name, pl)
    for k in ("nblk", "lds_attr", "lds_bytes", "ranges_kernel"):
        if k in e:
            assert getattr(pl, k) == e[k], (name, k, pl)
    return pl


def covers(name):
    """Assert, from the oracle's binning and the plan mirror, that the case exercises its branch."""
    c = case(name)
    e = c.expect
    b = bins(name)
    kind, _, arg = name.partition("-")
    T, counts, touched = b["T"], b["counts"], b["touched"]
    for variant in c.variants:
        in_band(name, variant)
    pl = c.plan(c.variants[0])
    subs, bks = sub_totals(touched), bucket_totals(counts)
    print(f"{name}: T {T}, P {c.scene.P}, L {b['L']}, longest tile {int(counts.max())}, nblk {pl.nblk}, "
          f"sub-range totals {subs[:6]}{'...' if len(subs) > 6 else ''}")
    assert b["L"] >= e.get("min_L", 1), b["L"]
    if "culled" in e:
        assert not touched[e["culled"]].any() and (b["radii"][e["culled"]] == 0).all()
        assert (touched[~e["culled"]] > 0).mean() > 0.5  # (the fill's margin lies outside the frame)
    if kind == "band":
        if pl.lds:  # every workgroup the matrix allows is used, with Gaussians of its own
            assert pl.nblk == min(bin_blocks_max(T), (BAND_P + BIN_SUB - 1) // BIN_SUB), pl
            assert all(g1 > g0 for g0, g1 in block_ranges(c.scene.P, pl.nblk))
        w, h = c.cam.width, c.cam.height
        if T == BIN_MAX_TILES:
            assert plan(T + 1, c.scene.P).lds is False
        if (w, h) == (2048, 1536):
            assert raises_lds_limit(T + 1) and not raises_lds_limit(T)
    if kind == "tiles":
        assert len(bks) == (T + 15) // 16 and (T + 63) // 64 == {1: 1, 15: 1, 16: 1, 17: 1, 63: 1, 64: 1, 65: 2,
                                                                 129: 3}[T]
    if e.get("all_tiles"):
        assert (counts > 0).all(), int((counts == 0).sum())
    for k in e.get("empty_buckets", []):
        assert bks[k] == 0, (k, bks)
    for k in e.get("full_buckets", []):
        assert (counts[16 * k:16 * k + 16] > 0).all(), (k, counts[16 * k:16 * k + 16])
    if "bucket" in e:  # a staged range of more than one 1024-pair round, the last one partial
        k, n = e["bucket"]
        assert bks[k] == n and n > 1024 and n % 1024 != 0, (k, bks)
    if "longest" in e:
        assert int(counts.max()) == e["longest"], int(counts.max())
    if "max_longest" in e:
        assert int(counts.max()) <= e["max_longest"], int(counts.max())
    if kind == "long_tile":
        assert order_bucket(int(counts.max())) == ORDER_BUCKETS - 1 and int(counts.max()) >= 4 * (ORDER_BUCKETS - 1)
        assert len({order_bucket(int(n)) for n in counts}) >= 8  # and several other buckets of the order
    if kind == "count":
        assert len(subs) == pl.nblk and all(s > 0 for s in subs), subs
    for k in e.get("sub_zero", []):
        assert subs[k] == 0, subs
    if "sub_zero" in e:
        assert all(s > 0 for k, s in enumerate(subs) if k not in e["sub_zero"]), subs
    if "sub_totals" in e:
        assert subs == e["sub_totals"], subs
    if "plateau" in e:
        g0, g1 = e["plateau"]
        assert c.scene.P % BIN_SUB != 0 and subs[g0 // BIN_SUB] > 0
        assert len(set(b["offsets"][g0 - 1:g1].tolist())) == 1  # the sub-range's offsets end in a plateau
    if kind == "cull_middle":  # the one workgroup's range spans the empty sub-range
        assert block_ranges(c.scene.P, pl.nblk) == [(0, c.scene.P)]
    if kind == "cull_alternate":
        assert not touched[1::2].any() and (touched[0::2] > 0).mean() > 0.5
    if kind == "only_last":
        assert b["L"] == touched[-1] == subs[-1] and b["L"] > 1
    if "whole_grid" in e:
        g = e["whole_grid"]
        assert b["rect"][g].tolist() == [0, 0, b["gx"], b["gy"]] and touched[g] == T == 1200
        for sub in (BIN_SUB, ATOMIC_SUB):  # its run is split over many threads, most starting mid-rect
            tot = sub_totals(touched, sub)[g // sub]
            per = (tot + sub - 1) // sub
            assert T // per >= 64, (sub, tot, per)
            assert per % b["gx"] != 0  # thread runs start at columns k % w != 0
        assert np.median(touched[touched > 0]) <= 4
    if e.get("rects"):
        r, gx, gy = b["rect"][touched > 0], b["gx"], b["gy"]
        x0, y0, w, h = r.T
        n = dict(wide1=int(((w == 1) & (h > 1)).sum()), tall1=int(((h == 1) & (w > 1)).sum()),
                 single=int(((w == 1) & (h == 1)).sum()), left=int(((x0 == 0) & (w < gx)).sum()),
                 right=int(((x0 + w == gx) & (w < gx)).sum()), top=int(((y0 == 0) & (h < gy)).sum()),
                 bottom=int(((y0 + h == gy) & (h < gy)).sum()), full=int(((w == gx) & (h == gy)).sum()),
                 corner=int(((x0 == 0) & (y0 == 0) & (w < gx) & (h < gy)).sum()))
        print(f"{name}: rects {n}")
        assert all(v >= 3 for k, v in n.items() if k != "full"), n
        # clipped, not merely touching: centres outside the frame on every side
        m = c.scene.means3D[touched > 0]
        u = m[:, 0] / m[:, 2] * c.cam.focal[0] + c.cam.cx
        v = m[:, 1] / m[:, 2] * c.cam.focal[1] + c.cam.cy
        assert (u < 0).any() and (u > c.cam.width).any() and (v < 0).any() and (v > c.cam.height).any()
    if kind == "wave_rows":
        rows = colscan_rows(pl.nblk)
        want = {1: (15, 1, 1), 2: (14, 1, 1), 15: (1, 1, 1), 16: (0, 1, 1), 17: (0, 1, 2), 59: (0, 3, 4)}[pl.nblk]
        assert (rows.count(0), min(r for r in rows if r), max(rows)) == want and sum(rows) == pl.nblk, rows
        assert all(g1 > g0 for g0, g1 in block_ranges(c.scene.P, pl.nblk))
