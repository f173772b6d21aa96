"""CPU checks of the display and capture head and the environment background: tests/display_ref64.py against
tests/golden/display.npz (the reference's float32 torch bits and torch float64), the 8-bit quantiser at every
level and half-way point, the boundary of `_C.display` and of relightable3dgaussian_amd/display.py and
relight.env_background, and the C ABI's argument checks (no device work, so no GPU)."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import relightable3dgaussian_amd as r
from relightable3dgaussian_amd import display, relight
from tests import display_ref64 as d64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "r3dg_hip.h")
LIB = os.path.join(ROOT, "relightable3dgaussian_amd", "lib", "libr3dg_hip.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "display.npz")
NAMES = ("r3dg_display_frame", "r3dg_env_background")
ALLOC = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
EXACT = 1e-13  # float64 against float64: the same expressions, at most a different association
F = np.float32
ENV_LIGHTS = ("map8", "map8_T", "map64", "map64_T", "sh0", "sh3", "sh4")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def case(golden, name):
    return {k: golden[f"{name}/{k}"] for k in ("rgb", "gray", "count", "opacity", "bg", "bgimg")}


def same_bits(a, b):
    """Equal float32 bits; a NaN equals any NaN (IEEE 754 leaves the sign and payload of 0 / 0 open)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype == F and a.shape == b.shape
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def env_light(golden, name):
    if name.startswith("map"):
        m = d64.smooth_envmap(8, 16) if name.startswith("map8") else d64.smooth_envmap(64, 128)
        return dict(envmap=m, transform=golden["env/T"] if name.endswith("_T") else None, shs=None)
    deg = int(name[2:])
    return dict(envmap=None, transform=None, shs=np.ascontiguousarray(golden["env/shs"][:, :(deg + 1) ** 2]))


# ---- the yardstick ---------------------------------------------------------------------------------------------

def test_float32_restatement_is_the_golden_bits(golden):
    assert set(golden["cases_full"]) < set(golden["cases"]) and "r_67x131" in golden["cases"]
    for name in golden["cases"]:
        c = case(golden, name)
        full = name in golden["cases_full"]
        for view in d64.VIEWS:
            y = d64.view(c, view, "none", F)
            assert y.dtype == F and y.shape == c["rgb"].shape
            if full:
                assert same_bits(y, golden[f"{name}/{view}/f32/none"]), (name, view)
                np.testing.assert_array_equal(d64.quantise(d64.view(c, view, "clamp", F)), golden[f"{name}/{view}/u8/clamp"])
            np.testing.assert_array_equal(d64.quantise(y), golden[f"{name}/{view}/u8/none"], err_msg=f"{name} {view}")
            assert same_bits(d64.view(c, view, "clamp", F), d64.clamp01(y))
        if full:
            for kind in d64.RANGE_VARIANTS:
                y = d64.frame(d64.range_variant(c["gray"], kind), "range", "none", dt=F)
                assert same_bits(y, golden[f"{name}/range_{kind}/f32"]), (name, kind)
                np.testing.assert_array_equal(d64.quantise(y), golden[f"{name}/range_{kind}/u8"])


def test_range_variants_are_the_stated_edges(golden):
    g = golden["r_67x131/gray"]
    n = g.size
    assert n % 4 == 1 and (n + 1023) // 1024 == 9  # a tail lane of one pixel, nine workgroups of the pre-pass
    v = d64.range_variant(g, "first").reshape(-1)
    assert v[0] == v.min() == -3 and v.max() == 5
    v = d64.range_variant(g, "last").reshape(-1)
    assert v[-1] == v.max() == 5 and v.min() == -3
    v = d64.range_variant(g, "last_workgroup").reshape(-1)
    assert v.argmin() >= 8 * 1024 and v.argmax() >= 8 * 1024 and v.argmax() < n - 1
    assert np.isnan(d64.range_variant(g, "nan")).sum() == 1
    assert np.isnan(d64.frame(d64.range_variant(g, "nan"), "range", "none", dt=F)).all()
    assert np.isnan(d64.frame(d64.range_variant(g, "constant"), "range", "none", dt=F)).all()  # 0 / 0
    assert not d64.quantise(d64.frame(d64.range_variant(g, "nan"), "range", "none", dt=F)).any()


def test_float64_restatement_and_the_aces_floors(golden):
    for name in golden["cases"]:
        c = case(golden, name)
        for view in d64.ACES_VIEWS:
            floor = float(golden[f"{name}/{view}/floor/aces"])
            assert 0 <= floor < 1e-6
            y64 = d64.view(c, view, "aces", np.float64)
            if name in golden["cases_full"]:
                assert d64.rel_err(y64, golden[f"{name}/{view}/f64/aces"]) <= EXACT
            assert d64.rel_err(d64.view(c, view, "aces", F), y64) <= d64.bar(floor)
            near = d64.near_level(y64, d64.bar(floor))
            assert near.mean() <= d64.MAX_LEFT_OUT, (name, view, near.mean())
            diff = d64.quantise(d64.view(c, view, "aces", F)).astype(int) - d64.quantise(y64).astype(int)
            assert np.abs(diff).max() <= 1 and not np.any(diff[~near])


def test_env_restatement_reproduces_the_golden_float64(golden):
    h, w = 5, 7
    K, c2w = golden[f"env/K_{h}x{w}"], golden["env/c2w"]
    assert K[0, 2] != w / 2 and K[1, 2] != h / 2 and abs(np.linalg.det(c2w[:3, :3].astype(np.float64)) - 1) < 1e-6
    assert not np.allclose(c2w[:3, :3], np.eye(3), atol=0.1)
    for name in ENV_LIGHTS:
        ref = golden[f"env/{h}x{w}/{name}/f64"]
        got = d64.env_background(K, c2w, h, w, dt=np.float64, **env_light(golden, name))
        assert got.shape == (h, w, 3) and d64.rel_err(got, ref) <= EXACT, name
        assert d64.env_background(K, c2w, h, w, dt=F, **env_light(golden, name)).dtype == F
    for k in golden:
        if k.startswith("env/") and k.endswith("/floor"):
            assert 0 <= float(golden[k]) < 1e-5, k
    d = d64.world_directions(K, c2w, h, w)
    np.testing.assert_allclose(np.linalg.norm(d, axis=-1), 1.0, atol=1e-12)
    m = d64.smooth_envmap(64, 128)
    assert m.shape == (64, 128, 3) and m.dtype == F and np.array_equal(m * 64, np.round(m * 64)) and m.min() > 0


# ---- the 8-bit quantiser ---------------------------------------------------------------------------------------

def two_roundings(y):
    """floor(fl32(fl32(y * 255) + 0.5)) with both products and sums formed exactly in float64 (a float32 times 255
    and a float32 plus 0.5 are exact there) and rounded once to float32, independent of numpy's float32 arithmetic."""
    t = np.float32(np.float64(y) * 255.0)
    t = np.float32(np.float64(t) + 0.5)
    return np.uint8(np.floor(np.clip(np.float64(t), 0, 255)))


def test_quantiser_levels_and_half_way_points():
    levels = (np.arange(256) / 255).astype(F)
    np.testing.assert_array_equal(d64.quantise(levels), np.arange(256))
    half = ((np.arange(255) + 0.5) / 255).astype(F)
    ys = np.concatenate([levels, half, np.nextafter(half, F(-1)), np.nextafter(half, F(2)), np.nextafter(levels, F(-1)),
                         np.nextafter(levels, F(2)),
                         np.array([0.0, -0.0, -1e-30, -0.5, -np.inf, 1.0, 1.0001, 2.0, 1e30, np.inf], F)]).astype(F)
    got = d64.quantise(ys)
    np.testing.assert_array_equal(got, np.array([two_roundings(y) for y in ys]))
    ref = torch.from_numpy(ys.copy()).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()  # save_image
    np.testing.assert_array_equal(got, ref)
    # one float32 step below a half-way point stays in the lower byte or not exactly as the two roundings say:
    # the two sides of at least one half-way point land in different bytes
    lo, hi = d64.quantise(np.nextafter(half, F(-1))), d64.quantise(np.nextafter(half, F(2)))
    assert np.all(hi - lo <= 1) and np.all(hi >= lo) and np.any(hi != lo)
    assert np.all(got[-10:] == [0, 0, 0, 0, 0, 255, 255, 255, 255, 255])
    assert d64.quantise(np.array([np.nan], F))[0] == 0 and d64.quantise(np.array([np.nan]))[0] == 0
    # float64 mode at the levels
    np.testing.assert_array_equal(d64.quantise(np.arange(256) / 255), np.arange(256))


# ---- the boundary ----------------------------------------------------------------------------------------------

def test_binding_is_a_submodule_and_refuses_host_tensors():
    sub = r._C.display
    assert not callable(sub)
    assert {n for n in dir(sub) if callable(getattr(sub, n)) and not n.startswith("_")} == {"frame", "env_background"}
    assert dict(sub.MODES) == {m: i for i, m in enumerate(d64.MODES)} and sub.MAX_SPECS == 16
    assert dict(sub.TONES) == {t: i for i, t in enumerate(d64.TONES)} and dict(sub.ENCODINGS) == {"f32": 0, "u8": 1}
    s, o, b = torch.zeros(4, 5, 3), torch.zeros(4, 5, 1), torch.zeros(3)
    cnt = torch.zeros(4, 5, 1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sub.frame([s], [0], [0], [False], None, None, [], 1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sub.frame([s, o], [1, 1], [0, 1], [False, False], o, b, [], 0)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sub.frame([cnt], [5], [0], [False], None, None, [], 1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sub.frame([s.permute(2, 0, 1).contiguous()], [1], [0], [True], o, None, [0.5, 0.5, 0.5], 1)
    with pytest.raises(RuntimeError, match="float32"):
        sub.frame([s.double()], [0], [0], [False], None, None, [], 1)
    with pytest.raises(RuntimeError, match="int32"):
        sub.frame([s], [5], [0], [False], None, None, [], 1)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        sub.frame([s], [0], [0], [True], None, None, [], 1)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        sub.frame([s, torch.zeros(4, 6, 1)], [0, 0], [0, 0], [False, False], None, None, [], 1)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        sub.frame([s], [1], [0], [False], torch.zeros(4, 5), b, [], 1)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        sub.frame([s], [1], [0], [False], o, torch.zeros(4), [], 1)
    with pytest.raises(RuntimeError, match="unknown mode"):
        sub.frame([s], [6], [0], [False], None, None, [], 1)
    with pytest.raises(RuntimeError, match="unknown tone"):
        sub.frame([s], [0], [3], [False], None, None, [], 1)
    with pytest.raises(RuntimeError, match="unknown encoding"):
        sub.frame([s], [0], [0], [False], None, None, [], 2)
    with pytest.raises(RuntimeError, match="specs expected"):
        sub.frame([s] * 17, [0] * 17, [0] * 17, [False] * 17, None, None, [], 1)
    with pytest.raises(RuntimeError, match="specs expected"):
        sub.frame([], [], [], [], None, None, [], 1)
    K, c2w, m = torch.eye(3), torch.eye(4), torch.zeros(8, 16, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sub.env_background(K, c2w, 4, 5, m, None, None)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sub.env_background(K, torch.eye(3), 4, 5, None, None, torch.zeros(1, 16, 3))
    with pytest.raises(RuntimeError, match="shape mismatch"):
        sub.env_background(torch.eye(4), c2w, 4, 5, m, None, None)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        sub.env_background(K, c2w, 4, 5, None, None, torch.zeros(1, 36, 3))
    with pytest.raises(RuntimeError, match="one of envmap and shs"):
        sub.env_background(K, c2w, 4, 5, None, None, None)


def test_frame_buffers_argument_errors():
    s, o, b = torch.zeros(4, 5, 3), torch.zeros(4, 5, 1), torch.zeros(3)
    g, cnt = torch.zeros(4, 5, 1), torch.zeros(4, 5, 1, dtype=torch.int32)
    fb = display.frame_buffers
    bad = [
        (dict(specs=[(s.double(), "plain", "none")]), "spec 0: source: a float32 tensor"),        # dtype
        (dict(specs=[(s.numpy(), "plain", "none")]), "spec 0: source: a float32 tensor"),
        (dict(specs=[(torch.zeros(4, 5), "plain", "none")]), "spec 0: shape mismatch"),             # rank
        (dict(specs=[(torch.zeros(4, 5, 2), "plain", "none")]), "spec 0: shape mismatch"),          # channels
        (dict(specs=[(s, "plain", "none", "chw")]), "spec 0: shape mismatch"),                      # layout
        (dict(specs=[(torch.zeros(0, 5, 3), "plain", "none")]), "spec 0: shape mismatch"),
        (dict(specs=[(s, "plain", "none"), (torch.zeros(4, 6, 3), "plain", "none")]), "spec 1: shape mismatch: every source"),
        (dict(specs=[(s, "plain", "none"), (torch.zeros(3, 5, 1), "plain", "none")]), "spec 1: shape mismatch: every source"),
        (dict(specs=[(s, "plain", "none"), (torch.zeros(3, 5, 4), "plain", "none", "chw")]), "spec 1: shape mismatch: every source"),
        (dict(specs=[(s, "under", "none")]), "spec 0: mode"),
        (dict(specs=[(s, "plain", "gamma")]), "spec 0: tone"),
        (dict(specs=[(s, "plain", "none", "nhwc")]), "spec 0: layout"),
        (dict(specs=[(s, "plain")]), "spec 0: (source, mode, tone)"),
        (dict(specs=[(s, "plain", "none")], encoding="u16"), "encoding"),
        (dict(specs=[]), "1 to 16 specs"),
        (dict(specs=[(s, "plain", "none")] * 17), "1 to 16 specs"),
        (dict(specs=[(s, "over", "none")], bg=b), "spec 0: mode 'over' needs opacity"),
        (dict(specs=[(s, "normal_mask", "none")]), "spec 0: mode 'normal_mask' needs opacity"),
        (dict(specs=[(s, "over", "none")], opacity=o), "spec 0: mode 'over' needs bg"),
        (dict(specs=[(s, "normal_over", "clamp")], opacity=o), "spec 0: mode 'normal_over' needs bg"),
        (dict(specs=[(g, "count", "none")]), "spec 0: source: an int32 tensor"),                    # count on float
        (dict(specs=[(cnt, "plain", "none")]), "spec 0: source: a float32 tensor"),                 # another mode on int
        (dict(specs=[(cnt, "range", "none")]), "spec 0: source: a float32 tensor"),
        (dict(specs=[(torch.zeros(4, 5, 3, dtype=torch.int32), "count", "none")]), "spec 0: shape mismatch"),
        (dict(specs=[(s, "over", "none")], opacity=o.double(), bg=b), "opacity: a float32 tensor"),
        (dict(specs=[(s, "over", "none")], opacity=torch.zeros(4, 5), bg=b), "shape mismatch: opacity"),
        (dict(specs=[(s, "over", "none")], opacity=torch.zeros(4, 6, 1), bg=b), "shape mismatch: opacity"),
        (dict(specs=[(s, "over", "none")], opacity=o, bg=b.double()), "bg: a float32 tensor"),
        (dict(specs=[(s, "over", "none")], opacity=o, bg=torch.zeros(4)), "shape mismatch: bg"),
        (dict(specs=[(s, "over", "none")], opacity=o, bg=torch.zeros(4, 6, 3)), "shape mismatch: bg"),
        (dict(specs=[(s, "over", "none")], opacity=o, bg="white"), "bg: a float32 tensor [3]"),
        (dict(specs=[(s, "plain", "none"), (g.to("meta"), "plain", "none")]), "spec 1: source is on"),
        (dict(specs=[(s, "over", "none")], opacity=o.to("meta"), bg=b), "opacity is on"),
        (dict(specs=[(s, "over", "none")], opacity=o, bg=b.to("meta")), "bg is on"),
        (dict(specs=[(s.clone().requires_grad_(True), "plain", "none")]), "forward only"),
        (dict(specs=[(s, "over", "none")], opacity=o.clone().requires_grad_(True), bg=b), "forward only"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=re.escape("frame_buffers: " + msg)):
            fb(**kw)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU tensor"):  # forward only is fine without grad; no fallback
        fb([(s.clone().requires_grad_(True), "plain", "none")])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        fb([(s, "over", "aces"), (g, "range", "clamp"), (cnt, "count", "none")], opacity=o, bg=1, encoding="f32")


def test_env_background_argument_errors():
    K, c2w, shs = torch.eye(3), torch.eye(4), torch.zeros(1, 16, 3)
    bad = [(dict(intrinsics=K.double()), ValueError, "intrinsics: a float32"), (dict(intrinsics=c2w), ValueError, "shape mismatch: intrinsics"),
           (dict(c2w=torch.eye(2)), ValueError, "shape mismatch: c2w"), (dict(H=0), ValueError, "H, W >= 1"),
           (dict(light=shs.double()), ValueError, "light: a float32"), (dict(light=torch.zeros(1, 36, 3)), ValueError, "shape mismatch: environment SH"),
           (dict(light=torch.zeros(16, 3)), ValueError, "shape mismatch: environment SH"), (dict(light=None), TypeError, "light must be"),
           (dict(c2w=c2w.to("meta")), ValueError, "c2w is on"), (dict(light=shs.to("meta")), ValueError, "light is on")]
    for kw, exc, msg in bad:
        args = dict(light=shs, intrinsics=K, c2w=c2w, H=4, W=5)
        args.update(kw)
        with pytest.raises(exc, match=re.escape("env_background: " + msg)):
            relight.env_background(**args)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        relight.env_background(shs, K, c2w, 4, 5)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        relight.env_background(relight.EnvLight(torch.zeros(8, 16, 3)), K, torch.eye(3), 4, 5)


class Spec(ctypes.Structure):
    _fields_ = [("source", ctypes.c_void_p), ("channels", ctypes.c_int), ("layout", ctypes.c_int), ("mode", ctypes.c_int),
                ("tone", ctypes.c_int)]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(LIB)
    lib.r3dg_last_error.restype = ctypes.c_char_p
    ci, vp = ctypes.c_int, ctypes.c_void_p
    lib.r3dg_display_frame.argtypes = [ci, ci, ci, ctypes.POINTER(Spec), vp, vp, ci, ci, vp, ALLOC, vp, vp]
    lib.r3dg_env_background.argtypes = [ci, ci, vp, vp, ci, ci, vp, ci, ci, vp, vp, ci, vp, vp]
    for n in NAMES:
        getattr(lib, n).restype = ci
    return lib


def test_header_declares_and_library_exports(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert hasattr(lib, n), n
    assert re.search(r"typedef struct r3dg_display_spec", text) and "R3DG_DISPLAY_MAX_SPECS 16" in text
    assert int(re.search(r"#define R3DG_ABI_VERSION (\d+)", text).group(1)) == 2  # additive: no struct changed


def test_argument_errors_need_no_device(lib):
    """R3DG_ERR_ARG (-1) with a message before any device work or allocation."""
    calls = []

    @ALLOC
    def never(ctx, nbytes):
        calls.append(nbytes)
        return None

    no_alloc = ctypes.cast(None, ALLOC)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def frame(H=2, W=2, n=1, specs="one", source=p, channels=3, layout=1, mode=0, tone=0, opacity=p, bg=p, bg_kind=1, enc=1,
              out=p, alloc=never):
        arr = (Spec * 17)(*[Spec(source, channels, layout, mode, tone) for _ in range(17)])
        return lib.r3dg_display_frame(H, W, n, None if specs is None else arr, opacity, bg, bg_kind, enc, out, alloc, None, None)

    def env(H=2, W=2, K=p, c2w=p, stride=4, mode=2, envmap=p, eh=4, ew=8, shs=p, S=16, out=p):
        return lib.r3dg_env_background(H, W, K, c2w, stride, mode, envmap, eh, ew, None, shs, S, out, None)

    bad = {"H 0": lambda: frame(H=0), "negative W": lambda: frame(W=-1), "beyond int32": lambda: frame(H=65536, W=65536),
           "no spec": lambda: frame(n=0), "17 specs": lambda: frame(n=17), "null specs": lambda: frame(specs=None),
           "null out": lambda: frame(out=None), "null source": lambda: frame(source=None), "channels 2": lambda: frame(channels=2),
           "layout": lambda: frame(layout=2), "mode": lambda: frame(mode=6), "negative mode": lambda: frame(mode=-1),
           "tone": lambda: frame(tone=3), "encoding": lambda: frame(enc=2), "bg_kind": lambda: frame(bg_kind=4),
           "bg kind without bg": lambda: frame(bg=None), "bg without kind": lambda: frame(bg_kind=0),
           "over without opacity": lambda: frame(mode=1, opacity=None), "mask without opacity": lambda: frame(mode=3, opacity=None),
           "over without bg": lambda: frame(mode=1, bg=None, bg_kind=0), "normal_over without bg": lambda: frame(mode=2, bg=None, bg_kind=0),
           "count on three channels": lambda: frame(mode=5), "range without scratch_alloc": lambda: frame(mode=4, alloc=no_alloc),
           "env H 0": lambda: env(H=0), "env beyond int32": lambda: env(H=65536, W=65536), "env null K": lambda: env(K=None),
           "env null c2w": lambda: env(c2w=None), "env null out": lambda: env(out=None), "env stride": lambda: env(stride=5),
           "env mode none": lambda: env(mode=0), "env mode": lambda: env(mode=3), "env null map": lambda: env(envmap=None),
           "env map height 0": lambda: env(eh=0), "env null shs": lambda: env(mode=1, shs=None), "env S 0": lambda: env(mode=1, S=0),
           "env S 26": lambda: env(mode=1, S=26)}
    for what, call in bad.items():
        assert call() == -1, what
        assert len(lib.r3dg_last_error()) > 0, what
    assert calls == []
