"""The display and capture head and the environment background on the GPU (csrc/display.hip, csrc/relight.hip
`env_background_kernel`; relightable3dgaussian_amd/display.py, relight.env_background) against
tests/display_ref64.py and tests/golden/display.npz.

Exact cases: every mode with tone "none" or "clamp", in both encodings, is the reference's float32 torch bits
(a NaN for a NaN: IEEE 754 leaves the sign and payload of 0 / 0 open) or its uint8 bytes. For the cases of
golden["cases_full"] those are stored; at 67x131 only the tone-"none" bytes are, and the rest is
display_ref64's float32 mode, which tests/golden/make_golden_display.py asserts to be those bits for that
very case.
Inexact cases: the ACES tone and env_background, within 4 x max(floor, 2^-24) of the float64 result, the floor
being the distance of the reference's own float32 evaluation from it, in the measure rel_err = max|got - ref|
/ max|ref|; ACES bytes within 1 of the float64 bytes and only where float64 y * 255 + 0.5 is within the bar of an
integer. Every error figure is printed before it is asserted.

Measured on the MI355X (profiles/display/test_gpu_display.log): every figure within its bar.
The ACES image's error equals its floor at every shape (largest share of a bar 0.25) and none of its bytes differs
from the float64 bytes; the largest share of a bar is 0.72 (env_background, degree-3 SH on the one-pixel image:
1.7e-7 against a bar of four roundings, 2.4e-7); the map lookups reach 0.27 and direct_light 0.31.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

from tests import display_ref64 as d64
from tests._helpers import tt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
SHAPES = ["r_1x1", "r_1x3", "r_2x2", "r_5x7", "r_16x16", "r_33x31", "r_67x131"]
LAYOUTS = ("hwc", "chw")
# where the sources sit in a [S H W] feature buffer, in units of H W floats: (gray, opacity, rgb). S = 11 has group
# widths 1, 1, 3, 3, 3 (test_gpu_pbr_head.py::inputs): for odd H W rgb starts 8 bytes off a 16-byte boundary and
# opacity 4 or 12. S = 21 has widths 3, 3, 3, 1, 1, 3, 3, 3, 1 (relight.FEATURE_COLUMNS): rgb is its second block
# (4 or 12 bytes off), gray its roughness (4 or 12) and opacity its metallic block (8).
BLOCKS = {11: (0, 1, 2), 21: (9, 10, 3)}
GROUPS = {"vec": [v for v, (_, _, k) in d64.VIEWS.items() if k in (None, "vec")], "num": ["over1_num"], "img": ["over3_img"]}
ENV_SHAPES = [(1, 1), (5, 7), (33, 31)]
ENV_LIGHTS = ("map8", "map8_T", "map64", "map64_T", "sh0", "sh3", "sh4")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "display.npz"))
    out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def case(golden, name):
    return {k: golden[f"{name}/{k}"] for k in ("rgb", "gray", "count", "opacity", "bg", "bgimg")}


def lay(a, layout):
    return a if layout == "hwc" else np.ascontiguousarray(np.transpose(a, (2, 0, 1)))


def device_inputs(c, layout, S):
    """The case on the GPU: rgb and gray in `layout`, opacity [H,W,1]. S: None, or 11 / 21 for views into one
    [S H W] feature buffer (NaN elsewhere) at BLOCKS' offsets."""
    import torch

    rgb, gray, opacity = tt(lay(c["rgb"], layout)), tt(lay(c["gray"], layout)), tt(c["opacity"])
    if S is not None:
        n = c["gray"].size
        feat = torch.full((S * n,), float("nan"), device="cuda")
        assert feat.data_ptr() % 16 == 0
        views = []
        for t, at in zip((gray, opacity, rgb), BLOCKS[S]):
            feat[at * n:at * n + t.numel()] = t.reshape(-1)
            views.append(feat[at * n:at * n + t.numel()].view(t.shape))
        gray, opacity, rgb = views
        assert rgb.is_contiguous() and (n % 2 == 0 or rgb.data_ptr() % 16 != 0)
    count = torch.as_tensor(np.ascontiguousarray(c["count"]), device="cuda")
    return {"rgb": rgb, "gray": gray, "count": count, "opacity": opacity, "bg": tt(c["bg"]), "bgimg": tt(c["bgimg"])}


def call(specs, opacity=None, bg=None, encoding="u8"):
    """frame_buffers with the checks every output gets: fresh, contiguous, the stated dtype and shape."""
    import torch

    from relightable3dgaussian_amd.display import frame_buffers

    out = frame_buffers(specs, opacity=opacity, bg=bg, encoding=encoding)
    s0, lay0 = specs[0][0], specs[0][3] if len(specs[0]) == 4 else "hwc"
    H, W = (s0.shape[1:] if lay0 == "chw" else s0.shape[:2])
    assert out.shape == (len(specs), H, W, 3) and out.is_contiguous()
    assert out.dtype == (torch.uint8 if encoding == "u8" else torch.float32)
    own = out.untyped_storage().data_ptr()
    used = [s[0] for s in specs] + [t for t in (opacity, bg) if isinstance(t, torch.Tensor)]
    assert all(own != t.untyped_storage().data_ptr() for t in used), "the output aliases an input"
    return out.cpu().numpy()


def same_bits(got, want, tag):
    assert got.dtype == want.dtype == F and got.shape == want.shape, tag
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=tag)
    np.testing.assert_array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32), err_msg=tag)


def expected(golden, name, c, view, tone):
    """(float32 image, bytes) of an exact view: stored where the golden file holds them, else the float32
    restatement that the golden maker asserts to be the reference's bits for this case."""
    full = name in golden["cases_full"]
    y = golden[f"{name}/{view}/f32/none"] if full else d64.view(c, view, "none", F)
    if tone == "clamp":
        y = d64.clamp01(y)
    key = f"{name}/{view}/u8/{tone}"
    return y, golden[key] if key in golden else d64.quantise(y)


def within(tag, what, err, floor):
    b = d64.bar(floor)
    print(f"{tag} {what:10s} {err:.3e} (bar {b:.2e}, floor {float(floor):.2e}, {err / b:5.1%} of the bar)")
    assert err <= b, (tag, what, err, b)


def spec_of(dev, view, tone, layout):
    src, mode, _ = d64.VIEWS[view]
    return (dev[src], mode, tone, layout) if src != "count" else (dev[src], mode, tone)


@pytest.mark.parametrize("S", [None, 11, 21], ids=["own", "views11", "views21"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SHAPES)
def test_exact_modes(hip_ext, golden, name, layout, S):
    """1x1 one lane, tail only; 1x3 tail of three; 2x2 one full quad; 5x7 odd H W with a tail of three; 16x16 one
    wave's worth; 33x31 odd H W, several waves, a tail of three; 67x131 several workgroups (nine of the range
    pre-pass) and a tail of one. Every view of display_ref64.VIEWS, grouped by the kind of bg, eight specs in
    the largest call."""
    c = case(golden, name)
    dev = device_inputs(c, layout, S)
    for kind, views in GROUPS.items():
        bg = {"vec": dev["bg"], "num": d64.BG_NUM, "img": dev["bgimg"]}[kind]
        for tone in ("none", "clamp"):
            specs = [spec_of(dev, v, tone, layout) for v in views]
            f = call(specs, dev["opacity"], bg, "f32")
            u = call(specs, dev["opacity"], bg, "u8")
            for k, v in enumerate(views):
                tag = f"{name} {layout} S={S} {v} {tone}"
                y, b = expected(golden, name, c, v, tone)
                same_bits(f[k], y, tag)
                np.testing.assert_array_equal(u[k], b, err_msg=tag)


@pytest.mark.parametrize("S", [None, 21], ids=["own", "views21"])
@pytest.mark.parametrize("kind", d64.RANGE_VARIANTS)
@pytest.mark.parametrize("name", SHAPES)
def test_range_edges(hip_ext, golden, name, kind, S):
    """The extremum in the first pixel, in the last (tail) pixel, in the last workgroup of the pre-pass; one NaN
    (every output NaN, every byte 0); a constant image (0 / 0)."""
    c = case(golden, name)
    g = d64.range_variant(c["gray"], kind)
    dev = device_inputs(dict(c, gray=g), "hwc", S)
    full = name in golden["cases_full"]
    y = golden[f"{name}/range_{kind}/f32"] if full else d64.frame(g, "range", "none", dt=F)
    b = golden[f"{name}/range_{kind}/u8"] if full else d64.quantise(y)
    tag = f"{name} range {kind} S={S}"
    same_bits(call([(dev["gray"], "range", "none")], encoding="f32")[0], y, tag)
    np.testing.assert_array_equal(call([(dev["gray"], "range", "none")], encoding="u8")[0], b, err_msg=tag)
    if kind in ("nan", "constant"):
        assert np.isnan(y).all() and not b.any()


@pytest.mark.parametrize("S", [None, 11], ids=["own", "views11"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SHAPES)
def test_aces(hip_ext, golden, name, layout, S):
    c = case(golden, name)
    dev = device_inputs(c, layout, S)
    specs = [spec_of(dev, v, "aces", layout) for v in d64.ACES_VIEWS]
    f = call(specs, dev["opacity"], dev["bg"], "f32")
    u = call(specs, dev["opacity"], dev["bg"], "u8")
    for k, v in enumerate(d64.ACES_VIEWS):
        tag = f"{name} {layout} S={S} {v}"
        floor = float(golden[f"{name}/{v}/floor/aces"])
        y64 = golden[f"{name}/{v}/f64/aces"] if name in golden["cases_full"] else d64.view(c, v, "aces", np.float64)
        within(tag, "aces f32", d64.rel_err(f[k], y64), floor)
        near = d64.near_level(y64, d64.bar(floor))
        diff = u[k].astype(int) - d64.quantise(y64).astype(int)
        print(f"{tag} aces u8    {int(np.abs(diff).sum())} bytes off by one, {near.mean():.2e} of the case near a level "
              f"(cap {d64.MAX_LEFT_OUT})")
        assert near.mean() <= d64.MAX_LEFT_OUT, tag
        assert np.abs(diff).max() <= 1 and not np.any(diff[~near]), tag


def relight_list(dev):
    """relighting.py's default --capture_list: base_color, metallic, normal, pbr, pbr_env, shader, points, render,
    roughness, visibility (:139), with their composites of :225-229; `points` is render_points' [3,H,W]."""
    import torch

    pts = dev["rgb"].permute(2, 0, 1).contiguous()
    other = torch.flip(dev["bgimg"], (0,)).contiguous()
    return [(dev["rgb"], "over", "none"), (dev["gray"], "over", "none"), (dev["rgb"], "normal_over", "none"),
            (dev["bgimg"], "plain", "none"), (other, "plain", "none"), (dev["rgb"], "plain", "none"),
            (pts, "plain", "none", "chw"), (other, "plain", "none"), (dev["opacity"], "over", "none"),
            (dev["gray"], "over", "none")]


@pytest.mark.parametrize("name", ["r_5x7", "r_67x131"])
def test_capture_list_in_one_call_is_the_single_calls(hip_ext, golden, name):
    dev = device_inputs(case(golden, name), "hwc", 21)
    specs = relight_list(dev)
    assert len(specs) == 10
    for enc in ("u8", "f32"):
        for bg in (dev["bg"], 1, 0.25, dev["bgimg"]):
            together = call(specs, dev["opacity"], bg, enc)
            for k, s in enumerate(specs):
                one = call([s], dev["opacity"], bg, enc)[0]
                np.testing.assert_array_equal(together[k].view(np.uint32 if enc == "f32" else np.uint8),
                                              one.view(np.uint32 if enc == "f32" else np.uint8), err_msg=f"{name} {enc} spec {k}")


def test_sixteen_specs_and_no_more(hip_ext, golden):
    c = case(golden, "r_33x31")
    dev = device_inputs(c, "hwc", 11)
    views = list(d64.VIEWS)
    views = [v for v in views if d64.VIEWS[v][2] in (None, "vec")]
    specs = [spec_of(dev, views[k % len(views)], ("none", "clamp")[k // len(views)], "hwc") for k in range(16)]
    u = call(specs, dev["opacity"], dev["bg"], "u8")
    for k in range(16):
        _, b = expected(golden, "r_33x31", c, views[k % len(views)], ("none", "clamp")[k // len(views)])
        np.testing.assert_array_equal(u[k], b, err_msg=f"spec {k}")
    with pytest.raises(ValueError, match="1 to 16 specs"):
        call(specs + specs[:1], dev["opacity"], dev["bg"], "u8")


@pytest.mark.parametrize("name", ["r_5x7", "r_67x131"])
def test_two_range_specs_each_get_their_own_range(hip_ext, golden, name):
    """Sources of different ranges and channel counts, with a spec of another mode between them."""
    c = case(golden, name)
    wide = d64.range_variant(c["gray"], "last_workgroup")
    dev = device_inputs(c, "hwc", None)
    f = call([(dev["gray"], "range", "none"), (dev["rgb"], "plain", "none"), (tt(wide), "range", "clamp"),
              (dev["rgb"], "range", "none")], encoding="f32")
    same_bits(f[0], d64.frame(c["gray"], "range", "none", dt=F), name)
    same_bits(f[1], c["rgb"], name)
    same_bits(f[2], d64.frame(wide, "range", "clamp", dt=F), name)
    same_bits(f[3], d64.frame(c["rgb"], "range", "none", dt=F), name)
    assert not np.array_equal(f[0], f[2])


# ---- the environment background --------------------------------------------------------------------------------

def env_light(golden, lname):
    """(EnvLight or SH tensor for the GPU, the numpy keywords of display_ref64.env_background)."""
    from relightable3dgaussian_amd.relight import EnvLight

    if lname.startswith("map"):
        m = d64.smooth_envmap(8, 16) if lname.startswith("map8") else d64.smooth_envmap(64, 128)
        T = golden["env/T"] if lname.endswith("_T") else None
        light = EnvLight(tt(m))
        light.transform = None if T is None else tt(T)
        return light, dict(envmap=m, transform=T, shs=None)
    deg = int(lname[2:])
    shs = np.ascontiguousarray(golden["env/shs"][:, :(deg + 1) ** 2])
    return tt(shs), dict(envmap=None, transform=None, shs=shs)


@pytest.mark.parametrize("lname", ENV_LIGHTS)
@pytest.mark.parametrize("hw", ENV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_env_background(hip_ext, golden, hw, lname):
    """A principal point off the centre and a rotated c2w (the golden file's); the map lookup with and without
    light.transform on a smooth 8x16 and a 64x128 map; SH of degree 0, 3 and 4. c2w as [4,4] and as its [3,3]."""
    import torch

    from relightable3dgaussian_amd.relight import env_background

    H, W = hw
    K, c2w = golden[f"env/K_{H}x{W}"], golden["env/c2w"]
    light, kw = env_light(golden, lname)
    ref = d64.env_background(K, c2w, H, W, dt=np.float64, **kw)
    floor = float(golden[f"env/{H}x{W}/{lname}/floor"])
    env = env_background(light, tt(K), tt(c2w), H, W)
    assert env.shape == (H, W, 3) and env.dtype == torch.float32 and env.is_contiguous()
    tag = f"env {H}x{W} {lname}"
    within(tag, "background", d64.rel_err(env.cpu().numpy(), ref), floor)
    env3 = env_background(light, tt(K), tt(np.ascontiguousarray(c2w[:3, :3])), H, W)
    assert torch.equal(env, env3), tag
    if lname.startswith("map"):
        # EnvLight.direct_light, fed with the direction image, is held to the same bar
        dirs = tt(d64.world_directions(K, c2w, H, W, np.float64).astype(F))
        within(tag, "direct", d64.rel_err(light.direct_light(dirs).cpu().numpy(), ref), floor)


def test_env_background_is_a_bg_image(hip_ext, golden):
    """As the bg of an `over` spec it gives pbr_image(x, o, env)'s composite bit for bit, clamped too."""
    import torch

    from relightable3dgaussian_amd.pbr import pbr_image
    from relightable3dgaussian_amd.relight import env_background

    H, W = 33, 31
    c = case(golden, "r_33x31")
    dev = device_inputs(c, "hwc", 11)
    light, _ = env_light(golden, "map64_T")
    env = env_background(light, tt(golden[f"env/K_{H}x{W}"]), tt(golden["env/c2w"]), H, W)
    f = call([(dev["rgb"], "over", "none"), (dev["rgb"], "over", "clamp"), (dev["rgb"], "over", "aces")], dev["opacity"], env, "f32")
    with torch.no_grad():
        for k, tone in enumerate(("none", "clamp", "aces")):
            want = pbr_image(dev["rgb"], dev["opacity"], env, None, tone, "hwc").cpu().numpy()
            np.testing.assert_array_equal(f[k].view(np.uint32), want.view(np.uint32), err_msg=tone)
