"""Numpy restatement of the display and capture head (relightable3dgaussian_amd/display.py, include/r3dg_hip.h
`r3dg_display_frame`) and of the environment background (`relight.env_background`, `r3dg_env_background`).

Every function takes `dt`: np.float32 performs the header's operations one rounding at a time, constants
rounded to float32 where they meet the array, which is what torch does on float32 tensors and what the kernel
does (built without contraction); np.float64 takes the float32 inputs to float64 as they are and uses the
reference's Python doubles. tests/golden/make_golden_display.py asserts that the float32 mode reproduces the
reference's float32 torch bits for every exact case (every mode, tones "none" and "clamp", both encodings) and
that the float64 mode agrees with torch float64 to 1e-13.

Sources are "hwc" [H,W,1|3] or "chw" [1|3,H,W]; results are [H,W,3]. The measure of every inexact comparison is
`rel_err` of tests/relight_ref64.py, max|got - ref| / max|ref|, and the bar `pbr_ref64.bar`.
"""
from __future__ import annotations

import numpy as np

from tests.pbr_ref64 import MAX_LEFT_OUT, ONE_ROUNDING, bar  # noqa: F401  (re-exported)
from tests.relight_ref64 import rel_err  # noqa: F401

MODES = ("plain", "over", "normal_over", "normal_mask", "range", "count")
TONES = ("none", "clamp", "aces")
C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435]
C4 = [2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431,
      -0.6690465435572892, 0.47308734787878004, -1.7701307697799304, 0.6258357354491761]


def hwc3(source, layout="hwc"):
    """[H,W,3] from a source in `layout`: a one-channel source gives three equal channels."""
    s = np.asarray(source)
    if layout == "chw":
        s = np.transpose(s, (1, 2, 0))
    return np.repeat(s, 3, 2) if s.shape[2] == 1 else s


def aces(x, dt):
    c = dt  # the constants in the array's type
    s = x * c(0.666667)
    return (s * (c(2.51) * s + c(0.03))) / (s * (c(2.43) * s + c(0.59)) + c(0.14))


def clamp01(y):
    """torch.clamp(y, 0, 1): a NaN stays NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(y), y, np.clip(y, 0, 1)).astype(y.dtype)


def frame(source, mode, tone, opacity=None, bg=None, layout="hwc", dt=np.float32):
    """y [H,W,3] in dt for one spec. bg: a number, [3] or [H,W,3]."""
    s = hwc3(source, layout)
    if mode == "count":
        assert s.dtype == np.int32
        y = np.minimum(s, 1000).astype(dt) / dt(1000)
    else:
        assert s.dtype == np.float32
        s = s.astype(dt)
        o = None if opacity is None else np.asarray(opacity, np.float32).astype(dt)
        # a Python number meets the tensor in the tensor's type; arrays are float32 data
        b = None if bg is None else dt(bg) if isinstance(bg, (int, float)) else np.asarray(bg, np.float32).astype(dt)
        with np.errstate(invalid="ignore", divide="ignore"):
            if mode == "plain":
                y = s
            elif mode == "over":
                y = s + (dt(1) - o) * b
            elif mode == "normal_over":
                y = (s * dt(0.5) + dt(0.5)) + (dt(1) - o) * b
            elif mode == "normal_mask":
                y = s * dt(0.5) + dt(0.5) * o
            elif mode == "range":
                mn, mx = s.min(), s.max()  # numpy's propagate a NaN, as torch's
                y = (s - mn) / (mx - mn)
            else:
                raise ValueError(mode)
    assert y.dtype == dt
    if tone == "clamp":
        y = clamp01(y)
    elif tone == "aces":
        with np.errstate(invalid="ignore", divide="ignore"):
            y = aces(y, dt)
    elif tone != "none":
        raise ValueError(tone)
    assert y.dtype == dt
    return y


def quantise(y):
    """save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8) in y's type; a NaN gives 0."""
    dt = y.dtype.type
    with np.errstate(invalid="ignore"):
        t = y * dt(255)
        t = t + dt(0.5)
        t = np.where(np.isnan(t), dt(0), np.clip(t, 0, 255))
    return np.floor(t).astype(np.uint8)


def near_level(y64, b):
    """[H,W,3] bool: the elements whose float64 y * 255 + 0.5 lies within 255 * b * max|y| of an integer, the only
    ones whose byte may differ (by 1) between an evaluation within the bar b and the float64 one."""
    t = np.asarray(y64, np.float64) * 255.0 + 0.5
    return np.abs(t - np.round(t)) <= 255.0 * b * float(np.abs(y64).max())


# The views every case is run through: name -> (source, mode, bg kind). Sources of a case: "rgb" [H,W,3], "gray"
# [H,W,1], "count" int32 [H,W,1]; bg kinds: "vec" [3], "num" a Python number, "img" [H,W,3].
VIEWS = {"plain3": ("rgb", "plain", None), "plain1": ("gray", "plain", None), "over3_vec": ("rgb", "over", "vec"),
         "over1_num": ("gray", "over", "num"), "over3_img": ("rgb", "over", "img"),
         "normal_over": ("rgb", "normal_over", "vec"), "normal_mask": ("rgb", "normal_mask", None),
         "range1": ("gray", "range", None), "range3": ("rgb", "range", None), "count": ("count", "count", None)}
ACES_VIEWS = ("plain3", "over3_vec")
BG_NUM = 0.7
RANGE_VARIANTS = ("first", "last", "last_workgroup", "nan", "constant")


def view_bg(c, kind):
    return {None: None, "vec": c["bg"], "num": BG_NUM, "img": c["bgimg"]}[kind]


def view(c, name, tone, dt=np.float32):
    """y [H,W,3] of view `name` of case c = {rgb, gray, count, opacity, bg, bgimg}."""
    src, mode, kind = VIEWS[name]
    return frame(c[src], mode, tone, c["opacity"], view_bg(c, kind), "hwc", dt)


def range_variant(gray, kind):
    """A copy of a one-channel source with the `range` mode's edge: the extrema (-3 and 5, outside the drawn
    values) in the first pixel, in the last pixel (the tail lane's when H W is no multiple of 4), in the last
    workgroup of the pre-pass (the last 1024-element block, away from its end); one NaN; a constant image."""
    g = np.array(gray, np.float32)
    f = g.reshape(-1)
    n = f.size
    if kind == "first":
        f[0] = -3.0
        if n > 1:
            f[n // 2] = 5.0
    elif kind == "last":
        f[n - 1] = 5.0
        if n > 1:
            f[n // 2] = -3.0
    elif kind == "last_workgroup":
        lo = ((n - 1) // 1024) * 1024
        f[lo] = -3.0
        f[lo + (n - 1 - lo) // 2] = 5.0
    elif kind == "nan":
        f[n // 3] = np.nan
    elif kind == "constant":
        f[:] = 0.375
    else:
        raise ValueError(kind)
    return g


# ---- the environment background --------------------------------------------------------------------------------

def world_directions(K, c2w, H, W, dt=np.float64):
    """scene/cameras.py:87-99 as [H,W,3]: F.normalize(((u - cx) / fx, (v - cy) / fy, 1)), then c2w[:3,:3] @ d."""
    K, R = np.asarray(K, np.float32).astype(dt), np.asarray(c2w, np.float32).astype(dt)[:3, :3]
    v, u = np.meshgrid(np.arange(H).astype(dt), np.arange(W).astype(dt), indexing="ij")
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)
    nrm = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    d = d / np.maximum(nrm, dt(1e-12))[..., None]
    w = [(R[i, 0] * d[..., 0] + R[i, 1] * d[..., 1]) + R[i, 2] * d[..., 2] for i in range(3)]
    return np.stack(w, -1).astype(dt)


def envmap_lookup(dirs, envmap, transform=None, dt=np.float64):
    """EnvLight.direct_light (scene/envmap.py:31-48; nvdiffrast's linear filter with wrap) for dirs [...,3]."""
    d = np.asarray(dirs).astype(dt)
    m = np.asarray(envmap, np.float32).astype(dt)
    if transform is not None:
        T = np.asarray(transform, np.float32).astype(dt)
        d = np.stack([(T[i, 0] * d[..., 0] + T[i, 1] * d[..., 1]) + T[i, 2] * d[..., 2] for i in range(3)], -1)
    pi = dt(np.pi)
    tu = np.arctan2(d[..., 0], d[..., 1]) / (dt(2) * pi) + dt(0.5)
    tv = np.arccos(np.clip(d[..., 2], -1, 1)) / pi
    Hm, Wm = m.shape[:2]

    def axis(t, n):
        t = t - np.floor(t)
        x = t * dt(n) - dt(0.5)
        x0 = np.floor(x)
        i0 = x0.astype(np.int64)
        return i0 % n, (i0 + 1) % n, (x - x0)[..., None]

    x0, x1, fx = axis(tu, Wm)
    y0, y1, fy = axis(tv, Hm)
    one = dt(1)
    out = (m[y0, x0] * ((one - fx) * (one - fy)) + m[y0, x1] * (fx * (one - fy)) + m[y1, x0] * ((one - fx) * fy) +
           m[y1, x1] * (fx * fy))
    return out.astype(dt)


def sh_basis(d, M, dt):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    c = dt
    b = [np.full_like(x, C0), -c(C1) * y, c(C1) * z, -c(C1) * x,
         c(C2[0]) * xy, c(C2[1]) * yz, c(C2[2]) * (c(2) * zz - xx - yy), c(C2[3]) * xz, c(C2[4]) * (xx - yy),
         c(C3[0]) * y * (c(3) * xx - yy), c(C3[1]) * xy * z, c(C3[2]) * y * (c(4) * zz - xx - yy),
         c(C3[3]) * z * (c(2) * zz - c(3) * xx - c(3) * yy), c(C3[4]) * x * (c(4) * zz - xx - yy),
         c(C3[5]) * z * (xx - yy), c(C3[6]) * x * (xx - c(3) * yy),
         c(C4[0]) * xy * (xx - yy), c(C4[1]) * yz * (c(3) * xx - yy), c(C4[2]) * xy * (c(7) * zz - c(1)),
         c(C4[3]) * yz * (c(7) * zz - c(3)), c(C4[4]) * (zz * (c(35) * zz - c(30)) + c(3)),
         c(C4[5]) * xz * (c(7) * zz - c(3)), c(C4[6]) * (xx - yy) * (c(7) * zz - c(1)),
         c(C4[7]) * xz * (xx - c(3) * yy), c(C4[8]) * (xx * (xx - c(3) * yy) - yy * (c(3) * xx - yy))]
    return np.stack(b[:M], -1).astype(dt)


def env_sh(dirs, shs, dt=np.float64):
    """clamp_min(eval_sh(deg, shs, d) + 0.5, 0) of shs [1,M,3] (neilf_composite.py:212-213)."""
    s = np.asarray(shs, np.float32).astype(dt).reshape(-1, 3)
    d = np.asarray(dirs).astype(dt)
    Y = sh_basis(d, s.shape[0], dt)
    acc = Y[..., 0:1] * s[0]
    for k in range(1, s.shape[0]):
        acc = acc + Y[..., k:k + 1] * s[k]
    return np.maximum(acc + dt(0.5), dt(0)).astype(dt)


def env_background(K, c2w, H, W, envmap=None, transform=None, shs=None, dt=np.float64):
    d = world_directions(K, c2w, H, W, dt)
    return envmap_lookup(d, envmap, transform, dt) if envmap is not None else env_sh(d, shs, dt)


# ---- deterministic inputs that need no storage (exact arithmetic only) -----------------------------------------

def smooth_envmap(h, w):
    """[h,w,3] float32, a sum of two triangle waves per channel, periodic in both axes, every value a multiple of
    1/64: formed with exact arithmetic, so every machine draws the same bits."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    tri = lambda t, p: np.abs((t % p) - p // 2) / (p // 2)  # noqa: E731  in [0, 1], period p (even)
    m = np.stack([0.25 + tri(x * (c + 1), w) * 1.5 + tri(y * 2 + c * (h // 4), 2 * h) * (0.5 + 0.25 * c) for c in range(3)], -1)
    return np.ascontiguousarray((np.round(m * 64) / 64).astype(np.float32))


def rotation(ax, ay, az):
    """A float32 [3,3] rotation from three angles (float64 products, rounded once)."""
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float32)
