"""Float64 restatement of the PBR image head and the light regulariser (relightable3dgaussian_amd/pbr.py,
include/r3dg_hip.h `r3dg_pbr_head_forward` / `r3dg_light_loss_forward`) and of their gradients, in numpy.

Inputs are float32 arrays, taken to float64 as they are; every operation is then float64. The gamma clamp's
lower bound is the float32 constant torch uses on a float32 tensor, float(np.float32(1e-9)); the ACES constants
are the reference's Python doubles as written (utils/graphics_utils.py:197-201).

Layouts: "hwc" pbr [H,W,3], opacity [H,W,1]; "chw" pbr [3,H,W], opacity [1,H,W]; bg [3] or shaped like pbr.
The measure of every comparison is `rel_err` of tests/relight_ref64.py: max|got - ref| / max|ref|.
"""
from __future__ import annotations

import numpy as np

from tests.relight_ref64 import rel_err  # noqa: F401  (the measure, re-exported)

LO = float(np.float32(1e-9))
ACES_SCALE = 0.666667
TONES = ("none", "gamma", "aces", "clamp")
EDGE = 1e-6          # a pixel whose float64 x lies this close to a clamp bound: its side is ambiguous in float32
SIGN_EDGE = 1e-6     # an element with float64 |d_c - m| <= SIGN_EDGE * max|d|: its sign is ambiguous in float32
MAX_LEFT_OUT = 0.01  # at most this share of a case may be left out of a gradient comparison
ONE_ROUNDING = 2.0 ** -24


def bar(floor):
    """4 x the reference's own float32 distance, and no less than 4 float32 roundings."""
    return 4.0 * max(float(floor), ONE_ROUNDING)


def _bg(bg, layout):
    bg = np.asarray(bg, np.float64)
    if bg.ndim == 1:
        return bg.reshape((1, 1, 3) if layout == "hwc" else (3, 1, 1))
    return bg


def composite(pbr, opacity, bg, layout="hwc"):
    return np.asarray(pbr, np.float64) + (1.0 - np.asarray(opacity, np.float64)) * _bg(bg, layout)


def aces(x):
    s = x * ACES_SCALE
    return (s * (2.51 * s + 0.03)) / (s * (2.43 * s + 0.59) + 0.14)


def head_forward(pbr, opacity, bg, gamma=None, tone="none", layout="hwc"):
    x = composite(pbr, opacity, bg, layout)
    if tone == "none":
        return x
    if tone == "gamma":
        g = float(np.asarray(gamma, np.float64).reshape(-1)[0])
        with np.errstate(invalid="ignore"):
            xc = np.where(np.isnan(x), x, np.clip(x, LO, 1.0))
            return xc ** g
    if tone == "aces":
        return aces(x)
    if tone == "clamp":
        return np.where(np.isnan(x), x, np.clip(x, 0.0, 1.0))
    raise ValueError(tone)


def head_backward(pbr, opacity, bg, upstream, gamma=None, tone="none", layout="hwc"):
    """-> (dL/dpbr, dL/dopacity, dL/dgamma or None) for the upstream G in the output's layout."""
    x = composite(pbr, opacity, bg, layout)
    G = np.asarray(upstream, np.float64)
    d_gamma = None
    if tone == "none":
        dx = G.copy()
    elif tone == "gamma":
        g = float(np.asarray(gamma, np.float64).reshape(-1)[0])
        xc = np.clip(x, LO, 1.0)
        inside = (x >= LO) & (x <= 1.0)
        dx = np.where(inside, G * g * xc ** (g - 1.0), 0.0)
        d_gamma = np.array([(G * xc ** g * np.log(xc)).sum()])
    else:
        raise ValueError(f"tone {tone!r} is forward only")
    d_opacity = -(dx * _bg(bg, layout)).sum(2 if layout == "hwc" else 0, keepdims=True)
    return dx, d_opacity, d_gamma


def near_clamp_bound(pbr, opacity, bg, layout="hwc"):
    """Bool mask in pbr's shape: float64 x within EDGE of lo or of 1 but not ON the bound (an x that is a bound
    exactly, as the hand-made edge pixels are, is not ambiguous: opacity = 1 makes x = pbr in both precisions)."""
    x = composite(pbr, opacity, bg, layout)
    exact = (np.asarray(opacity, np.float64) == 1.0) & np.ones_like(x, bool)
    return ((np.abs(x - LO) <= EDGE) | (np.abs(x - 1.0) <= EDGE)) & ~exact


def pixel_mask(elem_mask, layout="hwc"):
    """A pixel is left out of d_opacity when any of its channels is."""
    return elem_mask.any(2 if layout == "hwc" else 0, keepdims=True)


def light_loss(d):
    d = np.asarray(d, np.float64)
    if d.shape[0] == 0:
        return 0.0
    m = d.sum(1, keepdims=True) / 3.0
    return float(np.abs(d - m).sum() / d.size)


def light_loss_backward(d, upstream=1.0):
    d = np.asarray(d, np.float64)
    if d.shape[0] == 0:
        return np.zeros((0, 3))
    s = np.sign(d - d.sum(1, keepdims=True) / 3.0)
    return float(upstream) * (s - s.sum(1, keepdims=True) / 3.0) / d.size


def ambiguous_sign(d):
    """[P,3] bool: the rows with an element of 0 < float64 |d_c - m| <= SIGN_EDGE * max|d| (a sign reaches the
    whole row through the mean's gradient; an exact zero is not ambiguous: a row of equal channels, or a
    channel equal to an exactly representable mean)."""
    d = np.asarray(d, np.float64)
    if d.size == 0:
        return np.zeros(d.shape, bool)
    a = np.abs(d - d.sum(1, keepdims=True) / 3.0)
    rows = ((a > 0) & (a <= SIGN_EDGE * np.abs(d).max())).any(1, keepdims=True)
    return np.broadcast_to(rows, d.shape).copy()


def draw_light(P, seed):
    """diffuse_light [P,3] float32 in [0, 2) with the hand-made rows: (1, 2, 3) and a rotation of it (one channel
    IS the row mean, exactly, in float32 and in float64), and rows of three equal channels whose mean is exact
    in both precisions (0.5, 0.75: 3 a and its third are representable)."""
    d = np.random.default_rng(seed).uniform(0, 2, (P, 3)).astype(np.float32)
    if P >= 1:
        d[0] = (1, 2, 3)
    if P >= 3:
        d[1], d[2] = (0.5, 0.5, 0.5), (3, 1, 2)
    if P >= 255:
        d[100], d[P - 1] = (0.75, 0.75, 0.75), (2, 3, 1)
    return d


def masked_rel_err(got, ref, skip):
    """rel_err with the skipped elements' error taken as 0 (the denominator keeps every element)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape == skip.shape, (got.shape, ref.shape, skip.shape)
    return rel_err(np.where(skip, ref, got), ref)
