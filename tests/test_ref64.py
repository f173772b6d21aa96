"""The oracle's raster backward against float64 autograd restatements (tests/ref64.py), on the scenes of
tests/_edge_scenes.py: the frustum-edge clamp of the 2D covariance, scale_modifier != 1, un-normalised
quaternions, SH degrees 0-2 with 16 coefficients, the alpha cap and a coloured background. CPU only.

Bars. The bar of a gradient is not taken from the oracle: the restatement runs once in float32 and once
in float64 on the same inputs, and the bar is |d| <= 1e-4 |ref| + frac max|ref| with frac = 4 x the larger
of max|f32 - f64| / max|f64| and the fraction that difference needs at rel 1e-4 -- the operation's own f32
rounding floor, x 4 because the oracle's operation order differs from torch's. That frac must not exceed
the gradient's entry in GRAD_BARS (tests/test_gpu_parity.py), or the scene is too ill-conditioned to pin
anything. dL_dconic has no entry there; it is capped at dL_dcov3D's, the gradient it turns into. The
measured floors and bars are printed (run with -s) and recorded in DESIGN.md §5. Images: 1e-5 absolute.

Pixels with a (pixel, Gaussian) pair within 1e-5 relative of a skip threshold (alpha = 1/255, power = 0,
T = 1e-4) in float64 may take the other branch in f32: their upstream gradients are zeroed on both sides,
and at most 1 % of the pixels of a scene may be left out this way.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import oracle
from tests import _edge_scenes as es
from tests import ref64
from tests.test_gpu_parity import GRAD_BARS

REL = 1e-4
IMG_ATOL = 1e-5
BLEND_KEYS = ["dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dfeatures"]
GAUSS_KEYS = ["dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations", "dL_dsh"]
CAPS = dict({k: v[1] for k, v in GRAD_BARS.items()}, dL_dconic=GRAD_BARS["dL_dcov3D"][1])


def _blend_inputs(c, o):
    return dict(W=c.cam.width, H=c.cam.height, ranges=o["ranges"], point_list=o["point_list"], means2D=o["means2D"],
                depths=o["depths"], conic=o["conic_opacity"][:, :3], opacity=o["conic_opacity"][:, 3],
                colors=o["rgb"], features=o["_in"]["features"], bg=c.bg)


def _gauss_inputs(c, o, go):
    sc = c.scene
    return dict(cam=c.cam, visible=o["radii"] > 0, dL_dmean2D=go["dL_dmeans2D"], dL_dconic=go["dL_dconic"],
                dL_dcolor=go["dL_dcolors"], means3D=sc.means3D, scales=sc.scales, rotations=sc.rotations, sh=sc.sh,
                degree=c.degree, scale_modifier=c.scale_modifier)


@functools.lru_cache(maxsize=None)
def _run(name):
    """Everything the tests of one scene share: the oracle's forward and backward (upstream gradients zeroed on
    the left-out pixels), the restatements in float64 and float32 on the same inputs. Read-only."""
    c = es.case(name)
    o, up, go = es.oracle_run(name)
    fwd = ref64.tile_blend(**_blend_inputs(c, o))
    near = fwd["near"]
    if near.any():
        keep = (~near).astype(np.float32)
        up = (up[0] * keep[None], up[1] * keep.reshape(-1), up[2] * keep.reshape(-1), up[3] * keep[None])
        go = oracle.rasterize_backward(o, *up)
    b64 = ref64.tile_blend(**_blend_inputs(c, o), upstream=up)
    b32 = ref64.tile_blend(**_blend_inputs(c, o), upstream=up, dtype=torch.float32)
    g64 = ref64.per_gaussian_backward(**_gauss_inputs(c, o, go))
    g32 = ref64.per_gaussian_backward(**_gauss_inputs(c, o, go), dtype=torch.float32)
    return dict(case=c, o=o, up=up, go=go, fwd=fwd, b64=b64, b32=b32, g64=g64, g32=g32,
                left_out=float(near.mean()))


def _need(d, ref, m):
    """(max |d| / max|ref|, the frac that |d| <= REL |ref| + frac max|ref| needs)."""
    if m == 0.0:
        return float(d.max(initial=0.0)), float(d.max(initial=0.0))
    return float(d.max(initial=0.0)) / m, float(max((d - REL * np.abs(ref)).max(initial=0.0), 0.0)) / m


def bar_of(key, r32, r64):
    """The bar's frac for one gradient from the restatement's own f32 rounding (module docstring)."""
    r64 = np.asarray(r64, np.float64)
    m = float(np.abs(r64).max(initial=0.0))
    floor, need = _need(np.abs(np.asarray(r32, np.float64) - r64), r64, m)
    return floor, need, 4.0 * max(floor, need)


def excess(got, r64, frac):
    """The worst |got - ref| / (REL |ref| + frac max|ref|): <= 1 passes."""
    got, r64 = np.asarray(got, np.float64), np.asarray(r64, np.float64)
    m = float(np.abs(r64).max(initial=0.0))
    if got.size == 0 or m == 0.0:
        return float(np.abs(got - r64).max(initial=0.0) > 0)
    return float((np.abs(got - r64) / (REL * np.abs(r64) + frac * m)).max())


def _hold(name, keys, got, r32, r64):
    worst = {}
    for k in keys:
        if not np.any(r64[k]) and not np.any(got[k]):
            continue
        floor, need, frac = bar_of(k, r32[k], r64[k])
        f, n = _need(np.abs(got[k].astype(np.float64) - r64[k]), r64[k], float(np.abs(r64[k]).max()))
        worst[k] = excess(got[k], r64[k], frac)
        print(f"ref64 {name} {k}: f32 floor {floor:.2e} (at rel 1e-4: {need:.2e}) -> bar frac {frac:.2e} "
              f"(GRAD_BARS {CAPS[k]:.1e}); oracle {f:.2e} (at rel 1e-4: {n:.2e}), worst |d| / bar {worst[k]:.2f}")
        assert frac <= CAPS[k], f"{name} {k}: the f32 floor's bar {frac:.2e} exceeds GRAD_BARS {CAPS[k]:.1e}"
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, f"{name}: oracle outside the bar (worst |d| / bar): {bad}"


@pytest.mark.parametrize("name", es.NAMES)
def test_scene_covers_its_branch(name):
    r = _run(name)
    es.covers(name, r["o"], r["go"], r["fwd"])
    print(f"{name}: {100 * r['left_out']:.3f} % of the pixels left out (a pair within 1e-5 of a skip threshold)")
    assert r["left_out"] <= 0.01


@pytest.mark.parametrize("name", es.NAMES)
def test_forward_matches_restatement(name):
    r = _run(name)
    c, o, f = r["case"], r["o"], r["fwd"]
    H, W, S = c.cam.height, c.cam.width, c.S
    a, m = oracle.feature_layout(S, H * W)
    pix = np.arange(H * W)
    feat = np.stack([o["feature"].reshape(-1)[a[ch] + pix * m[ch]] for ch in range(S)], 1).reshape(H, W, S)
    got = {"color": o["color"], "opacity": o["opacity"][..., 0], "depth": o["depth"][..., 0], "feature": feat,
           "final_T": o["final_T"].reshape(H, W)}
    for k, v in got.items():
        d = float(np.abs(v.astype(np.float64) - f[k]).max())
        print(f"ref64 {name} image {k}: max |d| {d:.2e}")
        assert d <= IMG_ATOL, (k, d)
    # the per-Gaussian forward: f32 rounding of a ~30-operation chain, 1e-5 of the quantity's scale
    sc = c.scene
    vis = o["radii"] > 0
    with torch.no_grad():
        p = ref64.per_gaussian(c.cam, sc.means3D[vis], sc.scales[vis], sc.rotations[vis], sc.sh[vis], c.degree,
                               c.scale_modifier)
    ndc = p["ndc"].numpy()
    px = np.stack([((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5], 1)
    for k, got_k, ref_k in [("means2D", o["means2D"][vis], px), ("depths", o["depths"][vis], p["depth"].numpy()),
                            ("conic", o["conic_opacity"][vis, :3], p["conic"].numpy()),
                            ("rgb", o["rgb"][vis], p["rgb"].numpy())]:
        d = np.abs(got_k.astype(np.float64) - ref_k)
        tol = 1e-5 * np.maximum(np.abs(ref_k), float(np.abs(ref_k).max()) * 1e-1)
        print(f"ref64 {name} {k}: max |d| {d.max():.2e} (max |ref| {np.abs(ref_k).max():.2e})")
        assert np.all(d <= tol), (k, float((d / tol).max()))


@pytest.mark.parametrize("name", es.NAMES)
def test_blend_backward_matches_restatement(name):
    r = _run(name)
    _hold(name, BLEND_KEYS, r["go"], r["b32"], r["b64"])


@pytest.mark.parametrize("name", es.NAMES)
def test_per_gaussian_backward_matches_restatement(name):
    r = _run(name)
    _hold(name, GAUSS_KEYS, r["go"], r["g32"], r["g64"])


# ------------------------------------------------------------------------------------------------
# the bars can fail: one convention of the reference replaced by a plausible wrong one
# ------------------------------------------------------------------------------------------------
def _must_fail(tag, keys, got, r32, r64, mutated):
    """The oracle meets the bar against the restatement and misses it against the mutated restatement on at
    least one of `keys`; prints by how much."""
    out = {}
    for k in keys:
        frac = bar_of(k, r32[k], r64[k])[2]
        assert excess(got[k], r64[k], frac) <= 1.0, (tag, k)
        out[k] = excess(got[k], mutated[k], frac)
        print(f"mutation {tag} {k}: worst |d| / bar {out[k]:.1f} (the unmutated restatement: "
              f"{excess(got[k], r64[k], frac):.2f})")
    assert max(out.values()) > 1.0, (tag, out)


@pytest.mark.parametrize("clamp", ["autograd", "off"])
def test_mutated_clamp_fails_bar(clamp):
    """Differentiating through the clamp, or leaving it out, must fail dL_dmeans3D on frustum_edge."""
    r = _run("frustum_edge")
    mut = ref64.per_gaussian_backward(**_gauss_inputs(r["case"], r["o"], r["go"]), clamp=clamp)
    _must_fail(f"clamp={clamp}", ["dL_dmeans3D"], r["go"], r["g32"], r["g64"], mut)


@pytest.mark.parametrize("name", ["modifier-0.6", "modifier-1.7"])
def test_mutated_scale_gradient_fails_bar(name):
    """dL_dscales with respect to `scale` instead of `mod * scale` must fail."""
    r = _run(name)
    mut = ref64.per_gaussian_backward(**_gauss_inputs(r["case"], r["o"], r["go"]), scale_grad="scale")
    _must_fail(f"scale_grad=scale {name}", ["dL_dscales"], r["go"], r["g32"], r["g64"], mut)


def test_mutated_alpha_cap_fails_bar():
    """A blend without the 0.99 cap must fail a blend gradient on `opaque`."""
    r = _run("opaque")
    mut = ref64.tile_blend(**_blend_inputs(r["case"], r["o"]), upstream=r["up"], alpha_cap=False)
    _must_fail("alpha_cap=False", BLEND_KEYS, r["go"], r["b32"], r["b64"], mut)


def test_mutated_background_fails_bar():
    """Two background channels swapped must fail dL_dopacity on the coloured background."""
    r = _run("coloured_bg-colour")
    inp = _blend_inputs(r["case"], r["o"])
    inp["bg"] = (inp["bg"][1], inp["bg"][0], inp["bg"][2])
    mut = ref64.tile_blend(**inp, upstream=r["up"])
    _must_fail("bg swapped", ["dL_dopacity"], r["go"], r["b32"], r["b64"], mut)
