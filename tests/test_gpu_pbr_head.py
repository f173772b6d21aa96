"""The PBR image head and the light regulariser on the GPU (csrc/pbr_head.hip, relightable3dgaussian_amd/pbr.py)
against tests/pbr_ref64.py and tests/golden/pbr_head.npz.

Bars: 4 x max(floor, 2^-24) per output and per case, the floor being the distance of the reference's own float32
evaluation from the float64 one (tests/golden/make_golden_pbr_head.py), in the measure rel_err =
max|got - ref| / max|ref|. "none" and "clamp" are exactly rounded operations and are compared bit for bit with
the reference's float32 images. Every error figure is printed before it is asserted.

Measured on the MI355X (profiles/pbr_head/test_gpu_pbr_head.log): every figure within its
bar; the largest share of a bar is 0.50 (dL/dpbr at 33x31 with gamma = 1: one float32 rounding, 1.2e-7, where
the reference's float32 result happens to be exact).
"""
from __future__ import annotations

import os

import numpy as np
import pytest

from tests import pbr_ref64 as p64
from tests._helpers import tt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
SHAPES = ["r_1x1", "r_1x3", "r_2x2", "r_5x7", "r_16x16", "r_33x31", "r_67x131"]
LAYOUTS = ("hwc", "chw")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "pbr_head.npz"))
    out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def case(golden, name):
    return {k: golden[f"{name}/{k}"] for k in ("pbr", "opacity", "bg", "bgimg", "G", "gamma")}


def lay(a, layout):
    """An "hwc" array in `layout`."""
    return a if layout == "hwc" or a.ndim != 3 else np.ascontiguousarray(np.transpose(a, (2, 0, 1)))


def hwc(t, layout):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return a if layout == "hwc" or a.ndim != 3 else np.transpose(a, (1, 2, 0))


def inputs(c, bgk, layout, views):
    """pbr, opacity, bg on the GPU in `layout`. views: pbr and opacity are views into one [11 H W] feature buffer
    at the S = 11 rasterizer's block offsets (group widths 1, 1, 3, 3, 3: pbr is the third block, at float
    2 H W; opacity takes the second, at float H W), so for odd H W the pixel-major pbr block starts 8 bytes off
    a 16-byte boundary and the opacity block 4 or 12."""
    import torch

    H, W = c["pbr"].shape[:2]
    pbr, opacity = tt(lay(c["pbr"], layout)), tt(lay(c["opacity"], layout))
    if views:
        n = H * W
        feat = torch.full((11 * n,), float("nan"), device="cuda")
        assert feat.data_ptr() % 16 == 0
        feat[2 * n:5 * n] = pbr.reshape(-1)
        feat[n:2 * n] = opacity.reshape(-1)
        pbr, opacity = feat[2 * n:5 * n].view(pbr.shape), feat[n:2 * n].view(opacity.shape)
        assert pbr.is_contiguous() and (pbr.data_ptr() % 16 == 0) == (n % 2 == 0)
    bg = tt(c["bg"]) if bgk == "vec" else tt(lay(c["bgimg"], layout))
    return pbr.detach().requires_grad_(True), opacity.detach().requires_grad_(True), bg


def run(c, bgk, layout, views, tone, gamma=None, grad=True):
    """-> (image, d_pbr, d_opacity, d_gamma) as "hwc" numpy; gradients of sum(image * G)."""
    import torch

    from relightable3dgaussian_amd.pbr import pbr_image

    pbr, opacity, bg = inputs(c, bgk, layout, views)
    g = tt(np.asarray(gamma, F).reshape(1)).requires_grad_(True) if tone == "gamma" else None
    if tone in ("aces", "clamp"):
        with torch.no_grad():
            y = pbr_image(pbr, opacity, bg, None, tone, layout)
        grad = False
    else:
        y = pbr_image(pbr, opacity, bg, g, tone, layout)
    assert y.shape == pbr.shape and y.is_contiguous() and y.dtype == torch.float32
    own = y.untyped_storage().data_ptr()
    assert all(own != t.untyped_storage().data_ptr() for t in (pbr, opacity, bg)), "the image aliases an input"
    if not grad:
        return hwc(y, layout), None, None, None
    y.backward(tt(lay(c["G"], layout)))
    assert pbr.grad.shape == pbr.shape and opacity.grad.shape == opacity.shape
    assert pbr.grad.is_contiguous() and opacity.grad.is_contiguous()
    return hwc(y, layout), hwc(pbr.grad, layout), hwc(opacity.grad, layout), None if g is None else g.grad.cpu().numpy()


def within(tag, what, err, floor):
    b = p64.bar(floor)
    print(f"{tag} {what:16s} {err:.3e} (bar {b:.2e}, floor {float(floor):.2e}, {err / b:5.1%} of the bar)")
    assert err <= b, (tag, what, err, b)


def check_case(golden, name, bgk, layout, views):
    c = case(golden, name)
    tag = f"{name} {layout} bg={bgk} views={int(views)}"
    bg = c["bg"] if bgk == "vec" else c["bgimg"]
    floor = lambda k: golden[f"{name}/floor/{k}"]  # noqa: E731
    full = name in golden["head_full"]
    f64 = (lambda k: golden[f"{name}/{bgk}/f64/{k}"]) if full else None
    skip = p64.near_clamp_bound(c["pbr"], c["opacity"], bg)
    assert skip.mean() <= p64.MAX_LEFT_OUT

    # the exact modes: the reference's float32 bits
    y, d_pbr, d_opacity, _ = run(c, bgk, layout, views, "none")
    np.testing.assert_array_equal(y.view(np.uint32), golden[f"{name}/{bgk}/f32/y_none"].view(np.uint32), err_msg=tag)
    np.testing.assert_array_equal(d_pbr.view(np.uint32), np.asarray(c["G"]).view(np.uint32), err_msg=tag)
    ref = p64.head_backward(c["pbr"], c["opacity"], bg, c["G"], None, "none")
    if full:
        assert p64.rel_err(ref[1], f64("d_opacity_none")) <= 1e-13
    within(tag, "d_opacity_none", p64.rel_err(d_opacity, ref[1]), floor("d_opacity_none"))
    y = run(c, bgk, layout, views, "clamp")[0]
    np.testing.assert_array_equal(y.view(np.uint32), golden[f"{name}/{bgk}/f32/y_clamp"].view(np.uint32), err_msg=tag)

    y = run(c, bgk, layout, views, "aces")[0]
    within(tag, "y_aces", p64.rel_err(y, f64("y_aces") if full else p64.head_forward(c["pbr"], c["opacity"], bg, None, "aces")),
           floor("y_aces"))

    y, d_pbr, d_opacity, d_gamma = run(c, bgk, layout, views, "gamma", c["gamma"])
    if full:
        ref_y, ref = f64("y_gamma"), (f64("d_pbr_gamma"), f64("d_opacity_gamma"), f64("d_gamma"))
    else:
        ref_y = p64.head_forward(c["pbr"], c["opacity"], bg, c["gamma"], "gamma")
        ref = p64.head_backward(c["pbr"], c["opacity"], bg, c["G"], c["gamma"], "gamma")
    within(tag, "y_gamma", p64.rel_err(y, ref_y), floor("y_gamma"))
    within(tag, "d_pbr_gamma", p64.masked_rel_err(d_pbr, ref[0], skip), floor("d_pbr_gamma"))
    within(tag, "d_opacity_gamma", p64.masked_rel_err(d_opacity, ref[1], p64.pixel_mask(skip)), floor("d_opacity_gamma"))
    within(tag, "d_gamma", p64.rel_err(d_gamma, ref[2]), floor("d_gamma"))
    # outside the clamp the gradient is exactly 0, away from the ambiguous band
    x = p64.composite(c["pbr"], c["opacity"], bg)
    out = ((x < p64.LO) | (x > 1.0)) & ~skip
    assert np.all(d_pbr[out] == 0), tag


@pytest.mark.parametrize("views", [False, True], ids=["own", "views"])
@pytest.mark.parametrize("bgk", ["vec", "img"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SHAPES)
def test_head_shapes(hip_ext, golden, name, layout, bgk, views):
    """1x1 the smallest image; 1x3 tail only; 2x2 one full quad; 5x7 odd H W; 16x16 an exact multiple of the quad
    and of a wave; 33x31 odd H W, several waves with a tail; 67x131 several workgroups (9 partial sums)."""
    check_case(golden, name, bgk, layout, views)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("g", [0.45, 1.0, 2.2])
def test_gamma_edges(hip_ext, golden, g, layout):
    """opacity = 1, so x = pbr exactly: x = 1 passes the gradient; nextafter(1, 2) gives y = 1 and gradient 0; lo
    passes; 0 and -0.5 clamp to lo (y = lo ** gamma, gradient 0) and still feed dL/dgamma."""
    name = f"edge_g{g}"
    c = case(golden, name)
    for bgk in ("vec", "img"):
        check_case(golden, name, bgk, layout, False)
    y, d_pbr, d_opacity, d_gamma = run(c, "vec", layout, False, "gamma", c["gamma"])
    lo_g = p64.LO ** float(c["gamma"][0])
    assert np.all(y[0, :2] == 1.0)
    assert np.abs(y[0, 2:] / lo_g - 1).max() <= p64.bar(0), y[0, 2:]  # relative: lo ** gamma is far below max|y| = 1
    assert np.all(d_pbr[0, [0, 2]] != 0) and np.all(d_pbr[0, [1, 3, 4]] == 0)
    # at x = 1: y = 1, the slope is gamma itself, and G * gamma rounds once
    np.testing.assert_array_equal(d_pbr[0, 0], c["G"][0, 0] * c["gamma"][0])
    clamped_only = dict(c, pbr=np.ascontiguousarray(c["pbr"][:, 3:]), opacity=np.ascontiguousarray(c["opacity"][:, 3:]),
                        bgimg=np.ascontiguousarray(c["bgimg"][:, 3:]), G=np.ascontiguousarray(c["G"][:, 3:]))
    _, d_pbr, _, d_gamma = run(clamped_only, "vec", layout, False, "gamma", c["gamma"])
    want = p64.head_backward(clamped_only["pbr"], clamped_only["opacity"], c["bg"], clamped_only["G"], c["gamma"], "gamma")[2]
    assert np.all(d_pbr == 0) and want[0] != 0
    within(f"{name} {layout} clamped only", "d_gamma", p64.rel_err(d_gamma, want), golden[f"{name}/floor/d_gamma"])


def test_gamma_gradient_is_bit_identical_across_runs(hip_ext, golden):
    c = case(golden, "r_67x131")
    for layout in LAYOUTS:
        a = run(c, "img", layout, True, "gamma", c["gamma"])
        b = run(c, "img", layout, True, "gamma", c["gamma"])
        assert a[3].view(np.uint32) == b[3].view(np.uint32) and np.isfinite(a[3]).all() and a[3] != 0
        for u, v in zip(a[:3], b[:3]):
            np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name,px", [("r_5x7", 17), ("r_5x7", 34), ("r_16x16", 130), ("r_33x31", 1022)])
def test_nan_pixel_stays_a_nan_pixel(hip_ext, golden, name, px, layout):
    """One NaN pixel (its pbr, or its opacity) gives NaN at that pixel's three channels and nowhere else, in
    every mode: torch.clamp passes a NaN on, a bare fminf / fmaxf would not."""
    for where in ("pbr", "opacity"):
        c = {k: np.array(v) for k, v in case(golden, name).items()}
        H, W = c["pbr"].shape[:2]
        c[where].reshape(H * W, -1)[px] = np.nan
        want = np.zeros((H * W, 3), bool)
        want[px] = True
        for bgk in ("vec", "img"):
            for tone in p64.TONES:
                y = run(c, bgk, layout, True, tone, c["gamma"], grad=False)[0]
                np.testing.assert_array_equal(np.isnan(y).reshape(H * W, 3), want, err_msg=f"{where} {bgk} {tone}")


def test_forward_only_modes_and_devices_raise(hip_ext, golden):
    import torch

    from relightable3dgaussian_amd.pbr import pbr_image

    c = case(golden, "r_5x7")
    pbr, opacity, bg = inputs(c, "vec", "hwc", False)
    for tone in ("aces", "clamp"):
        with pytest.raises(ValueError, match="forward only"):
            pbr_image(pbr, opacity, bg, None, tone)
        with pytest.raises(ValueError, match="forward only"):
            pbr_image(pbr.detach(), opacity, bg, None, tone)
        assert not pbr_image(pbr.detach(), opacity.detach(), bg, None, tone).requires_grad
    with pytest.raises(ValueError, match="bg is on"):
        pbr_image(pbr, opacity, bg.cpu())
    with pytest.raises(ValueError, match="gamma is on"):
        pbr_image(pbr, opacity, bg, torch.ones(1), "gamma")
    with pytest.raises(ValueError, match="no gradient with respect to bg"):
        pbr_image(pbr, opacity, bg.clone().requires_grad_(True))
    # a gradient only to gamma, and none at all
    g = torch.ones(1, device="cuda", requires_grad=True)
    pbr_image(pbr.detach(), opacity.detach(), bg, g, "gamma").sum().backward()
    assert g.grad is not None and g.grad.shape == (1,)
    with torch.no_grad():
        assert not pbr_image(pbr, opacity, bg).requires_grad


# ---- light_loss ------------------------------------------------------------------------------------------------

def light_inputs(golden, P):
    if P in golden["light"]:
        return golden[f"light_{P}/d"], f"light_{P}"
    assert (P, P) == tuple(golden["light_drawn"])
    return p64.draw_light(P, P), "light_drawn"


@pytest.mark.parametrize("P", [1, 3, 4, 255, 256, 257, 1025, 70001])
def test_light_loss(hip_ext, golden, P):
    """P = 1, 3: tail only; 4: one full lane; 255, 256, 257 and 1025 around a wave of quads and a workgroup (1024
    rows); 70001: 69 partial sums, odd. Rows of equal channels and rows with a channel equal to the mean are in
    every case that has room for them and are compared in full."""
    import torch

    from relightable3dgaussian_amd.pbr import light_loss

    d, name = light_inputs(golden, P)
    skip = p64.ambiguous_sign(d)
    assert skip.mean() <= p64.MAX_LEFT_OUT and not skip[[0, min(1, P - 1), min(2, P - 1)]].any()
    t = tt(d).requires_grad_(True)
    v = light_loss(t)
    assert v.dim() == 0 and v.dtype == torch.float32
    v.backward()
    assert t.grad.shape == (P, 3) and t.grad.is_contiguous()
    v2 = light_loss(tt(d))
    assert v.detach().cpu().numpy().view(np.uint32) == v2.cpu().numpy().view(np.uint32)
    ref_v, ref_g = p64.light_loss(d), p64.light_loss_backward(d)
    if name != "light_drawn":
        assert abs(ref_v - float(golden[f"{name}/f64/value"])) <= 1e-13 * ref_v
    within(f"light P={P}", "value", p64.rel_err(float(v.detach()), ref_v), golden[f"{name}/floor/value"])
    g = t.grad.cpu().numpy()
    within(f"light P={P}", "grad", p64.masked_rel_err(g, ref_g, skip), golden[f"{name}/floor/grad"])
    hand = [0] + ([1, 2] if P >= 3 else []) + ([100, P - 1] if P >= 255 else [])
    np.testing.assert_array_equal(np.sign(g[hand]), np.sign(ref_g[hand]))  # exact zeros where the sign is 0
    if P >= 3:
        assert np.all(g[1] == 0)
    # an upstream factor is read on the device
    t2 = tt(d).requires_grad_(True)
    (light_loss(t2) * torch.tensor(-2.5, device="cuda")).backward()
    within(f"light P={P}", "grad x -2.5", p64.masked_rel_err(t2.grad.cpu().numpy(), -2.5 * ref_g, skip),
           golden[f"{name}/floor/grad"])


def test_light_loss_of_nothing(hip_ext):
    import torch

    from relightable3dgaussian_amd.pbr import light_loss

    t = torch.zeros(0, 3, device="cuda", requires_grad=True)
    v = light_loss(t)
    assert v.dim() == 0 and float(v) == 0.0
    v.backward()
    assert t.grad.shape == (0, 3)


# ---- call sites ------------------------------------------------------------------------------------------------

def test_training_call_site(hip_ext, golden):
    """The rasterizer's 33x31 feature buffer -> pbr_image(tone="gamma") -> l1_ssim_loss(image_layout="hwc") ->
    backward, against pbr_ref64 chained with the suite's float64 image loss (tests/test_image_loss.py ssim64),
    which is what the golden file's call-site entries are (torch autograd in float64). The floors are the
    reference's float32 chain's."""
    import torch

    from relightable3dgaussian_amd.loss import l1_ssim_loss
    from relightable3dgaussian_amd.pbr import pbr_image
    from tests.test_image_loss import ssim64

    c = dict(case(golden, "r_33x31"), gamma=golden["callsite/gamma"])
    gt = golden["callsite/gt"]
    pbr, opacity, bg = inputs(c, "vec", "hwc", True)
    gamma = tt(c["gamma"]).requires_grad_(True)
    image = pbr_image(pbr, opacity, bg, gamma, tone="gamma")
    loss, stats = l1_ssim_loss(image, tt(gt), 0.2, image_layout="hwc")
    loss.backward()

    # the float64 chain once more, from pbr_ref64's forward and backward around the float64 image loss
    y = torch.from_numpy(p64.head_forward(c["pbr"], c["opacity"], c["bg"], c["gamma"], "gamma")).requires_grad_(True)
    g64 = torch.from_numpy(np.array(gt)).double()
    yc = y.permute(2, 0, 1)
    ref_loss = 0.8 * torch.nn.functional.l1_loss(yc, g64) + 0.2 * (1.0 - ssim64(yc, g64))
    up, = torch.autograd.grad(ref_loss, y)
    ref = p64.head_backward(c["pbr"], c["opacity"], c["bg"], up.numpy(), c["gamma"], "gamma")
    skip = p64.near_clamp_bound(c["pbr"], c["opacity"], c["bg"])
    for k, mine, m in zip(("d_pbr", "d_opacity", "d_gamma"), ref, (skip, p64.pixel_mask(skip), None)):
        stored = golden[f"callsite/f64/{k}"]
        e = p64.rel_err(mine, stored) if m is None else p64.masked_rel_err(mine, stored, m)
        assert e <= 1e-9, (k, e)  # two float64 chains
    got = (pbr.grad.cpu().numpy(), opacity.grad.cpu().numpy(), gamma.grad.cpu().numpy())
    assert abs(float(loss) - float(ref_loss)) <= 1e-6
    for k, g, m in zip(("d_pbr", "d_opacity", "d_gamma"), got, (skip, p64.pixel_mask(skip), None)):
        stored = golden[f"callsite/f64/{k}"]
        e = p64.rel_err(g, stored) if m is None else p64.masked_rel_err(g, stored, m)
        within("callsite 33x31", k, e, golden[f"callsite/floor/{k}"])


def test_light_loss_feeds_render_equation_backward(hip_ext):
    """light_loss's gradient as render_equation_backward's dL_ddiffuse_light (P = 257) against the same call fed
    the gradient torch autograd composes from neilf.py:279-281. The two inputs agree to four float32 roundings
    of the largest element (the kernel rounds once; autograd rounds sign / 3P, the three-term sum behind the
    mean, its third and the final sum). The backward is linear in dL_ddiffuse_light and a per-Gaussian output
    is a sum over the three elements of its own row, whose terms may cancel: a factor 4 for that, 16 roundings
    of the largest value. The environment gradient is a float atomic sum over every Gaussian and sample whose
    order differs between any two calls: tests/_helpers.assert_brdf's bar for it, 1e-4 of its scale."""
    import torch
    import torch.nn.functional as Fn

    from relightable3dgaussian_amd import synthetic
    from relightable3dgaussian_amd.pbr import light_loss

    P, Ns = 257, 4
    b = synthetic.brdf_inputs(P, seed=5, S=16)
    args = [tt(b[k]) for k in ("base", "rough", "metal", "normals", "viewdirs", "incidents", "env", "visibility")]
    pbr, dirs, diffuse = hip_ext.render_equation_forward(*args, Ns, True, False)
    assert diffuse.shape == (P, 3)
    d1 = diffuse.detach().clone().requires_grad_(True)
    light_loss(d1).backward()
    d2 = diffuse.detach().clone().requires_grad_(True)
    Fn.l1_loss(d2, d2.mean(-1, keepdim=True).expand_as(d2)).backward()
    assert not p64.ambiguous_sign(diffuse.cpu().numpy()).any()
    assert d1.grad.is_contiguous() and p64.rel_err(d1.grad.cpu().numpy(), d2.grad.cpu().numpy()) <= 4 * p64.ONE_ROUNDING
    zero = torch.zeros(P, 3, device="cuda")
    mine = hip_ext.render_equation_backward(*args, Ns, dirs, zero, d1.grad, False)
    theirs = hip_ext.render_equation_backward(*args, Ns, dirs, zero, d2.grad, False)
    names = ("base_color", "roughness", "metallic", "normals", "viewdirs", "incidents", "direct", "visibility")
    for k, a, r in zip(names, mine, theirs):
        e = p64.rel_err(a.cpu().numpy(), r.cpu().numpy())
        bar = 1e-4 if k == "direct" else 16 * p64.ONE_ROUNDING
        print(f"render_equation_backward d_{k:12s} {e:.3e} (bar {bar:.1e})")
        assert e <= bar, (k, e)
    assert any(float(a.abs().max()) > 0 for a in mine)
