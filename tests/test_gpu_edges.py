"""GPU parity on the branches no other scene reaches (tests/_edge_scenes.py): the frustum-edge clamp of
the 2D covariance, scale_modifier != 1 with un-normalised quaternions, SH degrees 0-2 with 16
coefficients, the alpha cap min(0.99, opacity * G) and the background term of the backward. The HIP
path against the oracle, which tests/test_ref64.py holds to float64 autograd on the same scenes.

Bars as in tests/test_gpu_parity.py: keys, point list, ranges, radii, n_contrib and final_T bit-exact,
images within IMG_ATOL, gradients at GRAD_BARS. On the clamp scenes the per-Gaussian gradients are
checked once more on the clamped Gaussians alone (max|ref| over that subset): their gradients are a
few per cent of the scene's largest, which the whole-array fraction would cover for.
"""
from __future__ import annotations

import contextlib

import numpy as np
import pytest

import oracle
from tests import _edge_scenes as es
from tests._helpers import hip_backward, hip_forward, lib_options, rows_reduction, upstream_grads
from tests.test_gpu_parity import _check_forward, grad_check

pytestmark = pytest.mark.gpu

GRADS = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dfeatures", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
         "dL_dscales", "dL_drotations"]
CLAMP_SCENES = ["frustum_edge", "modifier-0.6", "modifier-1.7"]
BLEND_SCENES = ["opaque", "coloured_bg-colour", "coloured_bg-black"]


def _forward(hip_ext, c, use_cov=False):
    return hip_forward(hip_ext, c.scene, c.cam, S=c.S, degree=c.degree, bg=c.bg, use_cov=use_cov,
                       scale_modifier=c.scale_modifier)


def _check_backward(tag, name, gh, go, o, keys=GRADS):
    grad_check(tag, gh, go, keys)
    if name in CLAMP_SCENES:
        cx, cy = es.clamped_xy(es.case(name))
        sub = (cx | cy) & (o["radii"] > 0)
        assert int(sub.sum()) >= 20
        per_gaussian = [k for k in ["dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations"] if k in keys]
        grad_check(f"{tag} clamped only", {k: gh[k][sub] for k in per_gaussian}, {k: go[k][sub] for k in per_gaussian},
                   per_gaussian)


@pytest.mark.parametrize("name", es.NAMES)
def test_forward_matches_oracle(hip_ext, name):
    c = es.case(name)
    o, _, go = es.oracle_run(name)
    if name != "opaque":  # its check needs the restatement's masks: tests/test_ref64.py asserts it
        es.covers(name, o, go)
    _check_forward(_forward(hip_ext, c), o, c.S)


@pytest.mark.parametrize("reduce", ["default", "rows"])
@pytest.mark.parametrize("name", es.NAMES)
def test_backward_matches_oracle(hip_ext, name, reduce):
    c = es.case(name)
    o, up, go = es.oracle_run(name)
    with rows_reduction() if reduce == "rows" else contextlib.nullcontext():
        gh = hip_backward(hip_ext, _forward(hip_ext, c), *up)
    _check_backward(f"edges {name} {reduce}", name, gh, go, o)


@pytest.mark.parametrize("name", BLEND_SCENES)
def test_backward_dpp_variant_matches_oracle(hip_ext, name):
    """The DPP wave-reduction variant of the backward blend has its own alpha cap and background term."""
    c = es.case(name)
    o, up, go = es.oracle_run(name)
    with lib_options(test_bwd_dpp=1):
        gh = hip_backward(hip_ext, _forward(hip_ext, c), *up)
    _check_backward(f"edges {name} dpp", name, gh, go, o)


@pytest.mark.parametrize("name", CLAMP_SCENES)
def test_precomputed_cov_matches_oracle(hip_ext, name):
    c = es.case(name)
    o, up, go = es.oracle_run(name, use_cov=True)
    h = _forward(hip_ext, c, use_cov=True)
    _check_forward(h, o, c.S)
    gh = hip_backward(hip_ext, h, *up)
    _check_backward(f"edges {name} cov", name, gh, go, o,
                    ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dfeatures", "dL_dmeans3D", "dL_dcov3D", "dL_dsh"])
    assert np.all(gh["dL_dscales"] == 0) and np.all(gh["dL_drotations"] == 0)


def test_autograd_wrapper_modifier_and_background(hip_ext):
    """GaussianRasterizer with scale_modifier = 0.6 and a coloured background: the settings reach both the
    forward and the backward call."""
    import torch

    from relightable3dgaussian_amd.r3dg_rasterization import GaussianRasterizer, settings_from_camera

    c = es.case("modifier-0.6")
    scene, cam = c.scene, c.cam
    dev = "cuda"
    rast = GaussianRasterizer(settings_from_camera(cam, es.COLOURED, scale_modifier=0.6))
    t = lambda a: torch.tensor(a, device=dev, requires_grad=True)  # noqa: E731
    means3D, opac, feats = t(scene.means3D), t(scene.opacity), t(scene.features)
    shs, scales, rots = t(scene.sh), t(scene.scales), t(scene.rotations)
    means2D = torch.zeros_like(means3D, requires_grad=True)
    out = rast(means3D=means3D, means2D=means2D, opacities=opac, shs=shs, scales=scales, rotations=rots,
               features=feats)
    num_rendered, n_contrib, color, opacity, depth, stencil, feature, shader, normal, xyz, radii = out
    H, W = cam.height, cam.width
    dc, do, dd, df = upstream_grads(H, W, 11, seed=16)
    loss = (color * torch.tensor(dc.transpose(1, 2, 0), device=dev)).sum() + \
        (opacity * torch.tensor(do.reshape(H, W, 1), device=dev)).sum() + \
        (depth * torch.tensor(dd.reshape(H, W, 1), device=dev)).sum()
    col = 0
    flat = feature.reshape(-1)
    for n in [1, 1, 3, 3, 3]:  # the block layout of S = 11
        blk = flat[H * W * col:H * W * (col + n)].view(H * W, n)
        loss = loss + (blk * torch.tensor(df[col:col + n].reshape(n, H * W).T.copy(), device=dev)).sum()
        col += n
    loss.backward()
    o = oracle.rasterize_forward(cam, scene.means3D, scene.opacity, scene.features, sh=scene.sh, scales=scene.scales,
                                 rotations=scene.rotations, bg=es.COLOURED, scale_modifier=0.6)
    np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])
    np.testing.assert_allclose(color.detach().cpu().numpy(), o["color"], rtol=0, atol=1e-4)
    go = oracle.rasterize_backward(o, dc, do, dd, df)
    got = {"dL_dmeans3D": means3D.grad, "dL_dmeans2D": means2D.grad, "dL_dfeatures": feats.grad, "dL_dsh": shs.grad,
           "dL_dopacity": opac.grad, "dL_dscales": scales.grad, "dL_drotations": rots.grad}
    _check_backward("edges autograd", "modifier-0.6", {k: v.cpu().numpy() for k, v in got.items()}, go, o, list(got))
