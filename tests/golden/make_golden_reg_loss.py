"""Golden vectors for the depth, mask-entropy, normal, base-colour and smoothness terms of calculate_loss
(gaussian_renderer/neilf.py:233-321), from the REFERENCE's own utils/loss_utils.py where it can be loaded
(CPU container; bilateral_smooth_loss and cal_gradient run on CPU tensors). gaussian_renderer/neilf.py imports
the native modules at the top and cannot be imported here, so the other five terms are evaluated from their
formulas, restated in this project's own words with the reference's sequence of tensor operations.

  reg_loss.npz   names [n], lambdas [8] (the weights of the gradient maps, in TERMS order), and per case <name>:
                 <name>/<map> f32 inputs: opacity, depth, roughness, metallic, gt_depth, image_mask [1,H,W];
                   normal, pseudo_normal, base_color, gt_image, mvs_normal [3,H,W]
                 <name>/f64/<term>   the eight values on .double() tensors, the clamp bounds being the f32
                   constants float(np.float32(1e-6)) and float(np.float32(1 - 1e-6)) that torch uses on f32
                 <name>/f64/d_<map>  the six gradient maps d(sum of lambda * term) / d map, f64
                 <name>/ref32/<term>, <name>/ref32/d_<map>  the distance of the reference's f32 evaluation from
                   the f64 one in the measure of tests/test_reg_loss.py (values absolute, a NaN pair 0;
                   gradients over max(max |f64 gradient|, 1 / elements), the smoothness gradients without the
                   pixels whose sign is ambiguous)

Usage:  python tests/golden/make_golden_reg_loss.py --reference <checkout of the reference project>
"""
from __future__ import annotations

import argparse
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
TERMS = ("loss_depth", "loss_mask_entropy", "loss_normal_render_depth", "loss_normal_mvs_depth", "loss_base_color",
         "loss_base_color_smooth", "loss_metallic_smooth", "loss_roughness_smooth")
LAMBDAS = (1.0, 0.5, 2.0, 1.5, 1.0, 0.75, 1.25, 0.5)
PLANES = {"opacity": 1, "depth": 1, "normal": 3, "pseudo_normal": 3, "base_color": 3, "roughness": 1, "metallic": 1,
          "gt_image": 3, "gt_depth": 1, "image_mask": 1, "mvs_normal": 3}
REACHES = {"opacity": (1,), "depth": (0,), "normal": (2, 3), "base_color": (4, 5), "roughness": (7,), "metallic": (6,)}
SMOOTH = ("base_color", "roughness", "metallic")
AMBIGUOUS = 1e-5
CLAMP32 = (float(np.float32(1e-6)), float(np.float32(1 - 1e-6)))


def load(reference: str, rel: str):
    spec = importlib.util.spec_from_file_location("ref_" + os.path.basename(rel)[:-3], os.path.join(reference, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def unit(rng, h, w):
    n = rng.standard_normal((3, h, w)).astype(np.float32)
    return (n / np.sqrt((n.astype(np.float64) ** 2).sum(0, keepdims=True))).astype(np.float32)


def random_case(rng, h, w):
    c = {k: rng.random((n, h, w), dtype=np.float32) for k, n in PLANES.items()}
    for k in ("normal", "pseudo_normal", "mvs_normal"):
        c[k] = unit(rng, h, w)
    mask = (rng.random((1, h, w)) > 0.3).astype(np.float32)
    valid = rng.random((1, h, w)) > 0.4       # gt_depth > 0 here: partly disagrees with the mask
    mask.flat[0], valid.flat[0] = 1.0, True   # at least one selected pixel
    if h * w > 1:                             # both mask values present (a 1x1 mask has one)
        mask.flat[-1] = 0.0
    c["image_mask"] = mask
    c["gt_depth"] = np.where(valid, c["gt_depth"] + np.float32(0.5), np.float32(0)).astype(np.float32)
    c["depth"] = (c["depth"] + np.float32(0.5)).astype(np.float32)
    return c


def cases():
    rng = np.random.default_rng(2025)
    out = {}
    for h, w in [(1, 1), (5, 7), (16, 16), (17, 15), (16, 33), (37, 53)]:
        out[f"r_{h}x{w}"] = random_case(rng, h, w)
    # the left half flat: constant data maps, depth == gt_depth, base_color == its target (gt 0.5, mask 1:
    # w = 0.5 and t = 0.5 exactly), and opacity exactly 0 and exactly 1 on two stripes
    c = random_case(rng, 20, 20)
    c["base_color"][:, :, :10], c["roughness"][:, :, :10], c["metallic"][:, :, :10] = 0.5, 0.25, 0.75
    c["gt_image"][:, :, :10], c["image_mask"][:, :, :10] = 0.5, 1.0
    c["gt_depth"][:, :, :10] = c["depth"][:, :, :10]
    c["opacity"][:, 3, :], c["opacity"][:, 5, :] = 0.0, 1.0
    out["flat_half"] = c
    # gt_depth > 0 exactly where the mask is 0: the depth term selects no pixel
    c = random_case(rng, 5, 7)
    c["gt_depth"] = np.where(c["image_mask"] == 0, np.float32(1.25), np.float32(0)).astype(np.float32)
    out["no_depth_pixels"] = c
    return out


class _DoubleKernels:
    """Stands in for the `torch` name inside the reference's loss_utils while it runs on .double() tensors:
    cal_gradient builds its two Sobel kernels with torch.FloatTensor, which F.conv2d refuses to mix with f64
    data. The kernels' entries (0, 1, 2) are exact in either type; everything else is torch itself."""
    FloatTensor = torch.DoubleTensor

    def __getattr__(self, name):
        return getattr(torch, name)


def smooth(lu, data, image, mask):
    """The reference's own bilateral_smooth_loss, in the dtype of its arguments."""
    if data.dtype == torch.float32:
        return lu.bilateral_smooth_loss(data, image, mask)
    lu.torch = _DoubleKernels()
    try:
        return lu.bilateral_smooth_loss(data, image, mask)
    finally:
        lu.torch = torch


def evaluate(lu, t, clamp):
    """The eight terms on the tensors of t. The three smoothness terms are the reference's own function; the
    other five are this project's restatement of the formulas of neilf.py:233-321, one tensor operation per
    operation of the reference so that the f32 evaluation rounds where the reference's does."""
    m, gd, gt = t["image_mask"], t["gt_depth"], t["gt_image"]
    v = {}
    agree = m.bool() == (gd > 0)  # the complement of the reference's xor of the two masks
    v["loss_depth"] = F.l1_loss(t["depth"][agree], gd[agree])
    o = t["opacity"].clamp(*clamp)
    v["loss_mask_entropy"] = -(m * torch.log(o) + (1 - m) * torch.log(1 - o)).mean()
    v["loss_normal_render_depth"] = F.mse_loss(t["normal"] * m, t["pseudo_normal"].detach() * m)
    dm = (gd > 0).to(m.dtype)
    v["loss_normal_mvs_depth"] = F.mse_loss(t["normal"] * dm, t["mvs_normal"] * dm)
    gm = gt * m
    w = 1 / (1 + torch.exp(-5 * (gm.max(0, keepdim=True)[0] - 0.5)))  # weight of the squared (specular) branch
    target = w * (gm * gm) + (1 - w) * (1 - (1 - gm) * (1 - gm))
    v["loss_base_color"] = F.l1_loss(target, t["base_color"])
    v["loss_base_color_smooth"] = smooth(lu, t["base_color"], gt, m)
    v["loss_metallic_smooth"] = smooth(lu, t["metallic"], gt, m)
    v["loss_roughness_smooth"] = smooth(lu, t["roughness"], gt, m)
    return v


def run(lu, case, dt):
    """-> ({term: value}, {map: gradient of sum lambda * term}) as numpy, evaluated in dtype dt."""
    t = {k: torch.from_numpy(a).to(dt) for k, a in case.items()}
    for k in REACHES:
        t[k].requires_grad_(True)
    clamp = (1e-6, 1 - 1e-6) if dt == torch.float32 else CLAMP32  # torch rounds the doubles to the tensor's f32
    v = evaluate(lu, t, clamp)
    grads = {}
    for k, reach in REACHES.items():
        total = sum(LAMBDAS[i] * v[TERMS[i]] for i in reach)
        grads[k] = torch.autograd.grad(total, t[k], retain_graph=True)[0].numpy()
    return {k: x.detach().numpy() for k, x in v.items()}, grads


def ambiguous(case, name):
    """[H,W] bool: within the 3x3 reach of a Sobel response of the map's channel mean with 0 < |f64 response|
    < AMBIGUOUS, whose sign an f32 evaluation may take either way."""
    mean = torch.from_numpy(case[name]).double().mean(0)[None, None]
    kx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], dtype=torch.float64)[None, None]
    r = torch.cat([F.conv2d(mean, kx, padding=1), F.conv2d(mean, kx.transpose(2, 3), padding=1)], 1).abs()
    bad = ((r > 0) & (r < AMBIGUOUS)).any(1, keepdim=True).double()
    return F.max_pool2d(bad, 3, stride=1, padding=1)[0, 0].bool().numpy()


def value_distance(got, ref):
    if np.isnan(ref):
        assert np.isnan(got)
        return 0.0
    return float(abs(float(got) - float(ref)))


def grad_distance(got, ref, skip=None):
    err = np.abs(got.astype(np.float64) - ref)
    if skip is not None:
        err = np.where(skip[None], 0.0, err)
    return float(err.max() / max(np.abs(ref).max(), 1.0 / ref.size))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    a = ap.parse_args()
    lu = load(a.reference, "utils/loss_utils.py")
    out, names = {"lambdas": np.array(LAMBDAS, np.float64)}, []
    for name, case in cases().items():
        names.append(name)
        for k, arr in case.items():
            assert arr.dtype == np.float32 and arr.shape[0] == PLANES[k], (name, k)
            out[f"{name}/{k}"] = arr
        v64, g64 = run(lu, case, torch.float64)
        v32, g32 = run(lu, case, torch.float32)
        for k in TERMS:
            assert v64[k].dtype == np.float64 and v32[k].dtype == np.float32
            out[f"{name}/f64/{k}"] = v64[k]
            out[f"{name}/ref32/{k}"] = np.float64(value_distance(v32[k], v64[k]))
        for k in REACHES:
            assert g64[k].dtype == np.float64 and np.isfinite(g64[k]).all(), (name, k)
            out[f"{name}/f64/d_{k}"] = g64[k]
            out[f"{name}/ref32/d_{k}"] = np.float64(grad_distance(g32[k], g64[k], ambiguous(case, k) if k in SMOOTH else None))
        if name == "no_depth_pixels":
            assert np.isnan(v64["loss_depth"]) and not g64["depth"].any()
        print(name, {k: float(out[f"{name}/ref32/{k}"]) for k in TERMS})
        print(" " * len(name), {k: float(out[f"{name}/ref32/d_{k}"]) for k in REACHES})
    out["names"] = np.array(names)
    path = os.path.join(HERE, "reg_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote reg_loss.npz", len(names), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
