"""Timing of the fused depth / mask / normal / base-colour / smoothness terms on one MI355X (csrc/reg_loss.hip
through relightable3dgaussian_amd.loss.regularizer_losses).

Workloads: all eight terms at 800x800 (the Blender scenes) and 1920x1080 (the headline size), the rendered maps
as the rasterizer's [H,W,n] blocks (image_layout="hwc"), uniform random maps, unit normals, a binary mask and a
gt_depth that is positive on a region partly disagreeing with it; the lambdas are those of the reference's
recipes (script/run_dtu.sh and the NeILF stage). Timed with HIP events around single calls after a warm-up
(median, min and max over --iters):
  fused forward              regularizer_losses under no_grad (the two forward launches + the scalar glue)
  fused forward + backward   regularizer_losses(...)[0].backward() into the six maps' .grad

Beside it, on the same GPU, what a user has without the operator: the formulas of calculate_loss
(gaussian_renderer/neilf.py:233-321) as f32 torch code with the reference's sequence of operations (the
restatement of tests/test_reg_loss.py in f32), on [n,H,W] views of the same blocks, including the three Sobel
passes over gt_image, the boolean indexing of the depth term and one .item() per term. Its loss is compared
with the fused one.

Also timed: single calls of _C.reg_loss_forward / _C.reg_loss_backward (calls_forward, calls_backward). These
hold the launches and their allocator calls, not the kernels alone, so the fraction of the HBM bound derived
from them is a lower bound. The HBM bound is the algorithmic byte count of DESIGN.md section 2h (forward 84 B
read per pixel, backward 84 B read + 40 B written) over --hbm-tbps (default 6.29, the measured copy rate).

Usage: python tools/reg_loss_bench.py [--sizes 800x800 1920x1080] [--iters 50] [--warmup 10] [--out file.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAMBDAS = {"lambda_depth": 1.0, "lambda_mask_entropy": 0.1, "lambda_normal_render_depth": 0.01,
           "lambda_normal_mvs_depth": 0.01, "lambda_base_color": 0.005, "lambda_base_color_smooth": 0.006,
           "lambda_metallic_smooth": 0.002, "lambda_roughness_smooth": 0.002}
RENDERED = {"opacity": 1, "depth": 1, "normal": 3, "pseudo_normal": 3, "base_color": 3, "roughness": 1, "metallic": 1}
TARGETS = {"gt_image": 3, "gt_depth": 1, "image_mask": 1, "mvs_normal": 3}
DIFFERENTIABLE = ("opacity", "depth", "normal", "base_color", "roughness", "metallic")


def make_maps(H, W, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rand = lambda *s: torch.rand(s, device="cuda", generator=g)
    maps = {k: rand(H, W, n) for k, n in RENDERED.items()}
    targets = {k: rand(n, H, W) for k, n in TARGETS.items()}
    for d, k, axis in ((maps, "normal", 2), (maps, "pseudo_normal", 2), (targets, "mvs_normal", 0)):
        d[k] = F.normalize(torch.randn(d[k].shape, device="cuda", generator=g), dim=axis)
    targets["image_mask"] = (targets["image_mask"] > 0.3).float()
    targets["gt_depth"] = torch.where(rand(1, H, W) > 0.4, targets["gt_depth"] + 0.5, torch.zeros(()).cuda())
    maps["depth"] = maps["depth"] + 0.5
    return maps, targets


def sobel_abs(mean, kernels):
    """|Sobel_x| + |Sobel_y| of a [1,H,W] map with zero "same" padding, one conv2d per filter as the reference."""
    x = mean[None]
    return (F.conv2d(x, kernels[0], padding="same").abs() + F.conv2d(x, kernels[1], padding="same").abs())[0]


def smoothness(data, image, mask, kernels):
    """The bilateral smoothness term; the guide is recomputed from `image` on every call, as the reference does."""
    guide = torch.exp(-sobel_abs(image.mean(0, keepdim=True), kernels))
    return (sobel_abs(data.mean(0, keepdim=True), kernels) * guide * mask).mean()


def torch_loss(r, t, lam, kernels):
    """The eight terms as f32 torch code with the reference's sequence of operations (the restatement of
    tests/test_reg_loss.py in f32): boolean indexing for the depth term, a Sobel pass over gt_image in each of
    the three smoothness terms, one .item() per term. r holds [n,H,W] views of the rendered blocks."""
    m, gd, gt = t["image_mask"], t["gt_depth"], t["gt_image"]
    stats, total = {}, [0.0]

    def add(key, term):  # the reference logs each term with .item() where it computes it
        stats["loss_" + key] = term.item()
        total[0] = total[0] + lam["lambda_" + key] * term

    agree = m.bool() == (gd > 0)
    add("depth", F.l1_loss(r["depth"][agree], gd[agree]))
    o = r["opacity"].clamp(1e-6, 1 - 1e-6)
    add("mask_entropy", -(m * torch.log(o) + (1 - m) * torch.log(1 - o)).mean())
    add("normal_render_depth", F.mse_loss(r["normal"] * m, r["pseudo_normal"].detach() * m))
    dm = (gd > 0).float()
    add("normal_mvs_depth", F.mse_loss(r["normal"] * dm, t["mvs_normal"] * dm))
    gm = gt * m
    w = 1 / (1 + torch.exp(-5 * (gm.max(0, keepdim=True)[0] - 0.5)))
    add("base_color", F.l1_loss(w * (gm * gm) + (1 - w) * (1 - (1 - gm) * (1 - gm)), r["base_color"]))
    for key in ("base_color", "metallic", "roughness"):
        add(key + "_smooth", smoothness(r[key], gt, m, kernels))
    return total[0]


def time_calls(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["800x800", "1920x1080"], help="WxH")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reg_loss_bench: needs a GPU (nothing is timed on the host)")
    from relightable3dgaussian_amd import _C, loss

    results = []
    for size in a.sizes:
        W, H = (int(v) for v in size.split("x"))
        maps, targets = make_maps(H, W)
        for k in DIFFERENTIABLE:
            maps[k].requires_grad_(True)
        views = {k: v.permute(2, 0, 1) for k, v in maps.items()}  # [n,H,W] views for the torch formulas
        leaves = [maps[k] for k in DIFFERENTIABLE]
        sobel_x = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], device="cuda")[None, None]
        kernels = (sobel_x, sobel_x.transpose(2, 3).contiguous())  # prebuilt: their upload is not charged

        def clear():
            for x in leaves:
                x.grad = None

        def fused_fwd():
            with torch.no_grad():
                return loss.regularizer_losses(maps, targets, LAMBDAS, image_layout="hwc")

        def fused_fwd_bwd():
            clear()
            loss.regularizer_losses(maps, targets, LAMBDAS, image_layout="hwc")[0].backward()

        def torch_fwd():
            with torch.no_grad():
                return torch_loss(views, targets, LAMBDAS, kernels)

        def torch_fwd_bwd():
            clear()
            torch_loss(views, targets, LAMBDAS, kernels).backward()

        # single binding calls (the launches and their allocator calls), without the autograd and scalar glue of
        # loss.py: an upper bound on the kernels' time, so a lower bound on their fraction of the HBM bound
        order = [maps[k].detach() for k in RENDERED] + [targets[k] for k in TARGETS]
        weights = torch.tensor([LAMBDAS[k] for k in LAMBDAS], device="cuda")
        _, count = _C.reg_loss_forward(order, H, W, 255, True)
        n = H * W
        res = {"W": W, "H": H,
               "fused_forward": time_calls(fused_fwd, a.warmup, a.iters),
               "fused_forward_backward": time_calls(fused_fwd_bwd, a.warmup, a.iters),
               "calls_forward": time_calls(lambda: _C.reg_loss_forward(order, H, W, 255, True), a.warmup, a.iters),
               "calls_backward": time_calls(lambda: _C.reg_loss_backward(order, H, W, 255, True, count, weights),
                                              a.warmup, a.iters),
               "torch_forward": time_calls(torch_fwd, a.warmup, a.iters),
               "torch_forward_backward": time_calls(torch_fwd_bwd, a.warmup, a.iters)}
        fused_fwd_bwd()
        g_fused = [x.grad.clone() for x in leaves]
        torch_fwd_bwd()
        res["max_abs_grad_diff_x_numel"] = {k: float((g - x.grad).abs().max()) * n
                                            for k, g, x in zip(DIFFERENTIABLE, g_fused, leaves)}
        res["abs_loss_diff"] = abs(float(fused_fwd()[0]) - float(torch_fwd()))
        res["speedup_forward"] = res["torch_forward"]["median_ms"] / res["fused_forward"]["median_ms"]
        res["speedup_forward_backward"] = (res["torch_forward_backward"]["median_ms"] /
                                           res["fused_forward_backward"]["median_ms"])
        bound = {"forward": 84 * n, "backward": (84 + 40) * n}
        res["hbm_bound_ms"] = {k: v / (a.hbm_tbps * 1e12) * 1e3 for k, v in bound.items()}
        res["fraction_of_hbm_bound"] = {
            "forward": res["hbm_bound_ms"]["forward"] / res["calls_forward"]["median_ms"],
            "backward": res["hbm_bound_ms"]["backward"] / res["calls_backward"]["median_ms"]}
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "hbm_tbps": a.hbm_tbps, "lambdas": LAMBDAS,
                       "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
