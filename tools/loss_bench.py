"""Image loss timing on one MI355X (csrc/loss.hip through relightable3dgaussian_amd.loss.l1_ssim_loss).

Workloads: one C = 3 image against its ground truth at 800x800 (the Blender scenes) and 1920x1080 (the
headline size), image = U(0,1), gt = clamp(image + 0.1 N(0,1), 0, 1), lambda = 0.2. Timed with HIP events
around single calls after a warm-up (median, min and max over --iters):
  fused forward              l1_ssim_loss under no_grad (the two forward launches + the scalar glue)
  fused forward + backward   l1_ssim_loss(...)[0].backward() into image.grad

Beside it, on the same GPU, what a user has without the operator: the reference's formula in torch
(utils/loss_utils.py:31-62 ssim with five depthwise 11x11 F.conv2d, F.l1_loss, psnr; the restatement of
tests/test_image_loss.py in f32), forward and forward + backward. Its loss is compared with the fused one.

The HBM bound of the fused pair is the algorithmic byte count of DESIGN.md section 4 (forward 8 B read +
12 B written per image element, backward 20 B + 4 B) over --hbm-tbps (default 6.29, the measured copy
rate); "forward" alone without the derivative planes reads 8 B per element.

Usage: python tools/loss_bench.py [--sizes 800x800 1920x1080] [--iters 50] [--warmup 10] [--out file.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAMBDA = 0.2


def make_images(C, H, W, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    img = torch.rand((C, H, W), device="cuda", generator=g)
    gt = (img + 0.1 * torch.randn((C, H, W), device="cuda", generator=g)).clamp(0, 1)
    return img, gt


def torch_window(channel, device):
    g = torch.Tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float()[None, None].expand(channel, 1, 11, 11).contiguous().to(device)


def torch_loss(img, gt, window):
    """calculate_loss's L1 + SSIM term and psnr as the reference computes them (window prebuilt: the
    reference rebuilds and uploads it on every call, which is not charged here)."""
    c = img.size(-3)
    mu1, mu2 = F.conv2d(img, window, padding=5, groups=c), F.conv2d(gt, window, padding=5, groups=c)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(img * img, window, padding=5, groups=c) - mu1_sq
    s2 = F.conv2d(gt * gt, window, padding=5, groups=c) - mu2_sq
    s12 = F.conv2d(img * gt, window, padding=5, groups=c) - mu1_mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim = (((2 * mu1_mu2 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))).mean()
    l1 = F.l1_loss(img, gt)
    mse = ((img - gt) ** 2).view(c, -1).mean(1, keepdim=True)
    psnr = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()
    return (1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - ssim), psnr


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
        sys.exit("loss_bench: needs a GPU (nothing is timed on the host)")
    from relightable3dgaussian_amd import _C, loss

    results = []
    for size in a.sizes:
        W, H = (int(v) for v in size.split("x"))
        C = 3
        img, gt = make_images(C, H, W)
        x = img.clone().requires_grad_(True)
        window = torch_window(C, img.device)

        def fused_fwd():
            with torch.no_grad():
                return loss.l1_ssim_loss(x, gt, LAMBDA)

        def fused_fwd_bwd():
            x.grad = None
            loss.l1_ssim_loss(x, gt, LAMBDA)[0].backward()

        def torch_fwd():
            with torch.no_grad():
                return torch_loss(x, gt, window)

        def torch_fwd_bwd():
            x.grad = None
            torch_loss(x, gt, window)[0].backward()

        # the kernels alone, without the autograd and scalar glue of loss.py
        sums_dmaps = _C.image_loss_forward(img, gt, False, True)
        ws, wa = (torch.full((C,), v, device="cuda") for v in (-LAMBDA / img.numel(), (1 - LAMBDA) / img.numel()))
        n = img.numel()
        res = {"W": W, "H": H, "C": C,
               "fused_forward": time_calls(fused_fwd, a.warmup, a.iters),
               "fused_forward_backward": time_calls(fused_fwd_bwd, a.warmup, a.iters),
               "kernels_forward_nograd": time_calls(lambda: _C.image_loss_forward(img, gt, False, False), a.warmup, a.iters),
               "kernels_forward": time_calls(lambda: _C.image_loss_forward(img, gt, False, True), a.warmup, a.iters),
               "kernels_backward": time_calls(lambda: _C.image_loss_backward(img, gt, False, sums_dmaps[1], ws, wa),
                                              a.warmup, a.iters),
               "torch_forward": time_calls(torch_fwd, a.warmup, a.iters),
               "torch_forward_backward": time_calls(torch_fwd_bwd, a.warmup, a.iters)}
        fused_fwd_bwd()
        g_fused = x.grad.clone()
        torch_fwd_bwd()
        res["max_abs_grad_diff_x_numel"] = float((g_fused - x.grad).abs().max()) * n
        res["abs_loss_diff"] = abs(float(fused_fwd()[0]) - float(torch_fwd()[0]))
        res["speedup_forward"] = res["torch_forward"]["median_ms"] / res["fused_forward"]["median_ms"]
        res["speedup_forward_backward"] = (res["torch_forward_backward"]["median_ms"] /
                                           res["fused_forward_backward"]["median_ms"])
        bound = {"forward_nograd": 8 * n, "forward": 20 * n, "backward": 24 * n}
        res["hbm_bound_ms"] = {k: v / (a.hbm_tbps * 1e12) * 1e3 for k, v in bound.items()}
        res["fraction_of_hbm_bound"] = {
            "forward_nograd": res["hbm_bound_ms"]["forward_nograd"] / res["kernels_forward_nograd"]["median_ms"],
            "forward": res["hbm_bound_ms"]["forward"] / res["kernels_forward"]["median_ms"],
            "backward": res["hbm_bound_ms"]["backward"] / res["kernels_backward"]["median_ms"]}
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "hbm_tbps": a.hbm_tbps, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
