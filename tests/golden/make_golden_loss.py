"""Golden vectors for the image loss from the REFERENCE's own utils/loss_utils.py and utils/image_utils.py
(CPU container; both run on CPU tensors).

The two modules are loaded by path. image_utils imports matplotlib at module level for a depth
visualiser that is not used here; when the package is absent an empty stand-in module satisfies the import.

  loss.npz   window [1,1,11,11] (create_window(11, 1)), gauss [11] (gaussian(11, 1.5)), names [n], and per
             case <name>: <name>/img, <name>/gt (f32; [C,H,W], or [B,C,H,W] for the batched case), then twice,
             <name>/f32/... as the reference runs it (ssim(), F.l1_loss, psnr on f32 tensors) and <name>/f64/...
             from the reference's own _ssim / create_window, F.l1_loss and psnr on .double() tensors:
               ssim, l1, psnr, loss  scalars, loss = (1 - 0.2) * l1 + 0.2 * (1 - ssim) (neilf.py:216-222)
               dssim, dloss          d ssim / d img and d loss / d img
             and for the batched case instead: ssim (size_average=True), dssim, ssim_b [B]
             (size_average=False) and dssim_b = d (sum_b (b + 1) ssim_b[b]) / d img.

Usage:  python tests/golden/make_golden_loss.py  [--reference /root/reference]
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
LAMBDA = 0.2  # arguments/__init__.py:115 lambda_dssim


def load(reference: str, rel: str):
    spec = importlib.util.spec_from_file_location("ref_" + os.path.basename(rel)[:-3], os.path.join(reference, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def noisy(rng, shape):
    img = rng.random(shape, dtype=np.float32)
    gt = np.clip(img + np.float32(0.1) * rng.standard_normal(shape, dtype=np.float32), 0, 1).astype(np.float32)
    return img, gt


def cases():
    rng = np.random.default_rng(2024)
    out = {}
    for c, h, w in [(3, 1, 1), (3, 5, 7), (1, 11, 11), (3, 16, 16), (3, 17, 15), (4, 16, 33), (3, 37, 53), (3, 64, 48)]:
        out[f"c{c}_{h}x{w}"] = noisy(rng, (c, h, w))
    img, gt = noisy(rng, (3, 20, 20))
    gt[:, :, :10] = img[:, :, :10]  # sign(0) on the left half, SSIM -> 1 there
    out["half_equal"] = (img, gt)
    out["constant"] = (np.full((3, 20, 20), 0.5, np.float32), np.full((3, 20, 20), 0.5, np.float32))
    out["batch"] = noisy(rng, (2, 3, 12, 18))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        sys.modules["matplotlib"] = types.ModuleType("matplotlib")
    lu = load(a.reference, "utils/loss_utils.py")
    iu = load(a.reference, "utils/image_utils.py")

    def ssim_of(x, y, size_average=True):
        if x.dtype == torch.float32:
            return lu.ssim(x, y, size_average=size_average)
        channel = x.size(-3)  # ssim() itself would cast the window to f32 first: go through its two parts
        return lu._ssim(x, y, lu.create_window(11, channel).double(), 11, channel, size_average)

    def grad(fn, x):
        x = x.clone().requires_grad_(True)
        fn(x).backward()
        return x.grad.numpy()

    out = {"window": lu.create_window(11, 1).numpy(), "gauss": lu.gaussian(11, 1.5).numpy()}
    assert out["window"].dtype == np.float32 and out["gauss"].dtype == np.float32
    names = []
    for name, (img, gt) in cases().items():
        names.append(name)
        out[f"{name}/img"], out[f"{name}/gt"] = img, gt
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            x, y = torch.from_numpy(img).to(dt), torch.from_numpy(gt).to(dt)
            k = f"{name}/{tag}/"
            out[k + "ssim"] = ssim_of(x, y).numpy()
            out[k + "dssim"] = grad(lambda t: ssim_of(t, y), x)
            if name == "batch":
                wts = torch.arange(1, x.shape[0] + 1, dtype=dt)
                out[k + "ssim_b"] = ssim_of(x, y, False).numpy()
                out[k + "dssim_b"] = grad(lambda t: (ssim_of(t, y, False) * wts).sum(), x)
                continue

            def loss(t):
                return (1.0 - LAMBDA) * F.l1_loss(t, y) + LAMBDA * (1.0 - ssim_of(t, y))

            out[k + "l1"] = F.l1_loss(x, y).numpy()
            out[k + "psnr"] = iu.psnr(x, y).mean().numpy()
            out[k + "loss"] = loss(x).detach().numpy()
            out[k + "dloss"] = grad(loss, x)
            assert out[k + "dloss"].dtype == (np.float32 if tag == "f32" else np.float64)
    out["names"] = np.array(names)
    path = os.path.join(HERE, "loss.npz")
    np.savez_compressed(path, **out)
    print("wrote loss.npz", len(names), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
