"""The training image loss: drop-in for the reference's `utils.loss_utils.ssim` and the fused form of
`calculate_loss`'s L1 + SSIM term (gaussian_renderer/neilf.py:216-222).

`ssim(img1, img2, window_size=11, size_average=True)` -- the reference's signature (loss_utils.py:31-62):
[C,H,W] or [B,C,H,W] f32 GPU tensors, differentiable in `img1`.

`l1_ssim_loss(image, gt, lambda_dssim, image_layout="chw")` -> (loss, stats):
loss = (1 - lambda) * L1 + lambda * (1 - SSIM), stats = {"l1", "ssim", "psnr"} as detached 0-dim device
tensors (psnr as utils/image_utils.py:24-29 and neilf.py:220: per-channel MSE -> 20 log10(1 / sqrt(mse))
-> mean). With image_layout="hwc", `image` is the rasterizer's [H,W,C] output as it is, `gt` stays
[C,H,W], and the gradient comes back [H,W,C].

Both are one forward launch pair and one backward launch of csrc/loss.hip (semantics in
include/r3dg_hip.h `r3dg_image_loss_forward`); a few [planes]-sized torch operations turn the per-plane
sums into the scalars. Nothing synchronises with the host. No CPU path and no torch fallback: the
extension rejects CPU tensors. There is no gradient with respect to `img2` / `gt`.
"""
from __future__ import annotations

import torch

from . import _C


def _planes(t: torch.Tensor, n: int, value: float) -> torch.Tensor:
    return torch.full((n,), value, dtype=torch.float32, device=t.device)


class _SSIM(torch.autograd.Function):
    """img1, img2 [B,C,H,W] -> the mean of ssim_map, over everything or per image."""

    @staticmethod
    def forward(ctx, img1, img2, per_image, need_grad):
        B, C, H, W = img1.shape
        sums, dmaps = _C.image_loss_forward(img1, img2, False, need_grad)
        ctx.save_for_backward(img1, img2, dmaps)
        ctx.per_image = per_image
        if per_image:
            return sums.reshape(B, C, 3).sum(1)[:, 0] / float(C * H * W)
        return (sums.sum(0) / float(B * C * H * W))[0]  # the expression of _L1SSIM: the same bits

    @staticmethod
    def backward(ctx, grad):
        img1, img2, dmaps = ctx.saved_tensors
        if dmaps.numel() == 0 and img1.numel() != 0:
            raise RuntimeError("ssim: backward of a forward that ran without a gradient request")
        B, C, H, W = img1.shape
        n = C * H * W if ctx.per_image else B * C * H * W
        scale = grad.to(torch.float32).reshape(-1, 1).expand(B, C).reshape(B * C)
        out = _C.image_loss_backward(img1, img2, False, dmaps, _planes(img1, B * C, 1.0 / n),
                                     _planes(img1, B * C, 0.0), scale)
        return out, None, None, None


class _L1SSIM(torch.autograd.Function):
    """-> loss, l1, ssim, psnr (the last three not differentiable)."""

    @staticmethod
    def forward(ctx, image, gt, lam, hwc, need_grad):
        C, H, W = gt.shape
        sums, dmaps = _C.image_loss_forward(image, gt, hwc, need_grad)
        ctx.save_for_backward(image, gt, dmaps)
        ctx.lam, ctx.hwc = lam, hwc
        tot = sums.sum(0) / float(C * H * W)
        ssim_val, l1 = tot[0], tot[1]
        loss = (1.0 - lam) * l1 + lam * (1.0 - ssim_val)
        psnr = (20.0 * torch.log10(1.0 / torch.sqrt(sums[:, 2] / float(H * W)))).mean()
        ctx.mark_non_differentiable(l1, ssim_val, psnr)
        return loss, l1, ssim_val, psnr

    @staticmethod
    def backward(ctx, grad, *_):
        image, gt, dmaps = ctx.saved_tensors
        if dmaps.numel() == 0 and image.numel() != 0:
            raise RuntimeError("l1_ssim_loss: backward of a forward that ran without a gradient request")
        C, H, W = gt.shape
        n = float(C * H * W)
        out = _C.image_loss_backward(image, gt, ctx.hwc, dmaps, _planes(gt, C, -ctx.lam / n),
                                     _planes(gt, C, (1.0 - ctx.lam) / n),
                                     grad.to(torch.float32).reshape(1).expand(C).contiguous())
        return out, None, None, None, None


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """utils/loss_utils.py:31 `ssim`: the mean of the SSIM map (per image, [B], with size_average=False on
    4-D input)."""
    if window_size != 11:
        raise ValueError(f"ssim: this build has the reference's window_size=11 only, got {window_size}")
    if img2.requires_grad:
        raise ValueError("ssim: no gradient with respect to img2 (detach it)")
    if img1.dim() not in (3, 4) or img1.shape != img2.shape:
        raise ValueError(f"ssim: [C,H,W] or [B,C,H,W] images of one shape expected, got {tuple(img1.shape)} "
                         f"and {tuple(img2.shape)}")
    if img1.dim() == 3 and not size_average:
        raise ValueError("ssim: size_average=False needs [B,C,H,W] input")
    a, b = (img1[None], img2[None]) if img1.dim() == 3 else (img1, img2)
    return _SSIM.apply(a, b, not size_average, torch.is_grad_enabled() and img1.requires_grad)


def l1_ssim_loss(image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float, image_layout: str = "chw"):
    """(1 - lambda) * L1 + lambda * (1 - SSIM) of `image` against `gt` [C,H,W], and the iteration's
    statistics, from one pass over the two images (neilf.py:216-222)."""
    if image_layout not in ("chw", "hwc"):
        raise ValueError(f"l1_ssim_loss: image_layout 'chw' or 'hwc' expected, got {image_layout!r}")
    if gt.requires_grad:
        raise ValueError("l1_ssim_loss: no gradient with respect to gt (detach it)")
    hwc = image_layout == "hwc"
    want = tuple(gt.permute(1, 2, 0).shape) if gt.dim() == 3 and hwc else tuple(gt.shape)
    if gt.dim() != 3 or tuple(image.shape) != want:
        raise ValueError(f"l1_ssim_loss: gt [C,H,W] and image in layout {image_layout!r} expected, got "
                         f"{tuple(gt.shape)} and {tuple(image.shape)}")
    loss, l1, ssim_val, psnr = _L1SSIM.apply(image, gt, float(lambda_dssim), hwc,
                                             torch.is_grad_enabled() and image.requires_grad)
    return loss, {"l1": l1, "ssim": ssim_val, "psnr": psnr}


__all__ = ["ssim", "l1_ssim_loss"]
