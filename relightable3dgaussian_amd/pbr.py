"""The PBR image head and the light regulariser of a training iteration (csrc/pbr_head.hip; semantics in
include/r3dg_hip.h `r3dg_pbr_head_forward` and `r3dg_light_loss_forward`).

`pbr_image(pbr, opacity, bg, gamma=None, tone="none", image_layout="hwc")` -> image: the composite over the
background and the tone step between the rasterizer's output and the image loss
(gaussian_renderer/neilf.py:169-175), in one launch forward and one backward (two with gamma):
  x = pbr + (1 - opacity) * bg
  tone "none"   y = x                            gradients to pbr and opacity
       "gamma"  y = clamp(x, 1e-9, 1) ** gamma   scene/gamma_trans.py:45-51 hdr2ldr; gradients to pbr, opacity
                                                 and gamma (a [1] device tensor, never read on the host)
       "aces"   utils/graphics_utils.py:197-201 hdr2ldr (the evaluation grid)               forward only
       "clamp"  y = clamp(x, 0, 1)                                                          forward only
`pbr` [H,W,3] and `opacity` [H,W,1] are the rasterizer's blocks as they are (image_layout="hwc"), or [3,H,W]
and [1,H,W] ("chw"). `bg` is [3], or an image shaped like `pbr` (the environment behind the object); it gets
no gradient. The image has `pbr`'s shape and layout and is always a fresh tensor; with "hwc" it goes straight
into `loss.l1_ssim_loss(..., image_layout="hwc")`. dL/dgamma is a deterministic reduction: two runs give the
same bits.

`light_loss(diffuse_light)` -> the lambda_light term (neilf.py:278-283): the mean over the 3 P elements of
|d_c - mean_c d| of `diffuse_light` [P,3], two launches forward and one backward. Its gradient is a contiguous
[P,3], the `dL_ddiffuse_light` that `render_equation_backward` takes. P = 0 gives 0 without a launch.

Nothing synchronises with the host. No CPU path and no torch fallback: the extension rejects CPU tensors.
There is no double backward.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _C

_TONES = dict(_C.pbr.TONES)
_FORWARD_ONLY = ("aces", "clamp")


class _PbrImage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pbr, opacity, gamma, bg, tone, hwc):
        ctx.save_for_backward(pbr, opacity, bg, gamma)
        ctx.tone, ctx.hwc = tone, hwc
        return _C.pbr.head_forward(pbr, opacity, bg, gamma, tone, hwc)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        pbr, opacity, bg, gamma = ctx.saved_tensors
        want = sum(1 << i for i in range(3) if ctx.needs_input_grad[i])
        d_pbr, d_opacity, d_gamma = _C.pbr.head_backward(pbr, opacity, bg, gamma, ctx.tone, ctx.hwc, grad, want)
        if d_gamma is not None:
            d_gamma = d_gamma.reshape(gamma.shape)
        return d_pbr, d_opacity, d_gamma, None, None, None


def pbr_image(pbr: torch.Tensor, opacity: torch.Tensor, bg: torch.Tensor, gamma: torch.Tensor | None = None,
              tone: str = "none", image_layout: str = "hwc") -> torch.Tensor:
    """tone(pbr + (1 - opacity) * bg): neilf.py:169-175 with the learnable gamma, the captures' composite, or
    the evaluation grid's clamp / ACES."""
    who = "pbr_image"
    if image_layout not in ("chw", "hwc"):
        raise ValueError(f"{who}: image_layout 'chw' or 'hwc' expected, got {image_layout!r}")
    if tone not in _TONES:
        raise ValueError(f"{who}: tone one of {sorted(_TONES)} expected, got {tone!r}")
    hwc = image_layout == "hwc"
    for name, t in (("pbr", pbr), ("opacity", opacity), ("bg", bg)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{who}: {name}: a float32 tensor expected")
    want = "[H,W,3] and [H,W,1]" if hwc else "[3,H,W] and [1,H,W]"
    c = 2 if hwc else 0
    if pbr.dim() != 3 or opacity.dim() != 3 or pbr.shape[c] != 3 or opacity.shape[c] != 1 or pbr.numel() == 0 or \
            tuple(pbr.shape[:c] + pbr.shape[c + 1:]) != tuple(opacity.shape[:c] + opacity.shape[c + 1:]):
        raise ValueError(f"{who}: shape mismatch: pbr and opacity {want} with H, W >= 1 expected in layout "
                         f"{image_layout!r}, got {tuple(pbr.shape)} and {tuple(opacity.shape)}")
    if tuple(bg.shape) != (3,) and bg.shape != pbr.shape:
        raise ValueError(f"{who}: shape mismatch: bg [3] or an image shaped like pbr expected, got {tuple(bg.shape)}")
    if bg.requires_grad:
        raise ValueError(f"{who}: no gradient with respect to bg (detach it)")
    if (tone == "gamma") != (gamma is not None):
        raise ValueError(f"{who}: gamma is given with tone 'gamma' and with no other, got tone {tone!r} and gamma "
                         f"{'None' if gamma is None else 'given'}")
    if gamma is not None and (not isinstance(gamma, torch.Tensor) or gamma.dtype != torch.float32 or gamma.numel() != 1):
        raise ValueError(f"{who}: gamma: a float32 tensor of one element expected")
    for name, t in (("opacity", opacity), ("bg", bg), ("gamma", gamma)):
        if t is not None and t.device != pbr.device:
            raise ValueError(f"{who}: {name} is on {t.device}, pbr on {pbr.device}: one device expected")
    if tone in _FORWARD_ONLY and torch.is_grad_enabled() and (pbr.requires_grad or opacity.requires_grad):
        raise ValueError(f"{who}: tone {tone!r} is forward only: detach pbr and opacity, or call under no_grad")
    return _PbrImage.apply(pbr, opacity, gamma, bg, _TONES[tone], hwc)


class _LightLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, diffuse_light):
        ctx.save_for_backward(diffuse_light)
        return _C.pbr.light_loss_forward(diffuse_light)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        diffuse_light, = ctx.saved_tensors
        return _C.pbr.light_loss_backward(diffuse_light, grad.to(torch.float32).reshape(1))


def light_loss(diffuse_light: torch.Tensor) -> torch.Tensor:
    """neilf.py:279-281: F.l1_loss(diffuse_light, its channel mean expanded), as a 0-dim tensor."""
    who = "light_loss"
    if not isinstance(diffuse_light, torch.Tensor) or diffuse_light.dtype != torch.float32:
        raise ValueError(f"{who}: diffuse_light: a float32 tensor expected")
    if diffuse_light.dim() != 2 or diffuse_light.shape[1] != 3:
        raise ValueError(f"{who}: shape mismatch: diffuse_light [P,3] expected, got {tuple(diffuse_light.shape)}")
    return _LightLoss.apply(diffuse_light)


__all__ = ["pbr_image", "light_loss"]
