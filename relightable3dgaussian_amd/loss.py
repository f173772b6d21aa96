"""The training image loss: drop-in for the reference's `utils.loss_utils.ssim` and the fused form of
`calculate_loss`'s L1 + SSIM term (gaussian_renderer/neilf.py:216-222).

`ssim(img1, img2, window_size=11, size_average=True)` -- the reference's signature (loss_utils.py:31-62):
[C,H,W] or [B,C,H,W] f32 GPU tensors, differentiable in `img1`.

`l1_ssim_loss(image, gt, lambda_dssim, image_layout="chw")` -> (loss, stats):
loss = (1 - lambda) * L1 + lambda * (1 - SSIM), stats = {"l1", "ssim", "psnr"} as detached 0-dim device
tensors (psnr as utils/image_utils.py:24-29 and neilf.py:220: per-channel MSE -> 20 log10(1 / sqrt(mse))
-> mean). With image_layout="hwc", `image` is the rasterizer's [H,W,C] output as it is, `gt` stays
[C,H,W], and the gradient comes back [H,W,C].

`bilateral_smooth_loss(data, image, mask)` -- the reference's signature (loss_utils.py:85-96): `data` [1,H,W]
or [3,H,W] (differentiable), `image` [3,H,W], `mask` [1,H,W] or [H,W].

`regularizer_losses(maps, targets, weights, image_layout="chw")` -> (loss, stats): the other eight image terms
of `calculate_loss` (neilf.py:233-321) from one forward launch pair and one backward launch of
csrc/reg_loss.hip (semantics in include/r3dg_hip.h `r3dg_reg_loss_forward`).
  maps     rendered: "opacity", "depth", "roughness", "metallic" [1,H,W]; "normal", "pseudo_normal",
           "base_color" [3,H,W]; with image_layout="hwc" the rasterizer's [H,W,n] blocks as they are
  targets  "gt_image", "mvs_normal" [3,H,W]; "gt_depth", "image_mask" [1,H,W] (no mask: 1 everywhere)
  weights  a mapping (or an object with attributes, such as the reference's `opt`) of lambda_depth,
           lambda_mask_entropy, lambda_normal_render_depth, lambda_normal_mvs_depth, lambda_base_color,
           lambda_base_color_smooth, lambda_metallic_smooth, lambda_roughness_smooth; a missing one is 0
Only terms with a weight > 0 are evaluated, as the reference does. loss = sum of lambda * term carries the
gradient, which comes back in each map's own layout; stats holds each evaluated term under its tb_dict key
("loss_depth", ...) as a detached 0-dim device tensor. pseudo_normal gets no gradient (the reference detaches
it), nor do the targets. The launches do not synchronise with the host; the one host-side wait is the upload
of the eight weights the first time a given set of lambdas is seen (`_lambdas`), so weights that change every
iteration cost one small blocking copy per iteration. There is no double backward.

l1_ssim_loss and ssim are one forward launch pair and one backward launch of csrc/loss.hip (semantics in
include/r3dg_hip.h `r3dg_image_loss_forward`); a few [planes]-sized torch operations turn the per-plane
sums into the scalars. Nothing synchronises with the host. No CPU path and no torch fallback: the
extension rejects CPU tensors. There is no gradient with respect to `img2` / `gt`.
"""
from __future__ import annotations

import functools
from collections.abc import Mapping

import torch
from torch.autograd.function import once_differentiable

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


# ---- the depth, mask, normal, base-colour and smoothness terms (csrc/reg_loss.hip) ---------------------------

# in the order of R3DG_REG_* (include/r3dg_hip.h): weight name, tb_dict key, the maps and targets the term needs
_REG_TERMS = (("lambda_depth", "loss_depth", ("depth", "gt_depth")),
              ("lambda_mask_entropy", "loss_mask_entropy", ("opacity",)),
              ("lambda_normal_render_depth", "loss_normal_render_depth", ("normal", "pseudo_normal")),
              ("lambda_normal_mvs_depth", "loss_normal_mvs_depth", ("normal", "mvs_normal", "gt_depth")),
              ("lambda_base_color", "loss_base_color", ("base_color", "gt_image")),
              ("lambda_base_color_smooth", "loss_base_color_smooth", ("base_color", "gt_image")),
              ("lambda_metallic_smooth", "loss_metallic_smooth", ("metallic", "gt_image")),
              ("lambda_roughness_smooth", "loss_roughness_smooth", ("roughness", "gt_image")))
# in the order of r3dg_reg_loss_inputs: name -> planes
_REG_MAPS = {"opacity": 1, "depth": 1, "normal": 3, "pseudo_normal": 3, "base_color": 3, "roughness": 1, "metallic": 1}
_REG_TARGETS = {"gt_image": 3, "gt_depth": 1, "image_mask": 1, "mvs_normal": 3}
_REG_ORDER = tuple(_REG_MAPS) + tuple(_REG_TARGETS)
_REG_GRADS = ("opacity", "depth", "normal", "base_color", "roughness", "metallic")  # _C.reg_loss_backward's result


@functools.lru_cache(maxsize=64)
def _lambdas(lams: tuple, device: torch.device) -> torch.Tensor:
    """The eight weights on the device, uploaded once per distinct set (the 64 most recent are kept). The
    upload is a copy from pageable host memory, which waits for the host: with constant weights it happens on
    the first call only, but a caller whose lambdas follow a schedule pays it on every change, and a first
    call cannot be part of a graph capture (call once before capturing)."""
    return torch.tensor(lams, dtype=torch.float32, device=device)


class _RegLoss(torch.autograd.Function):
    """The eleven maps (None: absent) -> loss = sum of lambda * term, values [8] (not differentiable)."""

    @staticmethod
    def forward(ctx, terms, hwc, H, W, lam, *maps):
        values, count = _C.reg_loss_forward(list(maps), H, W, terms, hwc)
        ctx.present = [m is not None for m in maps]
        ctx.save_for_backward(count, lam, *[m for m in maps if m is not None])
        ctx.geometry = (terms, hwc, H, W)
        loss = (values * lam).sum()
        ctx.mark_non_differentiable(values)
        return loss, values

    @staticmethod
    @once_differentiable
    def backward(ctx, grad, _):
        count, lam, *given = ctx.saved_tensors
        it = iter(given)
        maps = [next(it) if p else None for p in ctx.present]
        terms, hwc, H, W = ctx.geometry
        need = ctx.needs_input_grad[5:]
        want = sum(1 << i for i, name in enumerate(_REG_GRADS) if need[_REG_ORDER.index(name)])
        out = _C.reg_loss_backward(maps, H, W, terms, hwc, count, lam, grad.to(torch.float32).reshape(1), want)
        grads = [None] * len(_REG_ORDER)
        for name, g in zip(_REG_GRADS, out):
            grads[_REG_ORDER.index(name)] = g
        return (None, None, None, None, None, *grads)


def _reg_shapes(who, given, hwc):
    """(H, W) shared by every given map; ValueError on anything else."""
    hw = None
    for name, t in given.items():
        n = _REG_MAPS.get(name) or _REG_TARGETS[name]
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"{who}: {name}: a 3-D tensor expected")
        pixel_major = hwc and name in _REG_MAPS
        planes, mine = (t.shape[2], tuple(t.shape[:2])) if pixel_major else (t.shape[0], tuple(t.shape[1:]))
        if planes != n or (hw is not None and mine != hw):
            raise ValueError(f"{who}: shape mismatch: {name} {'[H,W,%d]' % n if pixel_major else '[%d,H,W]' % n} "
                             f"{'' if hw is None else 'with H, W = %s ' % (hw,)}expected, got {tuple(t.shape)}")
        hw = mine
    return hw


def regularizer_losses(maps, targets, weights, image_layout: str = "chw"):
    """The depth, mask-entropy, normal, base-colour and smoothness terms of calculate_loss
    (neilf.py:233-321) with weight > 0, fused: (sum of lambda * term, {tb_dict key: term})."""
    who = "regularizer_losses"
    if image_layout not in ("chw", "hwc"):
        raise ValueError(f"{who}: image_layout 'chw' or 'hwc' expected, got {image_layout!r}")
    hwc = image_layout == "hwc"
    for what, got, known in (("map", maps, _REG_MAPS), ("target", targets, _REG_TARGETS)):
        unknown = sorted(set(got) - set(known))
        if unknown:
            raise ValueError(f"{who}: unknown {what} {unknown}; known: {sorted(known)}")
    get = weights.get if isinstance(weights, Mapping) else (lambda k, d: getattr(weights, k, d))
    lams = tuple(float(get(name, 0.0) or 0.0) for name, _, _ in _REG_TERMS)
    given = {k: v for k, v in {**maps, **targets}.items() if v is not None}
    terms = 0
    for i, (name, _, needs) in enumerate(_REG_TERMS):
        if lams[i] > 0:
            missing = [k for k in needs if k not in given]
            if missing:
                raise ValueError(f"{who}: {name} > 0 needs {missing}")
            terms |= 1 << i
    for name in _REG_TARGETS:
        if name in given and given[name].requires_grad:
            raise ValueError(f"{who}: no gradient with respect to {name} (detach it)")
    if not given:
        raise ValueError(f"{who}: no map given")
    H, W = _reg_shapes(who, given, hwc)
    first = next(iter(given.values()))
    if terms == 0:
        return torch.zeros((), dtype=torch.float32, device=first.device), {}
    lam = _lambdas(tuple(l if terms >> i & 1 else 0.0 for i, l in enumerate(lams)), first.device)
    loss, values = _RegLoss.apply(terms, hwc, H, W, lam, *[given.get(k) for k in _REG_ORDER])
    return loss, {key: values[i].detach() for i, (_, key, _) in enumerate(_REG_TERMS) if terms >> i & 1}


def bilateral_smooth_loss(data: torch.Tensor, image: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """utils/loss_utils.py:85 `bilateral_smooth_loss`: the mean of G(data) * exp(-G(image)) * mask, with G the
    sum of the absolute Sobel responses of the channel mean."""
    who = "bilateral_smooth_loss"
    if image.requires_grad or (isinstance(mask, torch.Tensor) and mask.requires_grad):
        raise ValueError(f"{who}: no gradient with respect to image / mask (detach them)")
    if data.dim() != 3 or data.shape[0] not in (1, 3):
        raise ValueError(f"{who}: data [1,H,W] or [3,H,W] expected, got {tuple(data.shape)}")
    if image.dim() != 3 or image.shape[0] != 3 or image.shape[1:] != data.shape[1:]:
        raise ValueError(f"{who}: shape mismatch: image [3,H,W] with data's H, W expected, got {tuple(image.shape)}")
    if mask.dim() == 2:
        mask = mask[None]
    if mask.dim() != 3 or mask.shape[0] != 1 or mask.shape[1:] != data.shape[1:]:
        raise ValueError(f"{who}: shape mismatch: mask [1,H,W] or [H,W] with data's H, W expected, got {tuple(mask.shape)}")
    slot, name = ("base_color", "lambda_base_color_smooth") if data.shape[0] == 3 else ("roughness", "lambda_roughness_smooth")
    return regularizer_losses({slot: data}, {"gt_image": image, "image_mask": mask}, {name: 1.0})[0]


__all__ = ["ssim", "l1_ssim_loss", "bilateral_smooth_loss", "regularizer_losses"]
