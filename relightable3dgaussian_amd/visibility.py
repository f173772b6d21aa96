"""Visibility baking: everything the reference does around `RayTracer.trace_visibility` to produce the
per-Gaussian visibility that the render equations read (csrc/bvh.hip, csrc/visibility.hip; semantics in
include/r3dg_hip.h).

  fibonacci_dirs(normals, sample_num) -> [P, Ns, 3]
      `sample_incident_rays(normals, False, sample_num)`'s directions in one launch, each evaluated in double
      and rounded once (the reference's float32 sample angle is off by up to 3e-5 rad at sample 383).
  precompute_visibility(raytracer, means3D, symm_inv, opacity, normals, sample_num) -> [P, Ns, 1]
      relighting.py:62-84 (`update_visibility` without --bake) in one call and no chunk loop: Ns Fibonacci
      rays from every centre, the directions computed in the tracer. The result is
      `render_equation_relight(..., visibility_precompute=...)`'s argument as it stands.
  visibility_sh_loss(visibility_dc, visibility_rest, rays_d, traced, normals=None, index=None) -> 0-dim
      neilf.py:331-346 around the trace: mean |traced - clamp(eval_sh(sh[index], rays_d) + 0.5, 0, 1)|,
      differentiable in the two SH tensors. `normals` [P, 3] flips each direction into its Gaussian's
      hemisphere first (the call site's `rays_d[mask] *= -1`; pass None for directions already flipped).
  finetune_visibility(visibility_dc, visibility_rest, raytracer, means3D, symm_inv, opacity, normals,
                      iterations=1000, lr=1e-2, generator=None) -> [iterations] losses
      scene/gaussian_model.py:428-462 (`--bake`): per iteration one torch.randn, one trace from the centres
      and one fused launch for loss, gradient and Adam. Unlike the reference, which evaluates a copy of the
      coefficients taken before the loop (`get_visibility` is a torch.cat), every iteration evaluates the
      current coefficients, as the training loss does; the first iteration is the same either way.

An `index` entry outside [0, P) is the caller's error: it is not checked (that would read the device array
back), the kernels read nothing for it, and the trace's visibility / the loss come out NaN.
No CPU path and no torch fallback: the extension rejects CPU tensors.
"""
from __future__ import annotations

import torch

from . import _C


def fibonacci_dirs(normals: torch.Tensor, sample_num: int) -> torch.Tensor:
    return _C.fibonacci_dirs(normals, int(sample_num))


@torch.no_grad()
def precompute_visibility(raytracer, means3D, symm_inv, opacity, normals, sample_num: int) -> torch.Tensor:
    _, vis = _C.trace_bvh_opacity_centres(raytracer.tree, raytracer.aabb, None, means3D, symm_inv, opacity, normals,
                                          None, False, int(sample_num), False)
    return vis.unsqueeze(-1)


class _VisibilityShLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, visibility_dc, visibility_rest, rays_d, traced, normals, index):
        ctx.save_for_backward(visibility_dc, visibility_rest, rays_d, traced)
        ctx.normals, ctx.index = normals, index
        return _C.visibility_sh_loss_forward(visibility_dc, visibility_rest, rays_d, traced, normals, index)

    @staticmethod
    def backward(ctx, grad):
        dc, rest, rays_d, traced = ctx.saved_tensors
        g_dc, g_rest = _C.visibility_sh_loss_backward(dc, rest, rays_d, traced, ctx.normals, ctx.index,
                                                      grad.to(torch.float32).contiguous())
        return g_dc.view_as(dc), g_rest.view_as(rest), None, None, None, None


def visibility_sh_loss(visibility_dc, visibility_rest, rays_d, traced, normals=None, index=None) -> torch.Tensor:
    for name, t in (("rays_d", rays_d), ("traced", traced), ("normals", normals)):
        if t is not None and t.requires_grad:
            raise ValueError(f"visibility_sh_loss: {name} must not require grad (the loss is differentiable in the "
                             "two SH tensors only)")
    return _VisibilityShLoss.apply(visibility_dc, visibility_rest, rays_d, traced, normals, index)


@torch.no_grad()
def finetune_visibility(visibility_dc, visibility_rest, raytracer, means3D, symm_inv, opacity, normals,
                        iterations: int = 1000, lr: float = 1e-2, generator=None, betas=(0.9, 0.999),
                        eps: float = 1e-8) -> torch.Tensor:
    # fresh moments, as the reference builds a fresh optimizer
    m_dc, m_rest = torch.zeros_like(visibility_dc), torch.zeros_like(visibility_rest)
    v_dc, v_rest = torch.zeros_like(visibility_dc), torch.zeros_like(visibility_rest)
    losses = torch.empty(iterations, dtype=torch.float32, device=visibility_dc.device)
    P = means3D.shape[0]
    for it in range(iterations):
        rays_d = torch.randn((P, 3), dtype=torch.float32, device=means3D.device, generator=generator)
        # the trace flips the directions below the normal; the fit step decides the same flip from the same
        # arrays with the same device function
        _, traced = _C.trace_bvh_opacity_centres(raytracer.tree, raytracer.aabb, rays_d, means3D, symm_inv, opacity,
                                                 normals, None, True, 1, False)
        _C.visibility_sh_fit_step(visibility_dc, visibility_rest, rays_d, traced, normals, m_dc, m_rest, v_dc, v_rest,
                                  it + 1, float(lr), float(betas[0]), float(betas[1]), float(eps), losses, it)
    return losses


__all__ = ["fibonacci_dirs", "precompute_visibility", "visibility_sh_loss", "finetune_visibility"]
