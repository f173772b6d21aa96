"""The relighting render equation: what the reference's `relighting.py` runs for every frame
(gaussian_renderer/neilf_composite.py) and its environment-map light (scene/envmap.py), as one HIP
kernel each (csrc/relight.hip, semantics in include/r3dg_hip.h `r3dg_render_equation_relight`).

`EnvLight(envmap, scale=1.0)` -- the reference's class over an [He, We, 3] float32 GPU tensor in place of an
.hdr path (decoding .hdr needs cv2). `.transform` is the optional [3, 3] light rotation and
`.direct_light(dirs, transform=None)` the lat-long bilinear lookup for directions of any leading shape.

`render_equation_relight(base_color, roughness, metallic, normals, viewdirs, incidents, env_light,
visibility, sample_num, bake, visibility_precompute=None)` -> (rgb, extra_results, features) replaces the
chunk loop over `rendering_equation_python` and the `torch.cat` of nine tensors
(neilf_composite.py:106-133): `features` [P, 21] goes to the rasterizer as it is; `rgb` and the four
`extra_results` entries (the reference's keys) are views into it.
  env_light   None (no global light), an object with `get_env_shs` [1, S, 3] (the reference's
              DirectLightEnv), or an EnvLight
  visibility  the baked visibility SH [P, S, 1], read when `bake` is true
  bake=False  the per-sample traced visibility `visibility_precompute` [P, Ns] or [P, Ns, 1]
              (pc._visibility_tracing); without it a ValueError, as the reference raises
`render_points(xyz, color, world_view_transform, intrinsics, H, W, bg, return_depth=False)` is the script's
`points` capture (relighting.py:89-123), a z-buffered point cloud (csrc/compose.hip `r3dg_render_points`).
`env_background(light, intrinsics, c2w, H, W)` -> [H, W, 3] is the environment behind the object
(neilf_composite.py:209-215) in one launch, without the direction image (`r3dg_env_background`).

Each SH width is 0..25. Forward only: the relighting script runs under torch.no_grad(). No CPU path and
no torch fallback: the extension rejects CPU tensors.
"""
from __future__ import annotations

import torch

from . import _C

LIGHT_NONE, LIGHT_SH, LIGHT_MAP = 0, 1, 2  # R3DG_LIGHT_* (include/r3dg_hip.h)

# column ranges of `features` (neilf_composite.py:129-133)
FEATURE_COLUMNS = {"rgb": (0, 3), "normal": (3, 6), "base_color": (6, 9), "roughness": (9, 10), "metallic": (10, 11),
                   "incident_lights": (11, 14), "local_incident_lights": (14, 17),
                   "global_incident_lights": (17, 20), "incident_visibility": (20, 21)}


class EnvLight(torch.nn.Module):
    """scene/envmap.py EnvLight over a tensor: `envmap` [He, We, 3] float32 on the GPU, multiplied by `scale`
    as the reference's loader does."""

    def __init__(self, envmap: torch.Tensor, scale: float = 1.0):
        super().__init__()
        if envmap.dim() != 3 or envmap.shape[2] != 3:
            raise ValueError("EnvLight: envmap must be [He, We, 3], got %s" % (tuple(envmap.shape),))
        self.scale = scale
        self.device = envmap.device
        self.envmap = (envmap.detach().to(torch.float32) * scale).contiguous()
        self.transform = None

    def direct_light(self, dirs: torch.Tensor, transform: torch.Tensor | None = None) -> torch.Tensor:
        """Light from the map along dirs [..., 3] -> [..., 3]; `transform`, else `self.transform`, rotates
        the directions first (d' = T d)."""
        if transform is None:
            transform = self.transform
        return _C.envmap_direct_light(dirs, self.envmap, transform)


@torch.no_grad()
def render_equation_relight(base_color, roughness, metallic, normals, viewdirs, incidents, env_light, visibility,
                            sample_num, bake, visibility_precompute=None):
    if not bake and visibility_precompute is None:
        raise ValueError("visibility should be pre-computed.")
    direct_shs = envmap = transform = None
    if env_light is None:
        mode = LIGHT_NONE
    elif isinstance(env_light, EnvLight):
        mode, envmap, transform = LIGHT_MAP, env_light.envmap, env_light.transform
    elif hasattr(env_light, "get_env_shs"):
        mode, direct_shs = LIGHT_SH, env_light.get_env_shs
    else:
        raise TypeError("render_equation_relight: env_light must be None, an EnvLight or an object with get_env_shs")
    features = _C.render_equation_relight(base_color, roughness, metallic, normals, viewdirs, incidents, direct_shs,
                                          visibility if bake else None, int(sample_num), mode, envmap, transform,
                                          None if bake else visibility_precompute)
    cols = {k: features[:, a:b] for k, (a, b) in FEATURE_COLUMNS.items()}
    extra_results = {k: cols[k] for k in ["incident_lights", "local_incident_lights", "global_incident_lights",
                                          "incident_visibility"]}
    return cols["rgb"], extra_results, features


@torch.no_grad()
def env_background(light, intrinsics: torch.Tensor, c2w: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """The environment behind the object (neilf_composite.py:209-215) -> [H, W, 3], in one launch and without
    the [3, H, W] direction image of `Camera.get_world_directions()` (scene/cameras.py:87-99): per pixel (v, u)
    d = normalize(((u - cx) / fx, (v - cy) / fy, 1)) with F.normalize's eps, then c2w[:3, :3] @ d. `light` is an
    `EnvLight` (the lookup `direct_light` runs, with `light.transform`) or the environment SH [1, M, 3],
    M = (deg + 1)^2 <= 25 (`clamp_min(eval_sh(deg, shs, d) + 0.5, 0)`). `intrinsics` [3, 3] and `c2w` [4, 4] or
    [3, 3] are device tensors, read on the device. The result is a valid `bg` image of `display.frame_buffers`
    and of `pbr.pbr_image`."""
    who = "env_background"
    for name, t, shapes in (("intrinsics", intrinsics, ((3, 3),)), ("c2w", c2w, ((4, 4), (3, 3)))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{who}: {name}: a float32 tensor expected")
        if tuple(t.shape) not in shapes:
            raise ValueError(f"{who}: shape mismatch: {name} {' or '.join(str(list(s)) for s in shapes)} expected, "
                             f"got {tuple(t.shape)}")
    if int(H) < 1 or int(W) < 1:
        raise ValueError(f"{who}: H, W >= 1 expected, got {H} x {W}")
    envmap = transform = shs = None
    if isinstance(light, EnvLight):
        envmap, transform = light.envmap, light.transform
    elif isinstance(light, torch.Tensor):
        if light.dtype != torch.float32:
            raise ValueError(f"{who}: light: a float32 tensor expected")
        if light.dim() != 3 or light.shape[0] != 1 or light.shape[2] != 3 or light.shape[1] not in (1, 4, 9, 16, 25):
            raise ValueError(f"{who}: shape mismatch: environment SH [1, M, 3] with M = (deg + 1)^2, deg <= 4 "
                             f"expected, got {tuple(light.shape)}")
        shs = light.detach()
    else:
        raise TypeError(f"{who}: light must be an EnvLight or the environment SH tensor [1, M, 3]")
    for name, t in (("c2w", c2w), ("light", envmap if shs is None else shs), ("light.transform", transform)):
        if t is not None and t.device != intrinsics.device:
            raise ValueError(f"{who}: {name} is on {t.device}, intrinsics on {intrinsics.device}: one device expected")
    return _C.display.env_background(intrinsics, c2w, int(H), int(W), envmap, transform, shs)


@torch.no_grad()
def render_points(xyz, color, world_view_transform, intrinsics, H, W, bg, return_depth: bool = False):
    """The `points` capture (relighting.py:89-123): the z-buffered point cloud -> [3, H, W], with
    return_depth=True also the [H, W] depth (10000 at empty pixels). `world_view_transform` is the reference's
    (transposed) [4, 4], `intrinsics` [3, 3], `bg` a number or [3]. One 64-bit atomic min per point and a resolve
    pass in place of the reference's loop; no host synchronisation.

    A point is projected as the reference does, operation for operation, dropped when its pixel coordinates
    are not finite (z == 0), truncated toward zero as `.long()` (so a coordinate in (-1, 0) lands in column /
    row 0), and kept when it lands inside the image with z < 10000. There is NO near plane, as in the reference:
    a point behind the camera takes part with its negative z and wins its pixel. Every pixel shows its point
    with the smallest z, the smallest index among equal z (the reference leaves that case undefined)."""
    # a background on the device is read there; a host value goes to the kernel by value (no copy)
    bg_dev, bg_value = None, []
    if isinstance(bg, torch.Tensor) and bg.device.type != "cpu":
        bg_dev = bg.detach().to(dtype=torch.float32).reshape(-1)
        bg_dev = (bg_dev.expand(3) if bg_dev.numel() == 1 else bg_dev).contiguous()
    else:
        bg_value = [float(v) for v in torch.as_tensor(bg, dtype=torch.float32).reshape(-1).tolist()]
        bg_value = bg_value * 3 if len(bg_value) == 1 else bg_value
    rgb, depth = _C.render_points(xyz, color, world_view_transform, intrinsics, int(H), int(W), bg_dev, bg_value,
                                  bool(return_depth))
    return (rgb, depth) if return_depth else rgb
