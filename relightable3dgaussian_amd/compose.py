"""Scene composition for relighting: the reference's `scene_composition` (relighting.py:31-55) with
`set_transform` (scene/gaussian_model.py:237-262) and `create_from_gaussians` (:464-476), followed by the getters,
as HIP kernels (csrc/compose.hip; semantics in include/r3dg_hip.h "scene composition and the points capture").

  set_transform(st, rotation=None, center=None, scale=None, offset=None, transform=None)
      (`GaussianTrainState.set_transform` is this function.) Moves the raw xyz, scaling, rotation and normal
      groups of st.param in place, in one launch. `transform` is a [4,4] (x' = T[:3,:3] x + T[:3,3]); without it
      `center`, `rotation` [3,3], `scale` (a number or [3]) and `offset` apply in that order, as in the
      reference. Each may be a device tensor, a CPU tensor or a (nested) list; a device tensor is never read back.
      Before the kernel the arguments are packed into 19 floats on the device (`pack_transform`): nothing to do
      for a contiguous device `transform`, one host-to-device copy for host values, a fill and a slice copy per
      part for the component form with a part on the device. No argument at all launches nothing.
      The raw rotation stays unnormalised; the SH groups are not rotated (the reference rotates none either), the
      opacity, the PBR groups, everything behind st.total() and the Adam moments are not touched.
  compose_scene(objects, inverse_covariance=True) -> ComposedScene
      objects: [(14-group GaussianTrainState, transform or None)]. What the reference's getters return for the
      composite: every object is transformed and activated straight into the composite's rows, at most two
      launches per object, no intermediate of the objects' size and no change to the objects' own buffers.
      `scaling` is expf(raw) * s where the reference computes exp(log(exp(raw) * s)): a few ulp apart.
  load_scene(scene_dict, max_sh_degree=3, **kw) -> ComposedScene
      scene_dict: the parsed transform.json, {name: {"path": ply, "transform": [16 floats]}}.

No CPU path and no torch fallback: the extension rejects CPU tensors.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _C
from .activation import role_groups

XF_TRANSFORM, XF_CENTER, XF_ROTATION, XF_SCALE, XF_OFFSET = 1, 2, 4, 8, 16  # R3DG_XF_* (include/r3dg_hip.h)


def _part(x, shape, name):
    """x as a float32 tensor of `shape`, on whatever device it lives."""
    t = torch.as_tensor(x, dtype=torch.float32) if not isinstance(x, torch.Tensor) else x.detach()
    if t.dtype != torch.float32:
        raise TypeError(f"set_transform: {name} must be float32, got {t.dtype}")
    if name == "scale" and t.numel() == 1:
        t = t.reshape(1).expand(3)
    if t.numel() != int(torch.Size(shape).numel()):
        raise ValueError(f"set_transform: {name} must hold {tuple(shape)} values, got {tuple(t.shape)}")
    return t.reshape(shape)


def pack_transform(dev, rotation=None, center=None, scale=None, offset=None, transform=None):
    """-> (19 float32 on dev or None, flags): the 4x4 M and the centre c of include/r3dg_hip.h (M's 16 floats
    alone for a full transform). What this costs on the device before the kernel: nothing for no argument and
    for a contiguous `transform` on the device; one host-to-device copy when every part is a host value; a fill
    and one slice copy per part when a part lives on the device (it stays there: no read-back)."""
    if transform is not None:
        # the kernel reads M's first three rows only, so the 16 floats go as they are
        return _part(transform, (4, 4), "transform").reshape(16).to(dev).contiguous(), XF_TRANSFORM
    given = [(center, (3,), "center", XF_CENTER, lambda xf: xf[16:19]),
             (rotation, (3, 3), "rotation", XF_ROTATION, lambda xf: xf[:16].view(4, 4)[:3, :3]),
             (scale, (3,), "scale", XF_SCALE, lambda xf: xf[:16].view(4, 4)[3, :3]),
             (offset, (3,), "offset", XF_OFFSET, lambda xf: xf[:16].view(4, 4)[:3, 3])]
    parts = [(_part(x, shape, name), flag, where) for x, shape, name, flag, where in given if x is not None]
    if not parts:
        return None, 0
    on_host = all(t.device.type == "cpu" for t, _, _ in parts)
    xf = torch.zeros(19, dtype=torch.float32, device="cpu" if on_host else dev)
    flags = 0
    for t, flag, where in parts:
        where(xf).copy_(t)
        flags |= flag
    return xf.to(dev), flags


def _normal_group(st) -> int:
    return [n for n, _ in st.groups].index("normal")


@torch.no_grad()
def set_transform(st, rotation=None, center=None, scale=None, offset=None, transform=None) -> None:
    xf, flags = pack_transform(st.param.device, rotation, center, scale, offset, transform)
    _C.set_transform(st.P, st.widths(), st.roles(), _normal_group(st), st.param, xf, flags)


@dataclass
class ComposedScene:
    """The composite after scene_composition as the reference's getters return it: float32 device tensors
    without autograd history, all contiguous (so `finetune_visibility` updates visibility_dc / visibility_rest in
    place). Rows offsets[i] : offsets[i + 1] (P behind the last) belong to object i."""

    xyz: torch.Tensor              # [P,3]
    scaling: torch.Tensor          # [P,3]
    rotation: torch.Tensor         # [P,4]
    normal: torch.Tensor           # [P,3]
    opacity: torch.Tensor          # [P,1]
    base_color: torch.Tensor       # [P,3]
    roughness: torch.Tensor        # [P,1]
    metallic: torch.Tensor         # [P,1]
    shs: torch.Tensor              # [P,16,3]
    incidents: torch.Tensor        # [P,16,3] zeros
    visibility_dc: torch.Tensor    # [P,1,1]
    visibility_rest: torch.Tensor  # [P,24,1] columns 15..23 zero
    symm_inv: object               # [P,6] or None
    offsets: list
    P: int

    @property
    def visibility(self) -> torch.Tensor:
        """[P,25,1], `render_equation_relight`'s visibility argument."""
        return torch.cat((self.visibility_dc, self.visibility_rest), 1)


_SHAPES = (("xyz", (3,)), ("scaling", (3,)), ("rotation", (4,)), ("normal", (3,)), ("opacity", (1,)),
           ("base_color", (3,)), ("roughness", (1,)), ("metallic", (1,)), ("shs", (16, 3)), ("incidents", (16, 3)),
           ("visibility_dc", (1, 1)), ("visibility_rest", (24, 1)), ("symm_inv", (6,)))


@torch.no_grad()
def compose_scene(objects, inverse_covariance: bool = True) -> ComposedScene:
    objects = list(objects)
    if not objects:
        raise ValueError("compose_scene: no objects")
    for st, _ in objects:
        if len(st.groups) != 14 or not any(n == "base_color" for n, _ in st.groups):
            raise ValueError("compose_scene: every object needs the 14 groups of a PBR state (use_pbr=True)")
    dev = objects[0][0].param.device
    if dev.type != "cuda":
        raise RuntimeError("compose_scene: the states must live on a GPU device (this build has no CPU path)")
    if any(st.param.device != dev for st, _ in objects):
        raise ValueError("compose_scene: the objects live on different devices")
    offsets, P = [], 0
    for st, _ in objects:
        offsets.append(P)
        P += st.P
    outs = {n: torch.empty((P, *s), dtype=torch.float32, device=dev) for n, s in _SHAPES
            if n != "symm_inv" or inverse_covariance}
    outs.setdefault("symm_inv", None)
    slots = [outs[n] for n, _ in _SHAPES]
    for (st, transform), row in zip(objects, offsets):
        xf, flags = pack_transform(dev, transform=transform)
        _C.compose_object(st.P, st.widths(), st.roles(), role_groups(st), st.param, xf, flags, slots, row)
    return ComposedScene(offsets=offsets, P=P, **outs)


def load_scene(scene_dict: dict, max_sh_degree: int = 3, **kw) -> ComposedScene:
    from .trainer import GaussianTrainState

    load_kw = {k: kw.pop(k) for k in ("device",) if k in kw}
    objects = [(GaussianTrainState.load_ply(e["path"], use_pbr=True, max_sh_degree=max_sh_degree, **load_kw),
                e.get("transform")) for e in scene_dict.values()]
    return compose_scene(objects, **kw)


__all__ = ["ComposedScene", "compose_scene", "load_scene", "set_transform", "pack_transform"]
