"""Generate tests/golden/compose.npz from the REFERENCE's own code (CPU, float32).

Runs the reference checkout's utils.general_utils.rotation_to_quaternion / quaternion_multiply and torch's exp,
log, matmul, composed as scene/gaussian_model.py:237-262 (set_transform) composes them; torch.cat per attribute
as :464-476 (create_from_gaussians), the visibility_rest padding and the zeroed incident SH of
relighting.py:46-53, then the getters (make_golden_activation.getters); and the body of relighting.py:89-123
(render_points) as its sequence of torch operations. The draws are tests/compose_ref64.py's. Stores inputs and
outputs only (data, no reference source).

  st_<group>                the raw parameters of the set_transform draw (P = 257; xyz, scaling, rotation, normal)
  st_<kind>_kw_<name>       set_transform's arguments, kind in compose_ref64.KINDS
  st_<kind>_<group>         the four raw groups afterwards
  sc_<i>_<group>            object i's raw parameters (the incident groups are left out: they are zeroed),
  sc_<i>_transform          its [4,4]
  sc_out_<field>            the composite's getters (ComposedScene's fields)
  pt_xyz, pt_color, pt_view, pt_K, pt_bg, pt_out_rgb    the points capture, H = 37, W = 53

The archive is written with fixed zip timestamps and one thread, so it regenerates byte for byte.

Usage:  python tests/golden/make_golden_compose.py [--reference /root/reference]
        python tests/golden/make_golden_compose.py --floors   (the FLOORS of tests/compose_ref64.py)
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_golden import CpuMode, load_reference  # noqa: E402
from make_golden_activation import getters  # noqa: E402
from make_golden_relight import write_npz  # noqa: E402

OUT = os.path.join(HERE, "compose.npz")
DEFAULT_REFERENCE = "/root/reference"
SCENE_INPUTS = [g for g in ("xyz", "normal", "rotation", "scaling", "opacity", "f_dc", "f_rest", "base_color",
                            "roughness", "metallic", "visibility_dc", "visibility_rest")]
SCENE_FIELDS = ("xyz", "scaling", "rotation", "normal", "opacity", "base_color", "roughness", "metallic", "shs",
                "incidents", "visibility_dc", "visibility_rest", "symm_inv")


def ref_set_transform(gu, t: dict, rotation=None, center=None, scale=None, offset=None, transform=None) -> dict:
    """What gaussian_model.py:237-262 computes, on the tensors t (name -> tensor): the same torch operations on
    the same operands (torch.exp / log, matmul with the transposed matrix, the reference's own
    rotation_to_quaternion and quaternion_multiply), arranged as this project's restatement is."""
    out = dict(t)

    def rescale(s):
        out["scaling"] = torch.log(torch.exp(out["scaling"]) * s)

    def turn(R):
        out["normal"] = out["normal"] @ R.T
        out["rotation"] = gu.quaternion_multiply(gu.rotation_to_quaternion(R[None]), out["rotation"])

    if transform is not None:
        A = transform[:3, :3]
        s = A.norm(dim=-1)
        rescale(s)
        homogeneous = torch.cat([out["xyz"], torch.ones_like(out["xyz"][:, :1])], dim=-1)
        out["xyz"] = (homogeneous @ transform.T)[:, :3]
        turn(A / s[:, None])
        return out
    if center is not None:
        out["xyz"] = out["xyz"] - center
    if rotation is not None:
        out["xyz"] = out["xyz"] @ rotation.T
        turn(rotation)
    if scale is not None:
        out["xyz"] = out["xyz"] * scale
        rescale(scale)
    if offset is not None:
        out["xyz"] = out["xyz"] + offset
    return out


def ref_render_points(xyz, color, view, K, H, W, bg):
    """What relighting.py:89-123 computes (`view` is camera.world_view_transform): its projection as the same
    torch operations (homogeneous matmul, matmul with K.T, division, .long()), then its z-buffer loop, two
    index_put per pass until no point is nearer than the buffer. -> (rgb [3,H,W], passes)"""
    ones = torch.ones_like(xyz[:, :1])
    cam = (torch.cat([xyz, ones], dim=-1) @ view.transpose(0, 1).T)[:, :3]
    projected = cam @ K.T
    pixel = (projected[:, :2] / projected[:, 2:]).long()
    col, row = pixel[:, 0], pixel[:, 1]
    inside = torch.logical_and(torch.logical_and(row >= 0, row < H), torch.logical_and(col >= 0, col < W))
    col, row, z, color = col[inside], row[inside], cam[:, 2][inside], color[inside]
    depth = torch.full((H, W), 10000.0)
    rgb = bg[:, None, None].expand(3, H, W).clone()
    passes = 0
    while True:
        nearer = depth[row, col] > z
        if nearer.sum() == 0:
            return rgb, passes
        depth[row[nearer], col[nearer]] = z[nearer]
        rgb[:, row[nearer], col[nearer]] = color[nearer].transpose(-1, -2)
        passes += 1


def generate(ref: str) -> dict:
    from tests import compose_ref64 as c64

    torch.set_num_threads(1)
    res = {}
    tt = torch.from_numpy
    with CpuMode(), torch.no_grad():
        _, _, _, gu = load_reference(ref)
        c = c64.draw_set_transform_case()
        for g in c64.MOVED:
            res[f"st_{g}"] = c[g]
        for i, kind in enumerate(c64.KINDS):
            kw = c64.draw_kwargs(kind, 100 + i)
            for k, v in kw.items():
                res[f"st_{kind}_kw_{k}"] = v
            # a one-element scale is the reference's scalar
            args = {k: (tt(v).reshape(()) if v.size == 1 else tt(v)) for k, v in kw.items()}
            out = ref_set_transform(gu, {g: tt(c[g]) for g in c64.MOVED}, **args)
            for g in c64.MOVED:
                res[f"st_{kind}_{g}"] = out[g].numpy().copy()

        moved = []
        for i, (c, T) in enumerate(c64.draw_scene()):
            for g in SCENE_INPUTS:
                res[f"sc_{i}_{g}"] = c[g]
            res[f"sc_{i}_transform"] = T
            t = {g: tt(v) for g, v in c.items()}
            moved.append(ref_set_transform(gu, t, transform=tt(T)))
        comp = {g: torch.cat([m[g] for m in moved], dim=0) for g in moved[0]}  # create_from_gaussians
        n = comp["xyz"].shape[0]
        comp["visibility_rest"] = torch.cat([comp["visibility_rest"], torch.zeros(n, 5 ** 2 - 4 ** 2, 1)], dim=1)
        comp["incidents_dc"][:] = 0
        comp["incidents_rest"][:] = 0
        out = getters(gu, comp, None, comp["rotation"])
        out["visibility_dc"], out["visibility_rest"] = comp["visibility_dc"], comp["visibility_rest"]
        for k in SCENE_FIELDS:
            res[f"sc_out_{k}"] = out[k].numpy().copy()

        pt = c64.draw_points_case()
        for k, v in pt.items():
            res[f"pt_{k}"] = v
        res["pt_bg"] = c64.PT_BG
        rgb, passes = ref_render_points(tt(pt["xyz"]), tt(pt["color"]), tt(pt["view"]), tt(pt["K"]), c64.PT_H,
                                        c64.PT_W, tt(c64.PT_BG))
        print("render_points: the reference's loop took", passes, "passes")
        res["pt_out_rgb"] = rgb.numpy().copy()
    return res


def set_transform_kwargs(g, kind: str) -> dict:
    pre = f"st_{kind}_kw_"
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def scene_objects(g) -> list:
    """[(raw parameters, transform)] of the stored scene (the incident groups as zeros: they are not read)."""
    from tests import compose_ref64 as c64

    objs = []
    for i, P in enumerate(c64.SCENE_P):
        c = {k: g[f"sc_{i}_{k}"] for k in SCENE_INPUTS}
        c["incidents_dc"] = np.zeros((P, 1, 3), np.float32)
        c["incidents_rest"] = np.zeros((P, 15, 3), np.float32)
        objs.append((c, g[f"sc_{i}_transform"]))
    return objs


def measure(g) -> dict:
    """row_err of every stored output against ref64, the worst over the cases."""
    from tests import activation_ref64 as a64
    from tests import compose_ref64 as c64

    worst = {}
    c = {k: g[f"st_{k}"] for k in c64.MOVED}
    for kind in c64.KINDS:
        ref = c64.set_transform(c, **set_transform_kwargs(g, kind))
        for k in c64.MOVED:
            e = a64.row_err(g[f"st_{kind}_{k}"], ref[k])
            print(f"st {kind:10s} {k:16s} {e:.3e}")
            worst[f"st_{k}"] = max(worst.get(f"st_{k}", 0.0), e)
    ref = c64.compose(scene_objects(g))
    for k in SCENE_FIELDS:
        e = a64.row_err(g[f"sc_out_{k}"], ref[k])
        print(f"scene {k:24s} {e:.3e}")
        worst[k] = e
    return worst


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=DEFAULT_REFERENCE)
    ap.add_argument("--floors", action="store_true", help="print golden-vs-ref64 distances of the stored file")
    args = ap.parse_args()
    if args.floors:
        for k, v in measure(np.load(OUT)).items():
            print(f"floor {k:22s} {v:.3e}")
        return
    write_npz(OUT, generate(args.reference))
    print("written", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
