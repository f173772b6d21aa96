"""Scene composition and the points capture on the MI355X (`compose.compose_scene`, `relight.render_points`;
csrc/compose.hip) against the same work as the torch code a caller had to write before.

  compose   three objects of --P Gaussians each (14 groups, a general 4x4 transform each), with and without
            symm_inv. Composed form: set_transform as the reference's tensor operations per object, torch.cat of
            the 14 groups, the visibility_rest padding, the zeroed incident SH, then the getters
            (tools/bench_activation.py `composed`). The fused form's algorithmic bytes (what it must read and
            write, from the shapes: 83 floats in, 140 out, +6 for symm_inv, per Gaussian) over its time give the
            achieved rate and its share of the 6.3 TB/s copy rate, next to the activation's.
            The same number of rows as one object (two launches in place of six) is timed as well.
  points    --points points into --size x --size, "spread" over the image (about 1.6 points per pixel) and
            "deep" (the same points into the central eighth of each axis, about 100 per pixel). Loop form:
            relighting.py:89-123 as its torch operations on the same GPU, with its `mask.sum() == 0` read-back
            per pass; its pass count is reported.
Each is timed both ways in this process with CUDA events (median of --iters after two warm-up calls); launches
from one profiled call outside the timed window. Nothing is asserted about any time.

Usage: python tools/bench_compose.py [--P 333000] [--points 1000000] [--size 800] [--iters 20]
                                     [--out profiles/compose/compose_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_activation import COPY_RATE, composed, launches, make_state, timed  # noqa: E402

FLOATS_IN, FLOATS_OUT = 83, 140  # per Gaussian: the groups read (the incident SH are not) / the fields written


def draw_transform(seed):
    rng = np.random.default_rng(seed)
    axis = rng.normal(0, 1, 3)
    axis /= np.linalg.norm(axis)
    th = rng.uniform(0.2, 2.2)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.array([0.7, 1.3, 2.1])[:, None] * (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K))
    T[:3, 3] = rng.normal(0, 2, 3)
    return torch.tensor(T, dtype=torch.float32, device="cuda")


def rotation_to_quaternion(R):
    """utils/general_utils.py:105-117 as tensor operations."""
    qw = torch.sqrt((1 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]).clamp_min(1e-7)) / 2
    q = torch.stack((qw, (R[:, 2, 1] - R[:, 1, 2]) / (4 * qw), (R[:, 0, 2] - R[:, 2, 0]) / (4 * qw),
                     (R[:, 1, 0] - R[:, 0, 1]) / (4 * qw)), dim=-1)
    return torch.nn.functional.normalize(q, dim=-1)


def quaternion_multiply(q1, q2):
    w1, x1, y1, z1 = q1[:, 0], q1[:, 1], q1[:, 2], q1[:, 3]
    w2, x2, y2, z2 = q2[:, 0], q2[:, 1], q2[:, 2], q2[:, 3]
    return torch.stack((w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2), dim=1)


def torch_compose(states, transforms, symm):
    """scene_composition (relighting.py:31-55) and the getters, as a caller composes them around the operators."""
    moved = []
    for st, T in zip(states, transforms):
        p = {n: st.view(n) for n, _ in st.groups}
        A = T[:3, :3]
        s = A.norm(dim=-1)
        R = A / s[:, None]
        ones = torch.ones_like(p["xyz"][:, :1])
        p.update(scaling=torch.log(torch.exp(p["scaling"]) * s),
                 xyz=(torch.cat([p["xyz"], ones], dim=-1) @ T.T)[:, :3], normal=p["normal"] @ R.T,
                 rotation=quaternion_multiply(rotation_to_quaternion(R[None]), p["rotation"]))
        moved.append(p)
    comp = {n: torch.cat([m[n] for m in moved], dim=0) for n in moved[0]}
    n = comp["xyz"].shape[0]
    comp["visibility_rest"] = torch.cat([comp["visibility_rest"], torch.zeros(n, 9, 1, device="cuda")], dim=1)
    comp["incidents_dc"][:] = 0
    comp["incidents_rest"][:] = 0
    return composed(comp, comp["xyz"].new_zeros(3), symm)


def measure_compose(P, iters):
    from relightable3dgaussian_amd.compose import compose_scene

    states = [make_state(P, seed=i) for i in range(3)]
    transforms = [draw_transform(10 + i) for i in range(3)]
    objects = list(zip(states, transforms))
    res = {"objects": 3, "P_each": P, "iters": iters, "floats_in": FLOATS_IN, "floats_out": FLOATS_OUT}
    with torch.no_grad():
        a, b = compose_scene(objects, True), torch_compose(states, transforms, True)
        res["xyz_max_abs_diff_vs_composed"] = float((a.xyz - b["xyz"]).abs().max())
        for symm in (False, True):
            tag = "_symm" if symm else ""
            nbytes = 4 * 3 * P * (FLOATS_IN + FLOATS_OUT + (6 if symm else 0))
            f = timed(lambda: compose_scene(objects, symm), iters)
            c = timed(lambda: torch_compose(states, transforms, symm), iters)
            res.update({f"fused{tag}_ms": f, f"composed{tag}_ms": c, f"ratio{tag}": c / f, f"fused{tag}_bytes": nbytes,
                        f"fused{tag}_TBps": nbytes / f / 1e9, f"fused{tag}_of_copy_rate": nbytes / (f * 1e-3) / COPY_RATE,
                        f"fused{tag}_launches": launches(lambda: compose_scene(objects, symm)),
                        f"composed{tag}_launches": launches(lambda: torch_compose(states, transforms, symm))})
        # the same rows as ONE object (two launches in place of six): what the per-object launches cost
        one =[(make_state(3 * P, seed=5), transforms[0])]
        f = timed(lambda: compose_scene(one, False), iters)
        nbytes = 4 * 3 * P * (FLOATS_IN + FLOATS_OUT)
        res.update({"fused_one_object_ms": f, "fused_one_object_TBps": nbytes / f / 1e9,
                    "fused_one_object_of_copy_rate": nbytes / (f * 1e-3) / COPY_RATE})
    return res


def loop_render_points(xyz, color, view, K, H, W, bg):
    """What relighting.py:89-123 does on the GPU (`view` is camera.world_view_transform): the projection as
    tensor operations, then the z-buffer loop of two index_put per pass with a `sum() == 0` read-back each.
    -> (rgb, passes)"""
    ones = torch.ones_like(xyz[:, :1])
    cam = (torch.cat([xyz, ones], dim=-1) @ view.transpose(0, 1).T)[:, :3]
    projected = cam @ K.T
    pixel = (projected[:, :2] / projected[:, 2:]).long()
    col, row = pixel[:, 0], pixel[:, 1]
    inside = torch.logical_and(torch.logical_and(row >= 0, row < H), torch.logical_and(col >= 0, col < W))
    pixel, z, color = pixel[inside], cam[:, 2][inside], color[inside]
    depth = torch.full((H, W), 10000.0, device=xyz.device)
    rgb = torch.full((3, H, W), bg, device=xyz.device)
    passes = 0
    while True:
        nearer = depth[pixel[:, 1], pixel[:, 0]] > z
        if nearer.sum() == 0:
            return rgb, passes
        hit = pixel[nearer]  # one boolean gather per pass for both coordinates, as the reference has it
        depth[hit[:, 1], hit[:, 0]] = z[nearer]
        rgb[:, hit[:, 1], hit[:, 0]] = color[nearer].transpose(-1, -2)
        passes += 1


def measure_points(N, size, iters):
    from relightable3dgaussian_amd.relight import render_points

    g = torch.Generator(device="cuda").manual_seed(3)
    f = float(size)
    K = torch.tensor([[f, 0, f / 2], [0, f, f / 2], [0, 0, 1]], device="cuda")
    view = torch.eye(4, device="cuda")
    color = torch.rand((N, 3), device="cuda", generator=g)
    res = {"points": N, "H": size, "W": size, "iters": iters}
    for name, spread in (("spread", 1.0), ("deep", 0.125)):
        z = 1.0 + 4.0 * torch.rand(N, device="cuda", generator=g)
        uv = (torch.rand((N, 2), device="cuda", generator=g) - 0.5) * spread  # (u - cx) / f
        xyz = torch.cat([uv * z[:, None], z[:, None]], dim=1).contiguous()
        a = (xyz, color, view, K, size, size)
        with torch.no_grad():
            rgb, depth = render_points(*a, 0.0, return_depth=True)
            _, passes = loop_render_points(*a, 0.0)
            fused = timed(lambda: render_points(*a, 0.0), iters)
            loop = timed(lambda: loop_render_points(*a, 0.0), iters)
            res[name] = {"fused_ms": fused, "loop_ms": loop, "ratio": loop / fused, "loop_passes": passes,
                         "covered_pixels": int((depth < 10000).sum()),
                         "fused_launches": launches(lambda: render_points(*a, 0.0)),
                         "loop_launches": launches(lambda: loop_render_points(*a, 0.0))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=333_000, help="Gaussians per object (three objects)")
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compose", "compose_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_compose: needs the GPU (no CPU path, and a CPU time says nothing)")
    line = json.dumps({"copy_rate_Bps": COPY_RATE, "compose": measure_compose(args.P, args.iters),
                       "render_points": measure_points(args.points, args.size, args.iters)})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
