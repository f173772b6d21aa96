"""Visibility baking on the MI355X (relightable3dgaussian_amd/visibility.py) against the same work composed
the way a caller had to before: torch ray arrays -> RayTracer.trace_visibility -> an SH evaluation written as
torch tensor operations (below, with torch autograd) -> torch.optim.Adam.

Three workloads on the two scenes of tools/bench_bvh.py ("volume", "surface"), P Gaussians:
  fit        one finetune_visibility iteration: randn, trace from every centre, loss + gradient + Adam
  loss       one visibility_sh_loss forward and backward with 10k rays (the lambda_visibility term)
  precompute precompute_visibility at Ns = 24 (relighting.py's update_visibility without --bake);
             the composed form chunks as the reference does, so that its ray arrays fit
Each is timed both ways with CUDA events (median of --iters after two warm-up calls); the trace alone is timed
too and the non-trace part reported as the difference, since the trace dominates. Peak memory of the
precompute is torch's max_memory_allocated over one call, beyond what was allocated before it.

Usage: python tools/bench_visibility.py [--P 1000000] [--iters 10] [--scene volume|surface] [--out FILE]
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

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435]


def torch_eval_sh3(sh, d):
    """Degree-3 real SH sum as elementwise tensor operations: sh [R, 16], d [R, 3] -> [R]."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    r = C0 * sh[:, 0] - C1 * y * sh[:, 1] + C1 * z * sh[:, 2] - C1 * x * sh[:, 3]
    r = (r + C2[0] * xy * sh[:, 4] + C2[1] * yz * sh[:, 5] + C2[2] * (2.0 * zz - xx - yy) * sh[:, 6] +
         C2[3] * xz * sh[:, 7] + C2[4] * (xx - yy) * sh[:, 8])
    r = (r + C3[0] * y * (3 * xx - yy) * sh[:, 9] + C3[1] * xy * z * sh[:, 10] +
         C3[2] * y * (4 * zz - xx - yy) * sh[:, 11] + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12] +
         C3[4] * x * (4 * zz - xx - yy) * sh[:, 13] + C3[5] * z * (xx - yy) * sh[:, 14] +
         C3[6] * x * (xx - 3 * yy) * sh[:, 15])
    return r


def torch_fib_dirs(normals, Ns):
    """fibonacci_sphere_sampling(normals, Ns, random_rotate=False) as tensor operations -> [P, Ns, 3]."""
    P = normals.shape[0]
    idx = torch.arange(Ns, device=normals.device, dtype=torch.float32)
    z = 1 - 2 * idx / (2 * Ns - 1)
    rad = torch.sqrt(1 - z * z)
    theta = float(np.pi * (3 - np.sqrt(5))) * idx
    local = torch.stack([torch.sin(theta) * rad, torch.cos(theta) * rad, z], -1)
    v1, v2 = -normals[:, 1], normals[:, 0]
    cp1 = (normals[:, 2] + 1).clamp_min(1e-7)
    R = torch.zeros(P, 3, 3, device=normals.device)
    R[:, 0, 0] = 1 - v2 * v2 / cp1
    R[:, 0, 1] = v1 * v2 / cp1
    R[:, 0, 2] = v2
    R[:, 1, 0] = v1 * v2 / cp1
    R[:, 1, 1] = 1 - v1 * v1 / cp1
    R[:, 1, 2] = -v1
    R[:, 2, 0] = -v2
    R[:, 2, 1] = v1
    R[:, 2, 2] = 1 + (-v2 * v2 - v1 * v1) / cp1
    R = torch.where((normals[:, 2] + 1 > 0)[:, None, None], R, -torch.eye(3, device=normals.device).expand_as(R))
    return torch.nn.functional.normalize((R[:, None] @ local[None, :, :, None])[..., 0], dim=-1)


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts))


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--loss-rays", type=int, default=10000)
    ap.add_argument("--samples", type=int, default=24)
    ap.add_argument("--scene", choices=["volume", "surface"], default="volume")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from bench_bvh import surface_scene
    from relightable3dgaussian_amd import _C, visibility
    from relightable3dgaussian_amd.bvh import RayTracer
    from tests.test_bvh import scene

    torch.cuda.set_device(0)
    P, Ns, K = args.P, args.samples, 16
    sc = scene(P, seed=8, spread=1.0) if args.scene == "volume" else surface_scene(P, seed=8)
    dev = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    means, cov, opac, normals = dev(sc["means"]), dev(sc["cov_inv"]), dev(sc["opacity"]), dev(sc["normals"])
    rt = RayTracer(means, dev(sc["scales"]), dev(sc["rots"]))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    dc0 = 0.3 * torch.randn(P, 1, 1, device="cuda", generator=gen)
    rest0 = 0.3 * torch.randn(P, K - 1, 1, device="cuda", generator=gen)
    res = {"P": P, "K": K, "scene": args.scene, "sample_num": Ns, "loss_rays": args.loss_rays,
           "device": torch.cuda.get_device_name(0), "iters": args.iters}

    # ---- one fit iteration -------------------------------------------------------------------------------
    dc, rest = dc0.clone(), rest0.clone()
    st = [torch.zeros_like(dc), torch.zeros_like(rest), torch.zeros_like(dc), torch.zeros_like(rest)]
    losses = torch.zeros(1, device="cuda")
    d_fixed = torch.randn(P, 3, device="cuda", generator=gen)

    def hip_trace():
        return _C.trace_bvh_opacity_centres(rt.tree, rt.aabb, d_fixed, means, cov, opac, normals, None, True, 1,
                                            False)[1]

    def hip_fit():
        d = torch.randn(P, 3, device="cuda", generator=gen)
        tr = _C.trace_bvh_opacity_centres(rt.tree, rt.aabb, d, means, cov, opac, normals, None, True, 1, False)[1]
        _C.visibility_sh_fit_step(dc, rest, d, tr, normals, *st, 1, 1e-2, 0.9, 0.999, 1e-8, losses, 0)

    pdc, prest = dc0.clone().requires_grad_(True), rest0.clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [pdc], "lr": 1e-2}, {"params": [prest], "lr": 1e-2}])

    def flipped(d, n):
        mask = (d * n).sum(-1) < 0
        d[mask] *= -1
        return d

    d_flipped = flipped(d_fixed.clone(), normals)

    def torch_trace():
        return rt.trace_visibility(means, d_flipped, means, cov, opac, normals)["visibility"]

    def torch_fit():
        d = flipped(torch.randn(P, 3, device="cuda", generator=gen), normals)
        vis = torch.clamp(torch_eval_sh3(torch.cat([pdc, prest], 1)[..., 0], d) + 0.5, 0.0, 1.0)
        tr = rt.trace_visibility(means, d, means, cov, opac, normals)["visibility"]
        loss = torch.nn.functional.l1_loss(tr[:, 0], vis)
        loss.backward()
        opt.step()
        opt.zero_grad()

    res["fit_ms"] = timed(hip_fit, args.iters)
    res["fit_trace_ms"] = timed(hip_trace, args.iters)
    res["fit_non_trace_ms"] = res["fit_ms"] - res["fit_trace_ms"]
    res["fit_composed_ms"] = timed(torch_fit, args.iters)
    res["fit_composed_trace_ms"] = timed(torch_trace, args.iters)
    res["fit_composed_non_trace_ms"] = res["fit_composed_ms"] - res["fit_composed_trace_ms"]

    # ---- the training term: 10k rays, forward and backward --------------------------------------------------
    n = args.loss_rays
    idx = torch.randperm(P, device="cuda", generator=gen)[:n]
    d10 = torch.randn(n, 3, device="cuda", generator=gen)
    ldc, lrest = dc0.clone().requires_grad_(True), rest0.clone().requires_grad_(True)

    def hip_loss_trace():
        return _C.trace_bvh_opacity_centres(rt.tree, rt.aabb, d10, means, cov, opac, normals, idx, True, 1, False)[1]

    def hip_loss():
        tr = hip_loss_trace()
        loss = visibility.visibility_sh_loss(ldc, lrest, d10, tr, normals, idx)
        loss.backward()
        ldc.grad = lrest.grad = None

    d10_flipped = flipped(d10.clone(), normals[idx])

    def torch_loss_trace():
        return rt.trace_visibility(means[idx], d10_flipped, means, cov, opac, normals)["visibility"]

    def torch_loss():
        d = flipped(d10.clone(), normals[idx])
        sh = torch.cat([ldc, lrest], 1)[..., 0][idx]
        vis = torch.clamp(torch_eval_sh3(sh, d) + 0.5, 0.0, 1.0)
        tr = rt.trace_visibility(means[idx], d, means, cov, opac, normals)["visibility"]
        loss = torch.nn.functional.l1_loss(tr[:, 0], vis)
        loss.backward()
        ldc.grad = lrest.grad = None

    res["loss_ms"] = timed(hip_loss, args.iters)
    res["loss_trace_ms"] = timed(hip_loss_trace, args.iters)
    res["loss_non_trace_ms"] = res["loss_ms"] - res["loss_trace_ms"]
    res["loss_composed_ms"] = timed(torch_loss, args.iters)
    res["loss_composed_trace_ms"] = timed(torch_loss_trace, args.iters)
    res["loss_composed_non_trace_ms"] = res["loss_composed_ms"] - res["loss_composed_trace_ms"]

    # ---- the precompute at Ns samples ---------------------------------------------------------------------
    def hip_pre():
        return visibility.precompute_visibility(rt, means, cov, opac, normals, Ns)

    def torch_pre():
        chunk = max(1, P // 4)  # the arrays of a quarter of the rays at a time, as the reference chunks
        out = []
        for off in range(0, P, chunk):
            dirs = torch_fib_dirs(normals[off:off + chunk], Ns)
            o = means[off:off + chunk, None].expand_as(dirs)
            out.append(rt.trace_visibility(o, dirs, means, cov, opac, normals)["visibility"])
        return torch.cat(out, 0)

    res["precompute_ms"] = timed(hip_pre, max(3, args.iters // 3))
    res["precompute_composed_ms"] = timed(torch_pre, max(3, args.iters // 3))
    res["precompute_peak_bytes"] = peak_bytes(hip_pre)
    res["precompute_composed_peak_bytes"] = peak_bytes(torch_pre)
    res["precompute_output_bytes"] = 4 * P * Ns
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
