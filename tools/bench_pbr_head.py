"""The PBR image head and the light regulariser on the MI355X (`relightable3dgaussian_amd.pbr`, csrc/pbr_head.hip)
against the same work composed from torch tensor operations the way the reference does it
(gaussian_renderer/neilf.py:169-175 with scene/gamma_trans.py:45-51, and neilf.py:279-281), in one process.

  head        800x800 and 1920x1080, "hwc" with pbr a view at float 2 H W of an [11 H W] feature buffer (the
              rasterizer's block), opacity [H,W,1], bg [3]; tone "none" and "gamma"; forward under no_grad, and
              forward + backward with one fixed upstream (so no loss kernel is timed), gradients to pbr, opacity
              and (with gamma) gamma
  light_loss  P = 1M rows; forward under no_grad, and forward + backward
Each is timed both ways with CUDA events: the median of --iters single calls after two warm-up calls, one run.
A single call includes launch latency and torch's autograd bookkeeping on the host, for both forms; at these
sizes that is most of a fused call, so the distance to the bound is given for what it is: (algorithmic bytes /
the measured 6.29 TB/s copy rate of DESIGN.md section 2h) over the single-call time. Launches (kernels and device
copies) and, where the profiler reports it, the summed device time of the kernels come from one profiled call
outside the timed window (null when the profiler yields nothing).

Usage: python tools/bench_pbr_head.py [--iters 20] [--out profiles/pbr_head/pbr_head_bench.json]
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

COPY_RATE = 6.29e12            # B/s, DESIGN.md section 2h
HEAD_FWD_B, HEAD_BWD_B = 28, 44  # per pixel: read 3 + 1 floats, write 3; read 3 + 3 + 1, write 3 + 1
LIGHT_FWD_B, LIGHT_BWD_B = 12, 24  # per row: read 3 floats; read 3, write 3


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


def profiled(fn):
    """(launches, summed device time in ms) of one call, from the profiler; (None, None) when it yields nothing."""
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        evs = [ev for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA")]
        if not evs:
            return None, None
        us = sum(float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0) or 0.0) for ev in evs)
        return len(evs), (us / 1e3 if us > 0 else None)
    except Exception:
        return None, None


def row(name, fused, composed, iters, bound_bytes):
    f, c = timed(fused, iters), timed(composed, iters)
    fl, fk = profiled(fused)
    cl, ck = profiled(composed)
    bound_ms = bound_bytes / COPY_RATE * 1e3
    return {"what": name, "fused_ms": f, "composed_ms": c, "ratio": c / f, "fused_launches": fl, "composed_launches": cl,
            "fused_kernels_ms": fk, "composed_kernels_ms": ck, "algorithmic_bytes": bound_bytes, "bound_ms": bound_ms,
            "fused_call_over_bound": f / bound_ms, "fused_kernels_over_bound": fk / bound_ms if fk else None}


def head(H, W, tone, iters):
    from relightable3dgaussian_amd.pbr import pbr_image

    n = H * W
    g = torch.Generator(device="cuda").manual_seed(H)
    feat = torch.rand(11 * n, device="cuda", generator=g) * 1.4 - 0.15
    pbr = feat[2 * n:5 * n].view(H, W, 3)
    opacity = torch.rand(H, W, 1, device="cuda", generator=g)
    bg = torch.tensor([0.2, 0.5, 1.0], device="cuda")
    up = torch.randn(H, W, 3, device="cuda", generator=g)
    gamma = torch.full((1,), 0.45, device="cuda") if tone == "gamma" else None

    def composed_image(p, o, gm):
        x = p + (1 - o) * bg[None, None, :]
        return x if gm is None else x.clamp(1e-9, 1) ** gm

    def leaves():
        return (pbr.detach().requires_grad_(True), opacity.detach().requires_grad_(True),
                None if gamma is None else gamma.detach().requires_grad_(True))

    def fused_fwd():
        with torch.no_grad():
            return pbr_image(pbr, opacity, bg, gamma, tone)

    def composed_fwd():
        with torch.no_grad():
            return composed_image(pbr, opacity, gamma)

    def fused_fb():
        p, o, gm = leaves()
        pbr_image(p, o, bg, gm, tone).backward(up)
        return p.grad, o.grad, None if gm is None else gm.grad

    def composed_fb():
        p, o, gm = leaves()
        composed_image(p, o, gm).backward(up)
        return p.grad, o.grad, None if gm is None else gm.grad

    # the two forms compute the same thing (checked once, at the size that is timed)
    assert (fused_fwd() - composed_fwd()).abs().max() <= 1e-6
    for a, b in zip(fused_fb(), composed_fb()):
        if a is not None:
            # dL/dgamma: torch's float32 sum of H W 3 terms of both signs carries its own summation error
            tol = 1e-3 if a.numel() == 1 else 1e-5
            assert float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-30), (tone, H, W)
    tag = f"head {W}x{H} {tone}"
    return [row(tag + " forward", fused_fwd, composed_fwd, iters, HEAD_FWD_B * n),
            row(tag + " forward+backward", fused_fb, composed_fb, iters, (HEAD_FWD_B + HEAD_BWD_B) * n)]


def light(P, iters):
    import torch.nn.functional as Fn

    from relightable3dgaussian_amd.pbr import light_loss

    d = torch.rand(P, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(P)) * 2

    def composed_loss(t):
        return Fn.l1_loss(t, t.mean(-1, keepdim=True).expand_as(t))

    def fused_fwd():
        with torch.no_grad():
            return light_loss(d)

    def composed_fwd():
        with torch.no_grad():
            return composed_loss(d)

    def fused_fb():
        t = d.detach().requires_grad_(True)
        light_loss(t).backward()
        return t.grad

    def composed_fb():
        t = d.detach().requires_grad_(True)
        composed_loss(t).backward()
        return t.grad

    assert abs(float(fused_fwd()) - float(composed_fwd())) <= 1e-5 * float(composed_fwd())
    # signs may differ where an element sits on its row mean to float32 rounding; the mean difference says the rest
    assert float((fused_fb() - composed_fb()).abs().mean()) <= 1e-3 / (3 * P)
    tag = f"light_loss P={P}"
    return [row(tag + " forward", fused_fwd, composed_fwd, iters, LIGHT_FWD_B * P),
            row(tag + " forward+backward", fused_fb, composed_fb, iters, (LIGHT_FWD_B + LIGHT_BWD_B) * P)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pbr_head", "pbr_head_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pbr_head: needs the GPU (no CPU path, and a CPU time says nothing)")
    rows = []
    for H, W in ((800, 800), (1080, 1920)):
        for tone in ("none", "gamma"):
            rows += head(H, W, tone, args.iters)
    rows += light(1_000_000, args.iters)
    line = json.dumps({"copy_rate_Bps": COPY_RATE, "iters": args.iters, "warmup": 2,
                       "timing": "CUDA events around one call (launch latency and host bookkeeping included), median",
                       "rows": rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
