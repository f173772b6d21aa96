"""Timing of the relighting render equation (csrc/relight.hip) on the GPU.

P Gaussians (default 1M) at Ns = 24 and Ns = 384, 16 SH coefficients, in the modes baked + SH light,
traced + environment map (6 x 10, rotated) and traced + no light. In the same process it also times the
nearest existing path, render_equation_forward_complex followed by the four .mean(-2) reductions of its
per-sample outputs, at Ns = 24 (at Ns = 384 that path writes 20 GB of per-sample arrays per call).

Reports device time per call (HIP events on the current stream, median of K after a warm-up) and the
effective HBM rate against the operator's bytes per Gaussian: 44 of attributes + 192 of incident SH
+ 64 of visibility SH (baked) or 4 Ns of traced visibility, and 84 written.

Writes one JSON document to --out (default profiles/relight/relight_bench.json) and prints it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relight", "relight_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import relightable3dgaussian_amd as r
    from relightable3dgaussian_amd import relight, synthetic

    _C = r._C
    P = args.P
    inp = synthetic.brdf_inputs(P, seed=0)
    t = {k: torch.as_tensor(v, device="cuda") for k, v in inp.items()}
    ins = [t[k] for k in ["base", "rough", "metal", "normals", "viewdirs", "incidents", "env", "visibility"]]
    g = torch.Generator(device="cuda").manual_seed(0)
    env_map = relight.EnvLight(torch.exp(1.5 * torch.randn(6, 10, 3, device="cuda", generator=g)))
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(0)))
    env_map.transform = q.cuda().contiguous()

    class ShLight:
        get_env_shs = t["env"]

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    def entry(ms, nbytes):
        med, lo, hi = ms
        return {"ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes_per_gaussian": nbytes,
                "GB/s": round(nbytes * P / med / 1e6, 1), "Mgauss/s": round(P / med / 1e3, 1)}

    def complex_and_means(Ns):
        o = _C.render_equation_forward_complex(*ins, Ns)
        return o[0], o[2].mean(-2), o[3].mean(-2), o[4].mean(-2), o[5].mean(-2)

    res = {}
    for Ns in (24, 384):
        traced = torch.rand(P, Ns, device="cuda", generator=g)
        args_ = (t["base"], t["rough"], t["metal"], t["normals"], t["viewdirs"], t["incidents"])
        modes = {
            "baked+sh": (lambda: relight.render_equation_relight(*args_, ShLight, t["visibility"], Ns, True),
                         44 + 192 + 64 + 84),
            "traced+map": (lambda: relight.render_equation_relight(*args_, env_map, t["visibility"], Ns, False, traced),
                           44 + 192 + 4 * Ns + 84),
            "traced+none": (lambda: relight.render_equation_relight(*args_, None, t["visibility"], Ns, False, traced),
                            44 + 192 + 4 * Ns + 84),
        }
        row = {name: entry(timed(fn), nbytes) for name, (fn, nbytes) in modes.items()}
        if Ns == 24:
            row["forward_complex"] = entry(timed(lambda: _C.render_equation_forward_complex(*ins, Ns)), 204 + 1312)
            row["forward_complex+4 means"] = entry(timed(lambda: complex_and_means(Ns)), 204 + 1312)
        res[f"Ns{Ns}"] = row
        del traced
    doc = {"P": P, "S": 16, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "results": res, "hbm_peak_GBs": 8000}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
