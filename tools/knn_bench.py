"""distCUDA2 timing on one MI355X (csrc/knn.hip; the reference's simple_knn._C.distCUDA2).

Workloads: P points (default 100k -- the reference's random initialisation for Blender scenes,
scene/dataset_readers.py -- and 1M), "uniform" in the unit cube and "clustered" (half uniform, half in
eight Gaussian blobs of sigma 0.01). Each is warmed up and timed with HIP events around single calls
(median, min and max over --iters).

Beside it, on the same GPU, the substitute a user without the operator has: a chunked
torch.cdist + topk(4, largest=False) (the nearest is the point itself), mean of the three squared
distances. It is O(P^2); at most --torch-rows query rows are timed against all P points and the full
time is that scaled by P / rows (reported as such). Its values are compared loosely (it is not
bit-exact: cdist goes through a matrix product).

Usage: python tools/knn_bench.py [--P 100000 1000000] [--iters 20] [--warmup 3] [--torch-rows 32768]
                                 [--no-torch] [--out file.json]
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


def make_points(P, kind, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        x = rng.random((P, 3))
    else:
        centres = rng.random((8, 3))
        blobs = centres[rng.integers(0, 8, P // 2)] + rng.normal(0.0, 0.01, (P // 2, 3))
        x = np.concatenate([rng.random((P - P // 2, 3)), blobs])
        x = x[rng.permutation(P)]
    return torch.from_numpy(x.astype(np.float32)).cuda()


def torch_substitute(x, rows, chunk_bytes=1 << 30):
    """Mean squared distance to the 3 nearest others of the first `rows` points, by cdist + topk."""
    P = x.shape[0]
    chunk = max(1, min(rows, chunk_bytes // (4 * P)))
    out = torch.empty(rows, device=x.device)
    for s in range(0, rows, chunk):
        e = min(s + chunk, rows)
        d = torch.cdist(x[s:e], x)
        near = torch.topk(d, min(4, P), dim=1, largest=False).values[:, 1:]
        out[s:e] = (near * near).sum(1) / 3.0
    return out


def time_calls(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-rows", type=int, default=32768)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_bench: needs a GPU (nothing is timed on the host)")
    import relightable3dgaussian_amd as r

    results = []
    for P in a.P:
        for kind in ("uniform", "clustered"):
            x = make_points(P, kind)
            res = {"P": P, "points": kind, "distCUDA2": time_calls(lambda: r._C.distCUDA2(x), a.warmup, a.iters)}
            if not a.no_torch:
                rows = min(P, a.torch_rows)
                t = time_calls(lambda: torch_substitute(x, rows), 1, 3)
                t["rows_timed"] = rows
                t["full_ms_scaled"] = t["median_ms"] * P / rows
                ours, sub = r._C.distCUDA2(x)[:rows], torch_substitute(x, rows)
                t["max_rel_diff"] = float(((ours - sub).abs() / ours.clamp_min(1e-12)).max())
                res["torch_cdist_topk"] = t
                res["speedup"] = t["full_ms_scaled"] / res["distCUDA2"]["median_ms"]
            print(json.dumps(res), flush=True)
            results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
