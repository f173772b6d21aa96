"""A numpy model of csrc/activation.hip's arithmetic on the CPU, against tests/activation_ref64.py: why the
backward departs from the float32 reference's operation sequence in two places.

Every operation is rounded to float32 as the kernel rounds it (numpy's float32 exp stands in for expf). The
backward is modelled twice:
  f32    the normalise gradient's projection (g - y (y.g)) / r and the sigmoid slope s (1 - s) in float32
  built  the projection in double from the float32 inputs, rounded once; the slope as t / (1 + t)^2
over tests/activation_ref64.draw_case at several P and seeds (the golden draw, P = 257 seed 41, among them).
Printed per quantity: the worst row_err over the draws divided by its bar (BARS = 4 x the golden draw's floor);
above 1 the form would fail the GPU tests on some draw whatever the hardware does.

Usage: python tools/analysis/activation_f32_model.py [--out profiles/activation/f32_model.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import activation_ref64 as a64  # noqa: E402

F = np.float32
DRAWS = [(257, 41), (1025, 1125), (65, 165), (255, 355), (63, 3), (257, 7), (257, 17)]


def norm(x):
    ss = x[:, 0] * x[:, 0]
    for c in range(1, x.shape[1]):
        ss = ss + x[:, c] * x[:, c]
    return np.sqrt(ss)[:, None]


def normalize(x, eps):
    return x / np.maximum(norm(x), F(eps))


def normalize_bwd(x, g, eps, double, xd=None):
    r = norm(x)
    with np.errstate(all="ignore"):
        if double:
            xd = x.astype(np.float64) if xd is None else xd
            inv = 1.0 / np.sqrt((xd * xd).sum(1, keepdims=True))
            y = xd * inv
            p = (g - y * (y * g).sum(1, keepdims=True)) * inv
        else:
            y = x / r
            dot = y[:, 0] * g[:, 0]
            for c in range(1, x.shape[1]):
                dot = dot + y[:, c] * g[:, c]
            p = (g - y * dot[:, None]) / r
    return np.where(r >= F(eps), p, (g / F(eps)).astype(p.dtype))


def sigmoid(x):
    with np.errstate(all="ignore"):
        return F(1) / (F(1) + np.exp(-x))


def symm_inverse(qh, s):
    q = qh / norm(qh)
    r, x, y, z = q.T
    one, two = F(1), F(2)
    R = [[one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)],
         [two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)],
         [two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]]
    inv = F(1) / s
    L = [[R[i][k] * inv[:, k] for k in range(3)] for i in range(3)]
    return np.stack([(L[i][0] * L[j][0] + L[i][1] * L[j][1]) + L[i][2] * L[j][2]
                     for i in range(3) for j in range(i, 3)], 1)


def model(c, ups, built):
    cam = a64.CAMPOS
    out = {"scaling": np.exp(c["scaling"]), "rotation": normalize(c["rotation_fwd"], 1e-12),
           "normal": normalize(c["normal"], 1e-3), "viewdirs": normalize(cam[None] - c["xyz"], 1e-12)}
    out.update({k: sigmoid(c[k]) for k in a64.SIGMOIDS})
    out["symm_inv"] = symm_inverse(out["rotation"], out["scaling"])
    v = cam[None] - c["xyz"]
    vd = cam[None].astype(np.float64) - c["xyz"]
    g = {"xyz": (ups["xyz"] - normalize_bwd(v, ups["viewdirs"], 1e-12, built, vd)).astype(F),
         "normal": normalize_bwd(c["normal"], ups["normal"], 1e-3, built).astype(F),
         "rotation": normalize_bwd(c["rotation"], ups["rotation"], 1e-12, built).astype(F),
         "scaling": ups["scaling"] * np.exp(c["scaling"])}
    for k in a64.SIGMOIDS:
        if built:
            t = np.exp(-np.abs(c[k]))
            d = F(1) + t
            g[k] = ups[k] * (t / (d * d))
        else:
            s = sigmoid(c[k])
            g[k] = ups[k] * s * (F(1) - s)
    return out, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    worst = {}
    for P, seed in DRAWS:
        c = a64.draw_case(P, seed, 14)
        ups = a64.draw_upstreams(P, seed + 1, 14, True)
        ref = a64.forward(c, a64.CAMPOS, True, "rotation_fwd")
        gref = a64.backward(c, ups, a64.CAMPOS)
        for name, built in (("f32", False), ("built", True)):
            out, g = model(c, ups, built)
            for k, val in list(out.items()) + [("grad_" + k, val) for k, val in g.items()]:
                e = a64.row_err(val, gref[k[5:]] if k.startswith("grad_") else ref[k]) / a64.BARS[k]
                key = (k, name)
                if e > worst.get(key, (0.0, None))[0] or key not in worst:
                    worst[key] = (e, (P, seed))
    lines = [f"{'quantity':18s} {'f32 err/bar':>12s} {'at (P, seed)':>14s} {'built err/bar':>14s} {'at (P, seed)':>14s}"]
    for k in dict.fromkeys(k for k, _ in worst):
        a, b = worst[(k, "f32")], worst[(k, "built")]
        lines.append(f"{k:18s} {a[0]:12.3f} {str(a[1]):>14s} {b[0]:14.3f} {str(b[1]):>14s}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
