"""Generate tests/golden/visibility.npz from the REFERENCE's own visibility-SH fit code (CPU, float32).

Runs utils/sh_utils.py eval_sh of the reference checkout with torch.clamp, F.l1_loss, autograd and
torch.optim.Adam(lr=1e-2), as scene/gaussian_model.py:428-462 (finetune_visibility) and
gaussian_renderer/neilf.py:331-346 (lambda_visibility) compose them, on seeded inputs, and stores inputs and
outputs only (data, no reference source). The reference is imported as tests/golden/make_golden.py does it.

Cases, P = 257, K = 16 ("k16") and K = 25 ("k25"): unnormalised randn directions flipped by the normals,
traced visibility as the tracer yields it (~30 % exact 0, ~20 % exact 1, the rest uniform in (0.9, 1)),
coefficients N(0, 0.3) so that raw + 0.5 lands below 0, inside [0, 1] and above 1. Recorded per case:
  loss, grad_dc, grad_rest                    the first evaluation
  dc_step{1,2,3}, rest_step{1,2,3}, loss_step the parameters after each of 3 Adam steps and the loss of each
                                              step, re-evaluating the current coefficients every step (as the
                                              training loss does), with fresh directions / traced per step
  idx, idx_dirs, idx_traced, idx_loss, idx_grad_dc, idx_grad_rest
                                              the training term's indexed form: 100 of the 257 rows

The archive is written with fixed zip timestamps and one thread, so it regenerates byte for byte.

Usage:  python tests/golden/make_golden_visibility.py [--reference /root/reference]
        python tests/golden/make_golden_visibility.py --floors   (the noise floors of tests/visibility_ref64.py)
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
from make_golden_relight import write_npz  # noqa: E402

OUT = os.path.join(HERE, "visibility.npz")
P = 257
CASES = {"k16": (16, 31), "k25": (25, 32)}  # name -> (K, seed)
STEPS = 3
N_INDEX = 100


def flipped(d, n):
    d = d.clone()
    mask = (d * n).sum(-1) < 0  # the call sites' flip (gaussian_model.py:447-448)
    d[mask] *= -1
    return d


def sample_loss(sh_mod, dc, rest, d, traced):
    """gaussian_model.py:442-459 with the view rebuilt from the current parameters."""
    view = torch.cat([dc, rest], dim=1).transpose(1, 2)  # get_visibility.transpose(1, 2): [P, 1, K]
    deg = int(round(np.sqrt(view.shape[-1]) - 1))
    vis = torch.clamp(sh_mod.eval_sh(deg, view, d) + 0.5, 0.0, 1.0)
    return torch.nn.functional.l1_loss(traced, vis)


def generate(ref: str) -> dict:
    from tests import visibility_ref64 as v64

    torch.set_num_threads(1)
    out = {}
    with CpuMode():
        _, sh_mod, _, _ = load_reference(ref)
        for name, (K, seed) in CASES.items():
            steps = [v64.draw_case(P, K, seed + 100 * s) for s in range(STEPS)]
            c0 = steps[0]
            normals = torch.from_numpy(c0["normals"])
            dc = torch.from_numpy(c0["dc"].copy()).requires_grad_(True)  # copies: Adam updates in place
            rest = torch.from_numpy(c0["rest"].copy()).requires_grad_(True)
            out[f"{name}_dc"], out[f"{name}_rest"], out[f"{name}_normals"] = c0["dc"], c0["rest"], c0["normals"]
            # the indexed training term on the initial coefficients
            rng = np.random.default_rng(seed + 7)
            idx = rng.permutation(P)[:N_INDEX].astype(np.int64)
            ci = v64.draw_case(P, K, seed + 50, R=N_INDEX)
            ti = torch.from_numpy(idx)
            d = flipped(torch.from_numpy(ci["dirs"]), normals[ti])
            view = torch.cat([dc, rest], dim=1).transpose(1, 2)[ti]
            vis = torch.clamp(sh_mod.eval_sh(int(round(np.sqrt(K) - 1)), view, d) + 0.5, 0.0, 1.0)
            loss = torch.nn.functional.l1_loss(torch.from_numpy(ci["traced"])[:, None], vis)
            g = torch.autograd.grad(loss, [dc, rest])
            out.update({f"{name}_idx": idx, f"{name}_idx_dirs": ci["dirs"], f"{name}_idx_traced": ci["traced"],
                        f"{name}_idx_loss": loss.detach().numpy(), f"{name}_idx_grad_dc": g[0].numpy(),
                        f"{name}_idx_grad_rest": g[1].numpy()})
            # three fit steps
            opt = torch.optim.Adam([{"params": [dc], "lr": 1e-2}, {"params": [rest], "lr": 1e-2}])
            losses = []
            for s, c in enumerate(steps):
                out[f"{name}_dirs_step{s + 1}"], out[f"{name}_traced_step{s + 1}"] = c["dirs"], c["traced"]
                d = flipped(torch.from_numpy(c["dirs"]), normals)
                loss = sample_loss(sh_mod, dc, rest, d, torch.from_numpy(c["traced"])[:, None])
                loss.backward()
                if s == 0:
                    out[f"{name}_loss"] = loss.detach().numpy()
                    out[f"{name}_grad_dc"], out[f"{name}_grad_rest"] = dc.grad.numpy().copy(), rest.grad.numpy().copy()
                losses.append(float(loss))
                opt.step()
                opt.zero_grad()
                out[f"{name}_dc_step{s + 1}"] = dc.detach().numpy().copy()
                out[f"{name}_rest_step{s + 1}"] = rest.detach().numpy().copy()
            out[f"{name}_loss_step"] = np.asarray(losses, np.float32)
    return out


def golden_fit(g, name):
    """ref64's three fit steps on golden case `name` -> (Fit after the steps, [losses], first evaluation)."""
    from tests import visibility_ref64 as v64

    fit = v64.Fit(g[f"{name}_dc"], g[f"{name}_rest"], g[f"{name}_normals"])
    losses, first = [], None
    for s in range(STEPS):
        losses.append(fit.step(g[f"{name}_dirs_step{s + 1}"], g[f"{name}_traced_step{s + 1}"]))
        if s == 0:
            first = fit.last
    return fit, losses, first


def golden_index(g, name):
    from tests import visibility_ref64 as v64

    return v64.evaluate(g[f"{name}_dc"], g[f"{name}_rest"], g[f"{name}_idx_dirs"], g[f"{name}_idx_traced"],
                        g[f"{name}_normals"], g[f"{name}_idx"])


def decided_rows(e, P):
    """Gaussians none of whose rays is undecided in evaluation e."""
    bad = np.zeros(P, bool)
    bad[e["rows"][e["undecided"]]] = True
    return ~bad


def measure(g) -> dict:
    """max|golden - ref64| / max|ref64| of the loss, the gradient (decided rays) and the parameters after the
    three steps (decided Gaussians), over the golden cases."""
    from tests import visibility_ref64 as v64

    worst = {"loss": 0.0, "grad": 0.0, "params": 0.0}
    for name in CASES:
        fit, losses, first = golden_fit(g, name)
        ei = golden_index(g, name)
        e = {"loss": max(v64.rel_err(g[f"{name}_loss_step"], np.asarray(losses)),
                         v64.rel_err(g[f"{name}_idx_loss"], np.asarray(ei["loss"])))}
        ok0, oki = decided_rows(first, P), decided_rows(ei, P)
        cat = lambda a, b, ok: np.concatenate([a.reshape(P, -1), b.reshape(P, -1)], 1)[ok]  # noqa: E731
        e["grad"] = max(v64.rel_err(cat(g[f"{name}_grad_dc"], g[f"{name}_grad_rest"], ok0),
                                    cat(first["grad_dc"], first["grad_rest"], ok0)),
                        v64.rel_err(cat(g[f"{name}_idx_grad_dc"], g[f"{name}_idx_grad_rest"], oki),
                                    cat(ei["grad_dc"], ei["grad_rest"], oki)))
        ok = ~fit.undecided
        e["params"] = v64.rel_err(cat(g[f"{name}_dc_step3"], g[f"{name}_rest_step3"], ok), cat(fit.dc, fit.rest, ok))
        for k, val in e.items():
            print(f"{name} {k:8s} {val:.3e}")
            worst[k] = max(worst[k], val)
    return worst


def fib_floor() -> float:
    from tests import visibility_ref64 as v64

    f = np.load(os.path.join(HERE, "fib.npz"))
    return v64.rel_err(f["dirs"], v64.fibonacci_dirs(f["normals"], f["dirs"].shape[1]))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--floors", action="store_true", help="print golden-vs-ref64 distances of the stored file")
    args = ap.parse_args()
    if args.floors:
        for k, v in measure(np.load(OUT)).items():
            print(f"floor {k:8s} {v:.3e}")
        print(f"floor fib      {fib_floor():.3e}")
        return
    write_npz(OUT, generate(args.reference))
    print("written", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
