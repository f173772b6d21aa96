"""Generate tests/golden/activation.npz from the REFERENCE's own activation code (CPU, float32).

Runs torch.exp, F.normalize, torch.sigmoid, torch.cat and the reference checkout's
utils.general_utils.build_scaling_rotation / strip_symmetric, composed as scene/gaussian_model.py:23-44,
331-413 (the getters, get_inverse_covariance) and gaussian_renderer/neilf.py:102 (the view directions) compose
them, on the seeded draw of tests/activation_ref64.py; the parameter gradients come from torch.autograd.grad
with seeded upstream gradients. Stores inputs and outputs only (data, no reference source). The reference is
imported as tests/golden/make_golden.py does it.

Cases: "a" P = 257 with 14 groups and a camera centre; "b" P = 65 with 7 groups and none. Per case:
  <group>            the raw parameters          rotation_fwd   rotation with one row scaled by 1e-6
  out_<output>       the forward outputs, computed with rotation_fwd (symm_inv included)
  up_<output>        the upstream gradients      grad_<group>   the gradients, computed with rotation

The archive is written with fixed zip timestamps and one thread, so it regenerates byte for byte.

Usage:  python tests/golden/make_golden_activation.py [--reference /root/reference]
        python tests/golden/make_golden_activation.py --floors   (the FLOORS of tests/activation_ref64.py)
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

OUT = os.path.join(HERE, "activation.npz")
CASES = {"a": dict(P=257, groups=14, seed=41, campos=True), "b": dict(P=65, groups=7, seed=42, campos=False)}


def getters(gu, t: dict, campos, rotation):
    """The reference's getters on leaf tensors t (name -> tensor)."""
    Fn = torch.nn.functional
    out = {"xyz": t["xyz"], "scaling": torch.exp(t["scaling"]), "rotation": Fn.normalize(rotation),
           "normal": Fn.normalize(t["normal"], dim=-1, eps=1e-3), "opacity": torch.sigmoid(t["opacity"]),
           "shs": torch.cat((t["f_dc"], t["f_rest"]), dim=1)}
    if "base_color" in t:
        out.update({n: torch.sigmoid(t[n]) for n in ("base_color", "roughness", "metallic")})
        out["incidents"] = torch.cat((t["incidents_dc"], t["incidents_rest"]), dim=1)
        out["visibility"] = torch.cat((t["visibility_dc"], t["visibility_rest"]), dim=1)
    if campos is not None:
        out["viewdirs"] = Fn.normalize(campos - t["xyz"], dim=-1)
    # get_inverse_covariance(scaling_modifier=1): covariance_activation(1 / scaling, 1 / 1, rotation)
    L = gu.build_scaling_rotation((1 / 1) * (1 / out["scaling"]), out["rotation"])
    out["symm_inv"] = gu.strip_symmetric(L @ L.transpose(1, 2))
    return out


def generate(ref: str) -> dict:
    from tests import activation_ref64 as a64

    torch.set_num_threads(1)
    res = {}
    with CpuMode():
        _, _, _, gu = load_reference(ref)
        for name, kw in CASES.items():
            c = a64.draw_case(kw["P"], kw["seed"], kw["groups"])
            ups = a64.draw_upstreams(kw["P"], kw["seed"] + 1000, kw["groups"], kw["campos"])
            campos = torch.from_numpy(a64.CAMPOS) if kw["campos"] else None
            for k, v in c.items():
                res[f"{name}_{k}"] = v
            for k, v in ups.items():
                res[f"{name}_up_{k}"] = v
            group_names = [g for g, _ in a64.groups_of(kw["groups"])]
            with torch.no_grad():
                t = {g: torch.from_numpy(c[g]) for g in group_names}
                for k, v in getters(gu, t, campos, torch.from_numpy(c["rotation_fwd"])).items():
                    if k != "xyz":
                        res[f"{name}_out_{k}"] = v.numpy().copy()
            t = {g: torch.from_numpy(c[g]).requires_grad_(True) for g in group_names}
            out = getters(gu, t, campos, t["rotation"])
            loss = sum((out[k] * torch.from_numpy(u)).sum() for k, u in ups.items())
            grads = torch.autograd.grad(loss, [t[g] for g in group_names])
            for g, d in zip(group_names, grads):
                res[f"{name}_grad_{g}"] = d.numpy().copy()
    return res


def case_inputs(g, name: str):
    """(params, upstreams, campos) of golden case `name`."""
    from tests import activation_ref64 as a64

    kw = CASES[name]
    c = {k: g[f"{name}_{k}"] for k, _ in a64.groups_of(kw["groups"])}
    c["rotation_fwd"] = g[f"{name}_rotation_fwd"]
    pre = f"{name}_up_"
    ups = {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}
    return c, ups, (a64.CAMPOS if kw["campos"] else None)


def measure(g) -> dict:
    """row_err of every stored output and gradient against ref64, the worst over the cases."""
    from tests import activation_ref64 as a64

    worst = {}
    for name in CASES:
        c, ups, campos = case_inputs(g, name)
        ref = a64.forward(c, campos, inverse_covariance=True, rotation="rotation_fwd")
        gref = a64.backward(c, ups, campos)
        pairs = [(k, g[f"{name}_out_{k}"], v) for k, v in ref.items() if k != "xyz"]
        pairs += [(f"grad_{k}", g[f"{name}_grad_{k}"], v) for k, v in gref.items()]
        for k, got, want in pairs:
            e = a64.row_err(got, want)
            print(f"{name} {k:22s} {e:.3e}")
            worst[k] = max(worst.get(k, 0.0), e)
    return worst


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
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
