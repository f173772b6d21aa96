"""Parameter activations on the MI355X (`GaussianTrainState.activate`, csrc/activation.hip) against the same
work composed the way a caller had to before: the getters as torch operations on per-group leaf views of the
flat buffer (exp, two F.normalize, four sigmoid, three torch.cat, F.normalize(campos - xyz), and for symm_inv
the rotation matrix, a bmm and the six upper entries), torch autograd, then the copy of each `.grad` into
`st.grad_view(name)`.

P Gaussians (by default 1M, where every group block is 16-byte aligned, and 1M + 1, where every small-group
block behind xyz takes the dword path), 14 groups, camera centre given; per P, with and without symm_inv:
  forward            the outputs under no_grad
  forward+backward   the outputs, then autograd with one fixed upstream gradient per output (made once, so no
                     loss kernels are timed), ending with every group's gradient in st.grad
Each is timed both ways in this process with CUDA events (median of --iters after two warm-up calls). Launches
are counted from one profiled call outside the timed window (null when the profiler is not available). The
fused form's algorithmic bytes (what the two directions must read and write, from the shapes) over its time
give the achieved rate and its share of the 6.3 TB/s copy rate.

Usage: python tools/bench_activation.py [--P 1000000 1000001] [--iters 20] [--out profiles/activation/activation_bench.json]
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

COPY_RATE = 6.3e12  # B/s, the HBM copy rate the element-wise kernels are held against
SMALL = 19          # floats per Gaussian of the groups up to 4 wide (xyz, normal, rotation, scaling, opacity,
                    # base_color, roughness, metallic)
PARAMS = 131        # floats per Gaussian of all 14 groups


def algorithmic_bytes(P, symm):
    """Bytes the fused form has to move: forward reads every parameter and writes every output (131 floats:
    the activations of 16 + viewdirs 3 + the SH rows 112; xyz is not copied) + symm_inv 6; backward reads the
    upstreams (131 + g_xyz 3) and the raw small groups, and writes 131 gradients."""
    fwd = 4 * P * (PARAMS + PARAMS + (6 if symm else 0))
    bwd = 4 * P * (PARAMS + 3 + SMALL + PARAMS)
    return fwd, bwd


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


def launches(fn):
    """Kernels and device copies of one call, from the profiler; None when it yields nothing."""
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def make_state(P, seed=0):
    from relightable3dgaussian_amd.trainer import BASE_GROUPS, PBR_GROUPS, GaussianTrainState

    g = torch.Generator(device="cuda").manual_seed(seed)
    t = {n: torch.randn((P, *s), device="cuda", generator=g) * (0.3 if len(s) == 2 else 1.0)
         for n, s in BASE_GROUPS + PBR_GROUPS}
    t["scaling"] = t["scaling"] - 4.0
    return GaussianTrainState.from_tensors(t, use_pbr=True)


def symm_inverse(rotation, scaling):
    """strip_symmetric(L L^T), L = R(q / |q|) diag(1 / s), as tensor operations."""
    q = rotation / rotation.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    L = R @ torch.diag_embed(1 / scaling)
    S = L @ L.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)


def composed(p, campos, symm):
    """The getters on per-group tensors p (name -> tensor)."""
    Fn = torch.nn.functional
    out = {"xyz": p["xyz"], "scaling": torch.exp(p["scaling"]), "rotation": Fn.normalize(p["rotation"]),
           "normal": Fn.normalize(p["normal"], dim=-1, eps=1e-3), "opacity": torch.sigmoid(p["opacity"]),
           "shs": torch.cat((p["f_dc"], p["f_rest"]), dim=1), "base_color": torch.sigmoid(p["base_color"]),
           "roughness": torch.sigmoid(p["roughness"]), "metallic": torch.sigmoid(p["metallic"]),
           "incidents": torch.cat((p["incidents_dc"], p["incidents_rest"]), dim=1),
           "visibility": torch.cat((p["visibility_dc"], p["visibility_rest"]), dim=1),
           "viewdirs": Fn.normalize(campos - p["xyz"], dim=-1)}
    if symm:
        with torch.no_grad():
            out["symm_inv"] = symm_inverse(out["rotation"], out["scaling"])
    return out


def measure(P, iters):
    st = make_state(P)
    names = [n for n, _ in st.groups]
    campos = torch.tensor([0.3, -4.0, 1.1], device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    with torch.no_grad():
        shapes = {k: v.shape for k, v in st.activate(campos=campos).items()}
    ups = {k: torch.randn(s, device="cuda", generator=g) for k, s in shapes.items()}

    def fused_fwd(symm):
        with torch.no_grad():
            return st.activate(campos=campos, inverse_covariance=symm)

    def fused_fwd_bwd(symm):
        out = st.activate(campos=campos, inverse_covariance=symm)
        torch.autograd.backward([out[k] for k in ups], [ups[k] for k in ups])

    def composed_fwd(symm):
        with torch.no_grad():
            return composed({n: st.view(n) for n in names}, campos, symm)

    def composed_fwd_bwd(symm):
        leaves = {n: st.view(n).detach().requires_grad_(True) for n in names}
        out = composed(leaves, campos, symm)
        torch.autograd.backward([out[k] for k in ups], [ups[k] for k in ups])
        for n in names:  # INTEGRATION.md's "copy each .grad into st.grad_view(name)"
            st.grad_view(n).copy_(leaves[n].grad)

    # the two forms compute the same thing (checked once, at the size that is timed)
    fused_fwd_bwd(True)
    ref_grad = st.grad.clone()
    composed_fwd_bwd(True)
    scale = float(ref_grad.abs().max())
    diff = float((st.grad - ref_grad).abs().max())
    assert diff <= 1e-3 * scale, (diff, scale)

    res = {"P": P, "groups": len(names), "iters": iters, "grad_max_abs_diff_vs_composed": diff,
           "grad_max_abs": scale}
    for symm in (False, True):
        tag = "_symm" if symm else ""
        fwd_b, bwd_b = algorithmic_bytes(P, symm)
        f = timed(lambda: fused_fwd(symm), iters)
        fb = timed(lambda: fused_fwd_bwd(symm), iters)
        c = timed(lambda: composed_fwd(symm), iters)
        cb = timed(lambda: composed_fwd_bwd(symm), iters)
        res.update({
            f"fused_forward{tag}_ms": f, f"fused_forward_backward{tag}_ms": fb,
            f"composed_forward{tag}_ms": c, f"composed_forward_backward{tag}_ms": cb,
            f"ratio_forward{tag}": c / f, f"ratio_forward_backward{tag}": cb / fb,
            f"fused_forward{tag}_bytes": fwd_b, f"fused_forward_backward{tag}_bytes": fwd_b + bwd_b,
            f"fused_forward{tag}_TBps": fwd_b / f / 1e9, f"fused_forward_backward{tag}_TBps": (fwd_b + bwd_b) / fb / 1e9,
            f"fused_forward{tag}_of_copy_rate": fwd_b / (f * 1e-3) / COPY_RATE,
            f"fused_forward_backward{tag}_of_copy_rate": (fwd_b + bwd_b) / (fb * 1e-3) / COPY_RATE,
            f"fused_forward{tag}_launches": launches(lambda: fused_fwd(symm)),
            f"fused_forward_backward{tag}_launches": launches(lambda: fused_fwd_bwd(symm)),
            f"composed_forward{tag}_launches": launches(lambda: composed_fwd(symm)),
            f"composed_forward_backward{tag}_launches": launches(lambda: composed_fwd_bwd(symm)),
        })
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, nargs="+", default=[1_000_000, 1_000_001],
                    help="Gaussians; the default times a multiple of 4 (every block 16-byte aligned) and an odd P "
                         "(every small-group block behind xyz on the dword path)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "activation", "activation_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_activation: needs the GPU (no CPU path, and a CPU time says nothing)")
    line = json.dumps({"copy_rate_Bps": COPY_RATE, "runs": [measure(P, args.iters) for P in args.P]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
