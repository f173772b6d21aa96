"""Float64 restatement of the render equation (csrc/brdf.hip, reference render_equation.cu), in torch
with autograd, vectorised over (Gaussian, sample).

Test infrastructure only (not collected: no test_ prefix). Written from the formulas, not from the
oracle's loops: Fibonacci directions on the hemisphere (z_r = 1 - 2 r / (2 Ns - 1), azimuth
r pi (3 - sqrt 5), optionally + 2 pi u) turned to the normal by R = I + K + K^2 / (1 + n_z) with K the
cross-product matrix of (-n_y, n_x, 0); incident + visibility-weighted environment light from degree-3
SH, each light cut to its own coefficient count; Lambert + spherical-Gaussian GGX. The reference's
constants are kept: pi = 3.14159, and 1e-7 floors on r^2, 1 + n_z, |o|^2, |h| and the two GGX
denominators.

Gradients are autograd's, with the directions held constant (the backward kernel receives them as an
input), except where the reference's backward is not the derivative of its forward:

  * the three light clamps are straight-through (ReLU of the incident light, ReLU of the environment
    light, visibility clamped to [0, 1]): x + (clamp(x) - x).detach(). The reference tests the clamped
    value after the clamp, so the gradient is never zeroed (render_equation.cu:440-449);
  * incident_cap: the incident-SH gradient of coefficient i >= min(S_direct, S_incident) is zero (the
    reference's update loop is bounded by S_direct, :450; brdf.hip n_inc_upd);
  * the gradients of the normals and view directions are NOT restated: the reference overwrites
    dL_dn_d_i before its use (:372 / :403) and has no projection term for the half vector's
    normalisation, so they are no gradients of anything. They stay held to the oracle only.

The keyword switches `straight_through`, `incident_cap`, `drop_sample`, `pi` and `half_floor` exist for
the mutation tests: each replaces one convention by a plausible wrong one, which must fail the bar.

Not restated as a departure: the r^2 floor. Autograd zeroes d r^2 / d roughness under the floor, the
reference does not; the two differ only where the lobe exp(2 (h.n - 1) / 1e-7) is non-zero, i.e. h.n
within 1e-6 of 1, which tests/_brdf_cases.py keeps away from the floored Gaussians.
"""
from __future__ import annotations

import math

import numpy as np
import torch

PI = 3.14159  # the reference's literal
EPS = 1e-7

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)

FORWARD_KEYS = ["pbr", "incident_dirs", "incident_lights", "local_incident_lights", "global_incident_lights",
                "incident_visibility", "diffuse_light", "local_diffuse_light", "accum", "rgb_d", "rgb_s"]
GRAD_KEYS = ["base", "rough", "metal", "incidents", "env", "visibility"]  # normals / viewdirs: see above


def _t(a, dtype):
    return torch.tensor(np.asarray(a, np.float64), dtype=dtype)


def sh_basis(d):
    """The 16 real SH basis values of degree <= 3 along d [..., 3] -> [..., 16]."""
    x, y, z = d.unbind(-1)
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return torch.stack([
        torch.full_like(x, C0), -C1 * y, C1 * z, -C1 * x,
        C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
        C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy),
        C3[3] * z * (2 * zz - 3 * xx - 3 * yy), C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy),
        C3[6] * x * (xx - 3 * yy)], -1)


def fibonacci_dirs(normals, Ns, rand=None, pi=PI, dtype=torch.float64):
    """Unit sample directions [P, Ns, 3] around normals [P, 3]; rand [P, Ns] in [0, 1) rotates each
    sample's azimuth by 2 pi rand (the training forward)."""
    n = normals if torch.is_tensor(normals) else _t(normals, dtype)
    P = n.shape[0]
    ray = torch.arange(Ns, dtype=dtype)
    z = 1 - 2 * ray / (2 * Ns - 1)
    rad = torch.sqrt(1 - z * z)
    theta = (pi * (3 - math.sqrt(5.0)) * ray).expand(P, Ns)
    if rand is not None:
        theta = theta + _t(rand, dtype).reshape(P, Ns) * 2 * pi
    local = torch.stack([torch.sin(theta) * rad, torch.cos(theta) * rad, z.expand(P, Ns)], -1)
    K = torch.zeros(P, 3, 3, dtype=dtype)  # cross-product matrix of v = (-n_y, n_x, 0)
    K[:, 0, 2] = n[:, 0]
    K[:, 2, 0] = -n[:, 0]
    K[:, 1, 2] = n[:, 1]
    K[:, 2, 1] = -n[:, 1]
    c = torch.clamp(n[:, 2] + 1, min=EPS)
    R = torch.eye(3, dtype=dtype) + K + (K @ K) / c[:, None, None]
    o = torch.einsum("pij,pnj->pni", R, local)
    return o / torch.sqrt(torch.clamp((o * o).sum(-1, keepdim=True), min=EPS))


def _clamped(x, f, straight_through):
    y = f(x)
    return x + (y - x).detach() if straight_through else y


def render(inp, Ns, dirs=None, rand=None, upstream=None, straight_through=True, incident_cap=True,
           drop_sample=None, pi=PI, half_floor=EPS, dtype=torch.float64):
    """Every output of the training and the complex forward (numpy, FORWARD_KEYS; the training forward's
    pbr / incident_dirs / diffuse_light are the same quantities) and the clamps' arguments ("raw_*").
    dirs [P, Ns, 3]: evaluate on these directions instead of fibonacci_dirs(normals, Ns, rand).
    upstream = (dL_dpbr, dL_ddiffuse_light): also "grad_<k>" for k in GRAD_KEYS."""
    t = {k: _t(inp[k], dtype) for k in ["base", "rough", "metal", "normals", "viewdirs", "incidents", "env",
                                        "visibility"]}
    if upstream is not None:
        for k in GRAD_KEYS:
            t[k].requires_grad_(True)
    base, rough, metal, n, v = t["base"], t["rough"], t["metal"], t["normals"], t["viewdirs"]
    inc, env, vis_sh = t["incidents"], t["env"][0], t["visibility"][..., 0]
    P, Si, Sd, Sv = base.shape[0], inc.shape[1], env.shape[0], vis_sh.shape[1]
    d = _t(dirs, dtype).reshape(P, Ns, 3) if dirs is not None else fibonacci_dirs(n.detach(), Ns, rand, pi, dtype)
    Y = sh_basis(d)
    raw_local = torch.einsum("pnk,pkc->pnc", Y[..., :Si], inc)
    raw_global = 0.5 + torch.einsum("pnk,kc->pnc", Y[..., :Sd], env)
    raw_vis = 0.5 + torch.einsum("pnk,pk->pn", Y[..., :Sv], vis_sh)
    local = _clamped(raw_local, torch.relu, straight_through)
    glob = _clamped(raw_global, torch.relu, straight_through)
    vis = _clamped(raw_vis, lambda x: torch.clamp(x, 0.0, 1.0), straight_through)[..., None]
    light = local + vis * glob
    # Lambert + spherical-Gaussian GGX
    h = d + v[:, None]
    raw_half = torch.sqrt((h * h).sum(-1, keepdim=True))
    half = h / torch.clamp(raw_half, min=half_floor)
    hdn = torch.relu((half * n[:, None]).sum(-1, keepdim=True))
    hdo = torch.relu((half * v[:, None]).sum(-1, keepdim=True))
    raw_ndi = (d * n[:, None]).sum(-1, keepdim=True)
    raw_ndo = (n * v).sum(-1, keepdim=True)[:, None]
    ndi, ndo = torch.relu(raw_ndi), torch.relu(raw_ndo)
    r2 = torch.clamp(rough * rough, min=EPS)[:, None]
    D = torch.exp(2 / r2 * (hdn - 1)) / (r2 * pi)
    F0 = (0.04 * (1 - metal) + base * metal)[:, None]
    F = F0 + (1 - F0) * (1 - hdo) ** 5
    k = ((1 + rough) ** 2 / 8)[:, None]
    den_i, den_o = ndi * (1 - k) + k, ndo * (1 - k) + k
    V = 0.5 / torch.clamp(den_i, min=EPS) * (0.5 / torch.clamp(den_o, min=EPS))
    fd = ((1 - metal) * base / pi)[:, None]
    fs = D * F * V
    w = ndi * (2 * pi / Ns) if Ns else ndi
    if drop_sample is not None:
        keep = torch.ones(Ns, dtype=dtype)
        keep[drop_sample] = 0
        w = w * keep[None, :, None]
    tr = light * w
    out = {"pbr": ((fd + fs) * tr).sum(1), "diffuse_light": tr.sum(1), "local_diffuse_light": (local * w).sum(1),
           "rgb_d": (fd * tr).sum(1), "rgb_s": (fs * tr).sum(1), "incident_dirs": d, "incident_lights": light,
           "local_incident_lights": local, "global_incident_lights": vis * glob, "incident_visibility": vis}
    out["accum"] = (out["diffuse_light"] / pi + out["rgb_s"]).mean(-1, keepdim=True)
    raw = dict(raw_local=raw_local, raw_global=raw_global, raw_vis=raw_vis, raw_half=raw_half[..., 0],
               raw_ndi=raw_ndi[..., 0], raw_ndo=raw_ndo[:, 0, 0], raw_r2=(rough * rough)[:, 0], raw_cp1=n[:, 2] + 1,
               raw_den_i=den_i[..., 0], raw_den_o=den_o[:, 0, 0])
    res = {kk: vv.detach().numpy() for kk, vv in {**out, **raw}.items()}
    if upstream is not None:
        gp, gd = (_t(u, dtype) for u in upstream)
        loss = (out["pbr"] * gp).sum() + (out["diffuse_light"] * gd).sum()
        grads = torch.autograd.grad(loss, [t[kk] for kk in GRAD_KEYS], allow_unused=True)
        for kk, g in zip(GRAD_KEYS, grads):
            g = torch.zeros_like(t[kk]) if g is None else g.clone()
            if kk == "incidents" and incident_cap:
                g[:, min(Sd, Si):] = 0  # the reference's update loop runs over S_direct coefficients
            res["grad_" + kk] = g.numpy()
    return res
