"""Float64 restatement of the relighting render equation (csrc/relight.hip; the reference's
gaussian_renderer/neilf_composite.py rendering_equation_python with is_training=False, and
scene/envmap.py EnvLight.direct_light), in torch, vectorised over (Gaussian, sample).

Test infrastructure only (not collected: no test_ prefix). Written from the formulas: unrotated
Fibonacci directions (z_r = 1 - 2 r / (2 Ns - 1), azimuth r pi (3 - sqrt 5)) turned to the normal by
R = I + K + K^2 / max(1 + n_z, 1e-7), K the cross-product matrix of (-n_y, n_x, 0), and by -I where
1 + n_z <= 0; the SH basis to degree 4; local light ReLU(sum), global light none / ReLU(sum + 0.5) /
environment map (unclamped), visibility clamp(sum + 0.5, 0, 1) or the caller's traced values, each SH
sum cut to its own width; Lambert + spherical-Gaussian GGX with pi = math.pi and the reference Python's
floors (1e-7 on r^2 and the two GGX denominators, 1e-12 in the two normalisations).

The environment lookup: d' = T d, v = (d'.x, d'.z, -d'.y), tu = atan2(v.x, -v.z) / 2 pi + 0.5,
tv = acos(clamp(v.y, -1, 1)) / pi, then the bilinear filter of nvdiffrast's dr.texture(filter_mode=
'linear', boundary_mode='wrap'): u <- u - floor(u), x = u W - 0.5, x0 = floor(x), weight x - x0, texels
x0 and x0 + 1 modulo W; the same in v with H. At a pole (d' = (0, 0, +-1)) the lookup is discontinuous in the
direction: tu is atan2 of two zeros and follows their signs, as the HIP kernel's atan2f(d'.x, d'.y) does.
Near a pole it is ill-conditioned in proportion to 1 / sin(polar angle): a direction 3e-3 rad from a pole
turns the 3e-5 rad rounding of a late sample's angle into 1e-2 of a texel.

FLOORS / BARS: the float32 noise floor of each output is the reference's own float32 result (the golden
file) against this restatement, max|golden - ref64| / max|ref64| over the golden cases, and the HIP bar
is 4 x that floor (the margin of GRAD_BARS: it allows for another summation order and another expf /
sincosf). Measured by

    python tests/golden/make_golden_relight.py --floors

which prints the maxima quoted at the constants (floors are those maxima rounded up to two digits). The
largest, 5.3e-5 on rgb at Ns = 384 under the environment map, is large for a float32 result for two
reasons that the HIP kernel shares with the reference: the reference forms the sample angle as
float(delta) * r, a product rounded to 6e-5 rad at r = 383, and the specular lobe exp(2 (h.n - 1) / r^2)
multiplies every rounding of h.n by 2 / r^2, up to 800 at the lowest roughness. The rgb floor therefore
depends on the draw: on other seeded inputs the reference's float32 rgb is 1.4e-5 (P = 257, Ns = 24) to
1.9e-4 (P = 257, Ns = 256) away from this restatement, where the 64 + 8 golden Gaussians give 5.3e-5.
A bar of 4 x 5.4e-5 does not separate np.pi from the CUDA kernels' 3.14159 on rgb (9e-5 at Ns = 24); the
light means, with bars of 3.4e-6 to 1.8e-5, and the comparison with the golden file itself do.
tests/test_relight_ref.py asserts golden-vs-ref64 <= floor = bar / 4, so the constants cannot drift
away from the measurement.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests.brdf_ref64 import C0, C1, C2, C3

C4 = (2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431,
      -0.6690465435572892, 0.47308734787878004, -1.7701307697799304, 0.6258357354491761)

LIGHT_NONE, LIGHT_SH, LIGHT_MAP = 0, 1, 2
FEATURE_COLUMNS = {"rgb": (0, 3), "normal": (3, 6), "base_color": (6, 9), "roughness": (9, 10), "metallic": (10, 11),
                   "incident_lights": (11, 14), "local_incident_lights": (14, 17),
                   "global_incident_lights": (17, 20), "incident_visibility": (20, 21)}
OUTPUT_KEYS = ["rgb", "incident_lights", "local_incident_lights", "global_incident_lights", "incident_visibility"]

# max|golden - ref64| / max|ref64| per output over the golden cases, rounded up (see the docstring).
# Measured: rgb 5.318e-05 (Ns = 384, map), incident_lights 4.274e-06, local_incident_lights 8.428e-07,
# global_incident_lights 4.295e-06, incident_visibility 1.655e-07; the envmap lookup alone 7.783e-07
FLOORS = {"rgb": 5.4e-5, "incident_lights": 4.3e-6, "local_incident_lights": 8.5e-7, "global_incident_lights": 4.3e-6,
          "incident_visibility": 1.7e-7}
ENVMAP_FLOOR = 7.8e-7
BARS = {k: 4 * v for k, v in FLOORS.items()}  # the HIP bars
ENVMAP_BAR = 4 * ENVMAP_FLOOR


def _t(a):
    return a.to(torch.float64) if torch.is_tensor(a) else torch.tensor(np.asarray(a, np.float64))


def sh_basis25(d):
    """The 25 real SH basis values of degree <= 4 along d [..., 3] -> [..., 25]."""
    x, y, z = d.unbind(-1)
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return torch.stack([
        torch.full_like(x, C0), -C1 * y, C1 * z, -C1 * x,
        C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
        C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy),
        C3[3] * z * (2 * zz - 3 * xx - 3 * yy), C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy),
        C3[6] * x * (xx - 3 * yy),
        C4[0] * xy * (xx - yy), C4[1] * yz * (3 * xx - yy), C4[2] * xy * (7 * zz - 1), C4[3] * yz * (7 * zz - 3),
        C4[4] * (zz * (35 * zz - 30) + 3), C4[5] * xz * (7 * zz - 3), C4[6] * (xx - yy) * (7 * zz - 1),
        C4[7] * xz * (xx - 3 * yy), C4[8] * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))], -1)


def fibonacci_dirs(normals, Ns):
    """Unit sample directions [P, Ns, 3] about normals [P, 3] (no random rotation)."""
    n = _t(normals)
    P = n.shape[0]
    ray = torch.arange(Ns, dtype=torch.float64)
    z = 1 - 2 * ray / (2 * Ns - 1)
    rad = torch.sqrt(1 - z * z)
    theta = math.pi * (3 - math.sqrt(5.0)) * ray
    local = torch.stack([torch.sin(theta) * rad, torch.cos(theta) * rad, z], -1).expand(P, Ns, 3)
    K = torch.zeros(P, 3, 3, dtype=torch.float64)
    K[:, 0, 2] = n[:, 0]
    K[:, 2, 0] = -n[:, 0]
    K[:, 1, 2] = n[:, 1]
    K[:, 2, 1] = -n[:, 1]
    cp1 = n[:, 2] + 1
    eye = torch.eye(3, dtype=torch.float64)
    R = eye + K + (K @ K) / torch.clamp(cp1, min=1e-7)[:, None, None]
    # -I as a negation, not a matrix product: the product's accumulator turns the -0 components of
    # -(0, 0, 1) into +0, and at that direction, a pole of the environment lookup, atan2 reads the sign
    o = torch.where((cp1 > 0)[:, None, None], torch.einsum("pij,pnj->pni", R, local), -local)
    return o / torch.clamp(torch.sqrt((o * o).sum(-1, keepdim=True)), min=1e-12)


def texcoords(dirs, transform=None):
    """(tu, tv) of directions [..., 3]."""
    d = _t(dirs)
    if transform is not None:
        d = torch.einsum("ij,...j->...i", _t(transform), d)
    vx, vy, vz = d[..., 0], d[..., 2], -d[..., 1]
    tu = torch.atan2(vx, -vz) / (2 * math.pi) + 0.5
    tv = torch.acos(torch.clamp(vy, -1, 1)) / math.pi
    return tu, tv


def bilinear_wrap(envmap, tu, tv):
    """nvdiffrast's linear filter with wrap in both axes: envmap [H, W, C], tu / tv [...] -> [..., C]."""
    m = _t(envmap)
    H, W = m.shape[0], m.shape[1]

    def axis(u, n):
        u = u - torch.floor(u)
        x = u * n - 0.5
        x0 = torch.floor(x)
        i0 = x0.to(torch.int64)
        return i0 % n, (i0 + 1) % n, x - x0

    x0, x1, fx = axis(tu, W)
    y0, y1, fy = axis(tv, H)
    fx, fy = fx[..., None], fy[..., None]
    return (m[y0, x0] * (1 - fx) * (1 - fy) + m[y0, x1] * fx * (1 - fy) + m[y1, x0] * (1 - fx) * fy +
            m[y1, x1] * fx * fy)


def envmap_direct_light(dirs, envmap, transform=None):
    """EnvLight.direct_light: dirs [..., 3] -> [..., 3] (numpy float64)."""
    tu, tv = texcoords(dirs, transform)
    return bilinear_wrap(envmap, tu, tv).numpy()


def render(inp, Ns, light_mode, envmap=None, transform=None, traced=None):
    """The five outputs (OUTPUT_KEYS, numpy float64) and "features" [P, 21] for inputs inp = {base, rough,
    metal, normals, viewdirs, incidents [P, Si, 3], env [1, Sd, 3] (LIGHT_SH), visibility [P, Sv, 1] (baked)};
    traced [P, Ns(, 1)] replaces the baked visibility."""
    base, rough, metal = _t(inp["base"]), _t(inp["rough"]), _t(inp["metal"])
    n, v, inc = _t(inp["normals"]), _t(inp["viewdirs"]), _t(inp["incidents"])
    P = base.shape[0]
    d = fibonacci_dirs(n, Ns)
    Y = sh_basis25(d)
    local = torch.relu(torch.einsum("pnk,pkc->pnc", Y[..., :inc.shape[1]], inc))
    if light_mode == LIGHT_SH:
        env = _t(inp["env"])[0]
        glob = torch.relu(0.5 + torch.einsum("pnk,kc->pnc", Y[..., :env.shape[0]], env))
    elif light_mode == LIGHT_MAP:
        tu, tv = texcoords(d, transform)
        glob = bilinear_wrap(envmap, tu, tv)
    else:
        glob = torch.zeros_like(local)
    if traced is not None:
        vis = _t(traced).reshape(P, Ns, 1)
    else:
        vsh = _t(inp["visibility"])[..., 0]
        vis = torch.clamp(0.5 + torch.einsum("pnk,pk->pn", Y[..., :vsh.shape[1]], vsh), 0.0, 1.0)[..., None]
    glob = glob * vis
    light = local + glob
    h = d + v[:, None]
    half = h / torch.clamp(torch.sqrt((h * h).sum(-1, keepdim=True)), min=1e-12)
    hdn = torch.relu((half * n[:, None]).sum(-1, keepdim=True))
    hdo = torch.relu((half * v[:, None]).sum(-1, keepdim=True))
    ndi = torch.relu((d * n[:, None]).sum(-1, keepdim=True))
    ndo = torch.relu((n * v).sum(-1, keepdim=True))[:, None]
    r2 = torch.clamp(rough * rough, min=1e-7)[:, None]
    D = torch.exp(2 / r2 * (hdn - 1)) / (r2 * math.pi)
    F0 = (0.04 * (1 - metal) + base * metal)[:, None]
    F = F0 + (1 - F0) * (1 - hdo) ** 5
    k = ((1 + rough) ** 2 / 8)[:, None]
    V = 0.5 / torch.clamp(ndi * (1 - k) + k, min=1e-7) * (0.5 / torch.clamp(ndo * (1 - k) + k, min=1e-7))
    fd = ((1 - metal) * base / math.pi)[:, None]
    fs = D * F * V
    tr = light * (2 * math.pi) * ndi
    out = {"rgb": (fd * tr).mean(1) + (fs * tr).mean(1), "incident_lights": light.mean(1),
           "local_incident_lights": local.mean(1), "global_incident_lights": glob.mean(1),
           "incident_visibility": vis.mean(1)}
    feats = torch.cat([out["rgb"], n, base, rough, metal, out["incident_lights"], out["local_incident_lights"],
                       out["global_incident_lights"], out["incident_visibility"]], -1)
    res = {kk: vv.numpy() for kk, vv in out.items()}
    res["features"] = feats.numpy()
    return res


def rel_err(got, ref):
    """max|got - ref| / max|ref| (0 / 0 = 0: an output that is identically zero, as the global light of
    LIGHT_NONE, must be reproduced exactly)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    num, den = float(np.abs(got - ref).max()) if got.size else 0.0, float(np.abs(ref).max()) if ref.size else 0.0
    if den == 0.0:
        return 0.0 if num == 0.0 else math.inf
    return num / den
