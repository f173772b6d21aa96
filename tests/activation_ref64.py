"""float64 numpy restatement of the parameter activations (csrc/activation.hip, include/r3dg_hip.h
"parameter activations"): the getters of scene/gaussian_model.py:23-44, 331-413 and neilf.py:102 forward, and
their gradients as the header states them. No torch here: the backward is written out, and
tests/test_activation_ref.py holds it against a float64 central difference of the forward.

Error measure (`row_err`): per Gaussian max_c |got - ref| over the row, divided by max(max_c |ref| over the
row, 1e-37); the worst row counts. The absolute term forgives only a flushed denormal (sigmoid(-100) is
3.8e-44). A whole-array maximum would hide everything here: symm_inv reaches 2e10 at scaling = -12, and a normal
of length 1e-4 has gradients of 1e3 beside rows of order 1. No row is left out of any comparison.

FLOORS are the distances of the reference's own float32 results (tests/golden/activation.npz, torch on the
CPU) from this file, as `python tests/golden/make_golden_activation.py --floors` prints them, rounded up to two
digits; BARS = 4 x FLOORS is the project's margin for another expf and another operation order, here also for
the projection form of the normalise gradient, which sums in another order than autograd. The SH concatenations
are copies: floor 0, compared with array_equal.

What the floors say about float32, not about the kernels:
  * grad_opacity is 1.0, so its bar is loose: the draw's opacity row 3 is +20, where float32 rounds
    sigmoid to exactly 1 and s (1 - s) to 0 while float64 keeps 2.1e-9 g. The other sigmoid gradients carry
    the same cancellation (1 - s loses |x| / ln 2 bits) at the largest |x| of the golden draw, so another draw
    with a larger |x| would not meet them in the reference's arithmetic. The kernel avoids the cancellation
    (t / (1 + t)^2, t = e^-|x|), and tests/test_gpu_activation.py also holds every sigmoid gradient against a
    16 x 2^-24 bar derived from that expression.
  * grad_normal, grad_rotation and grad_xyz depend on the draw in the same way: the projection
    g - y (y.g) cancels where g is nearly parallel to x, so the float32 floor is set by the worst-aligned row
    of the golden draw. The kernel evaluates the projection in double and rounds once.
  * symm_inv and the rotation outputs include the row of length 1e-6 (forward comparisons only).
"""
from __future__ import annotations

import numpy as np

F = np.float32
BASE_GROUPS = [("xyz", (3,)), ("normal", (3,)), ("rotation", (4,)), ("scaling", (3,)), ("opacity", (1,)),
               ("f_dc", (1, 3)), ("f_rest", (15, 3))]
PBR_GROUPS = [("base_color", (3,)), ("roughness", (1,)), ("metallic", (1,)), ("incidents_dc", (1, 3)),
              ("incidents_rest", (15, 3)), ("visibility_dc", (1, 1)), ("visibility_rest", (15, 1))]
CAMPOS = np.array([0.3, -4.0, 1.1], F)
EPS_NORMAL, EPS_UNIT = 1e-3, 1e-12
SIGMOIDS = ("opacity", "base_color", "roughness", "metallic")
# output -> (dc group, rest group)
SH = {"shs": ("f_dc", "f_rest"), "incidents": ("incidents_dc", "incidents_rest"),
      "visibility": ("visibility_dc", "visibility_rest")}
OUTPUT_SHAPES = {"xyz": (3,), "scaling": (3,), "rotation": (4,), "normal": (3,), "opacity": (1,), "shs": (16, 3),
                 "base_color": (3,), "roughness": (1,), "metallic": (1,), "incidents": (16, 3),
                 "visibility": (16, 1), "viewdirs": (3,)}


def groups_of(n_groups: int) -> list:
    assert n_groups in (7, 14)
    return BASE_GROUPS + (PBR_GROUPS if n_groups == 14 else [])


def normal_regions(P: int) -> dict:
    """Row indices of the four regimes of draw_case's normals."""
    e = P // 8
    return {"below": np.arange(0, e), "above": np.arange(e, 2 * e), "zero": np.array([2 * e]),
            "ordinary": np.arange(2 * e + 1, P)}


def short_rotation_row(P: int) -> int:
    return P // 2


def draw_case(P: int, seed: int, groups: int = 14) -> dict:
    """name -> float32 [P, *shape] raw parameters. `rotation_fwd` is `rotation` with one row scaled by 1e-6:
    forward comparisons use it, gradient comparisons the unmodified draw (a row that short carries unit-scale
    upstream gradients multiplied by 1e6 beside rows of order 1, and its projection cancels catastrophically)."""
    rng = np.random.default_rng(seed)
    c = {"xyz": rng.normal(0, 1.5, (P, 3)), "scaling": rng.uniform(-12, 3, (P, 3)), "opacity": rng.normal(0, 4, (P, 1)),
         "rotation": rng.normal(0, 1, (P, 4)), "f_dc": rng.normal(0, 0.3, (P, 1, 3)),
         "f_rest": rng.normal(0, 0.3, (P, 15, 3))}
    sat = np.array([-100.0, 100.0, -20.0, 20.0])
    c["opacity"][:min(P, 4), 0] = sat[:min(P, 4)]
    n = rng.normal(0, 1, (P, 3))
    reg = normal_regions(P)
    unit = n / np.linalg.norm(n, axis=1, keepdims=True)
    n[reg["below"]] = unit[reg["below"]] * rng.uniform(5e-5, 4.95e-4, (len(reg["below"]), 1))
    n[reg["above"]] = unit[reg["above"]] * rng.uniform(1.01e-3, 3e-3, (len(reg["above"]), 1))
    if P:
        n[reg["zero"]] = 0.0
    c["normal"] = n
    if groups == 14:
        for name, shape in PBR_GROUPS:
            c[name] = rng.normal(0, 3 if len(shape) == 1 else 0.3, (P, *shape))
    c = {k: np.ascontiguousarray(v, F) for k, v in c.items()}
    # no normal within 1 % of eps: float32 and float64 take the same branch on every row
    ln = np.linalg.norm(c["normal"].astype(np.float64), axis=1)
    assert not np.any(np.abs(ln - EPS_NORMAL) < 1e-5)
    c["rotation_fwd"] = c["rotation"].copy()
    if P:
        c["rotation_fwd"][short_rotation_row(P)] *= F(1e-6)
    return c


def draw_upstreams(P: int, seed: int, groups: int = 14, campos: bool = True) -> dict:
    """output name -> float32 N(0, 1) upstream gradient (symm_inv has none)."""
    rng = np.random.default_rng(seed)
    names = ["xyz", "scaling", "rotation", "normal", "opacity", "shs"]
    if groups == 14:
        names += ["base_color", "roughness", "metallic", "incidents", "visibility"]
    if campos:
        names += ["viewdirs"]
    return {n: rng.normal(0, 1, (P, *OUTPUT_SHAPES[n])).astype(F) for n in names}


def _normalize(x, eps):
    r = np.sqrt((x * x).sum(-1, keepdims=True))
    return x / np.maximum(r, eps)


def _normalize_bwd(x, g, eps):
    r = np.sqrt((x * x).sum(-1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        y = x / r
        proj = (g - y * (y * g).sum(-1, keepdims=True)) / r
    return np.where(r >= eps, proj, g / eps)


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def symm_inverse(rotation_act, scaling_act):
    """get_inverse_covariance (gaussian_model.py:410-413) of the ACTIVATED rotation and scaling."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = rotation_act / np.sqrt((rotation_act * rotation_act).sum(-1, keepdims=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    L = R * (1.0 / scaling_act)[:, None, :]
    S = L @ L.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)


def forward(c: dict, campos=None, inverse_covariance: bool = False, rotation: str = "rotation") -> dict:
    """float64 outputs of raw parameters c (name -> array); `rotation` names the rotation draw to use."""
    c = {k: np.asarray(v, np.float64) for k, v in c.items()}
    out = {"xyz": c["xyz"], "scaling": np.exp(c["scaling"]), "rotation": _normalize(c[rotation], EPS_UNIT),
           "normal": _normalize(c["normal"], EPS_NORMAL)}
    for n in SIGMOIDS:
        if n in c:
            out[n] = _sigmoid(c[n])
    for n, (dc, rest) in SH.items():
        if dc in c:
            out[n] = np.concatenate([c[dc], c[rest]], 1)
    if campos is not None:
        out["viewdirs"] = _normalize(np.asarray(campos, np.float64)[None] - c["xyz"], EPS_UNIT)
    if inverse_covariance:
        out["symm_inv"] = symm_inverse(out["rotation"], out["scaling"])
    return out


def backward(c: dict, ups: dict, campos=None) -> dict:
    """float64 gradient of every group of c; ups: output name -> upstream (a missing one is zero)."""
    c = {k: np.asarray(v, np.float64) for k, v in c.items() if k != "rotation_fwd"}
    ups = {k: np.asarray(v, np.float64) for k, v in ups.items() if v is not None}
    g = {k: np.zeros_like(v) for k, v in c.items()}
    if "xyz" in ups:
        g["xyz"] = g["xyz"] + ups["xyz"]
    if "viewdirs" in ups:
        v = np.asarray(campos, np.float64)[None] - c["xyz"]
        g["xyz"] = g["xyz"] - _normalize_bwd(v, ups["viewdirs"], EPS_UNIT)
    if "normal" in ups:
        g["normal"] = _normalize_bwd(c["normal"], ups["normal"], EPS_NORMAL)
    if "rotation" in ups:
        g["rotation"] = _normalize_bwd(c["rotation"], ups["rotation"], EPS_UNIT)
    if "scaling" in ups:
        g["scaling"] = ups["scaling"] * np.exp(c["scaling"])
    for n in SIGMOIDS:
        if n in ups:
            s = _sigmoid(c[n])
            g[n] = ups[n] * s * (1.0 - s)
    for n, (dc, rest) in SH.items():
        if n in ups:
            g[dc], g[rest] = ups[n][:, :1], ups[n][:, 1:]
    return g


def row_err(got, ref) -> float:
    """The worst row's max |got - ref| / max(max |ref|, 1e-37); inf for a non-finite `got` where ref is finite."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.shape[0] == 0:
        return 0.0
    got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float((np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1e-37)).max())


# golden vs this file, rounded up to two digits (make_golden_activation.py --floors); 0: copies
FLOORS = {
    "scaling": 5.9e-8, "rotation": 1.5e-7, "normal": 1.1e-7, "opacity": 3.8e-7, "base_color": 1.0e-7,
    "roughness": 1.0e-7, "metallic": 1.1e-7, "viewdirs": 1.2e-7, "symm_inv": 8.3e-7,
    "shs": 0.0, "incidents": 0.0, "visibility": 0.0,
    "grad_xyz": 3.0e-7, "grad_normal": 1.7e-6, "grad_rotation": 9.1e-7, "grad_scaling": 8.8e-8, "grad_opacity": 1.0,
    "grad_base_color": 1.9e-5, "grad_roughness": 2.1e-4, "grad_metallic": 2.4e-5,
    "grad_f_dc": 0.0, "grad_f_rest": 0.0, "grad_incidents_dc": 0.0, "grad_incidents_rest": 0.0,
    "grad_visibility_dc": 0.0, "grad_visibility_rest": 0.0,
}
BARS = {k: 4.0 * v for k, v in FLOORS.items()}
