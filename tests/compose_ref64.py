"""float64 numpy restatement of scene composition and the points capture (csrc/compose.hip, include/r3dg_hip.h
"scene composition and the points capture"): set_transform of scene/gaussian_model.py:237-262 with
rotation_to_quaternion / quaternion_multiply of utils/general_utils.py:105-149, scene_composition of
relighting.py:31-55 followed by the getters (tests/activation_ref64.py), and render_points of
relighting.py:89-123 as the header defines its result. No torch here. It also draws every seeded case that
tests/golden/make_golden_compose.py, tests/test_compose_ref.py and tests/test_gpu_compose.py use.

Error measure: activation_ref64.row_err (the worst row's max |got - ref| / max |ref| of the row), no row left out.

FLOORS are the distances of the reference's own float32 results (tests/golden/compose.npz, torch on the CPU)
from this file, as `python tests/golden/make_golden_compose.py --floors` prints them, rounded up to two
digits; BARS = 4 x FLOORS, the project's margin for another expf / logf and another operation order. The GPU
tests run on the golden's own draws (its first P rows for the smaller sizes), so a floor speaks about the rows a
bar is held against. Measured (worst over the cases):
  st_xyz 2.015e-07   st_scaling 9.152e-08   st_rotation 1.491e-07   st_normal 1.119e-07
  xyz 3.750e-07   scaling 5.049e-07   rotation 1.660e-07   normal 2.062e-07   opacity 3.720e-07
  base_color 9.302e-08   roughness 9.904e-08   metallic 8.842e-08   symm_inv 1.609e-06
  shs, incidents, visibility_dc, visibility_rest: copies and zeros, 0 (compared with array_equal)
What the floors say about float32, not about the kernels:
  * st_xyz / xyz: a row of A x + t may cancel; the floor is the golden draw's worst row.
  * st_scaling is the RAW group, log(exp(x) * s): its error is an ulp of exp carried through log, relative
    to the row's largest |log|. `scaling` (composed) is exp(log(exp(x) * s)) in the reference and expf(x) * s in
    the kernel: both sit within the bar of exp(x) s.
  * The transforms' rotation parts have 1 + trace >= 0.5. Below that the reference's quaternion formula divides
    small differences by a small qw; that is a condition on the inputs, not a tolerance.

render_points is compared exactly (colours are copies). Its case is built in float64 so that the float32
arithmetic cannot change a decision: every point's u, v lie at least 0.05 px from an integer and the depths of
points sharing a pixel differ by at least 1e-3 relative (tests/test_compose_ref.py checks both for every point).
"""
from __future__ import annotations

import numpy as np

from tests import activation_ref64 as a64

F = np.float32
KINDS = ("transform", "center", "rotation", "scale", "offset", "all")
MOVED = ("xyz", "scaling", "rotation", "normal")
ST_P, ST_SEED = 257, 51                       # the set_transform draw; smaller sizes take its first rows
SCENE_P, SCENE_SEEDS = (63, 1, 257), (61, 62, 63)
FAR = 10000.0
PT_H, PT_W, PT_P, PT_SEED = 37, 53, 4096, 81
PT_BG = np.array([0.25, 0.5, 0.75], F)


# ---- the seeded draws -------------------------------------------------------------------------------------

def draw_rotation(rng) -> np.ndarray:
    """A rotation matrix with 1 + trace >= 0.5 (angle <= 2.2 rad), float64."""
    axis = rng.normal(0, 1, 3)
    axis /= np.linalg.norm(axis)
    th = rng.uniform(0.2, 2.2)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    assert 1 + np.trace(R) >= 0.5
    return R


def draw_kwargs(kind: str, seed: int) -> dict:
    """set_transform's keyword arguments as float32 arrays: a full transform with three different row norms and
    a translation, each component alone, or all four (`scale` a [3] alone, one number in "all")."""
    rng = np.random.default_rng(seed)
    R = draw_rotation(rng)
    s3 = np.array([0.7, 1.3, 2.1]) * rng.uniform(0.9, 1.1, 3)
    t = rng.normal(0, 2.0, 3)
    c = rng.normal(0, 1.0, 3)
    if kind == "transform":
        T = np.eye(4)
        T[:3, :3] = s3[:, None] * R
        T[:3, 3] = t
        return {"transform": T.astype(F)}
    parts = {"center": c.astype(F), "rotation": R.astype(F), "scale": s3.astype(F), "offset": t.astype(F)}
    if kind == "all":
        return dict(parts, scale=np.array([1.7], F))
    return {kind: parts[kind]}


def draw_set_transform_case(groups: int = 14) -> dict:
    return a64.draw_case(ST_P, ST_SEED, groups)


def first_rows(c: dict, P: int) -> dict:
    return {k: np.ascontiguousarray(v[:P]) for k, v in c.items()}


def draw_scene(identity: bool = False) -> list:
    """[(raw parameters, transform [4,4] float32)] of the three objects."""
    out = []
    for i, (P, seed) in enumerate(zip(SCENE_P, SCENE_SEEDS)):
        c = a64.draw_case(P, seed, 14)
        c.pop("rotation_fwd")
        T = np.eye(4, dtype=F) if identity else draw_kwargs("transform", 71 + i)["transform"]
        out.append((c, T))
    return out


# ---- set_transform -------------------------------------------------------------------------------------

def rotation_to_quaternion(R):
    qw = np.sqrt(max(1 + R[0, 0] + R[1, 1] + R[2, 2], 1e-7)) / 2
    q = np.array([qw, (R[2, 1] - R[1, 2]) / (4 * qw), (R[0, 2] - R[2, 0]) / (4 * qw), (R[1, 0] - R[0, 1]) / (4 * qw)])
    return q / max(np.linalg.norm(q), 1e-12)


def quaternion_multiply(q1, q2):
    w1, x1, y1, z1 = q1
    w2, x2, y2, z2 = q2[:, 0], q2[:, 1], q2[:, 2], q2[:, 3]
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], 1)


def moved(c: dict, rotation=None, center=None, scale=None, offset=None, transform=None) -> dict:
    """float64 xyz, normal, rotation (raw, unnormalised) and `scaling_act` = exp(raw) * scale after
    set_transform; the other groups of c are not touched and not returned."""
    d = lambda v: None if v is None else np.asarray(v, np.float64)  # noqa: E731
    xyz, normal, rot = d(c["xyz"]), d(c["normal"]), d(c["rotation"])
    act = np.exp(d(c["scaling"]))
    if transform is not None:
        T = d(transform).reshape(4, 4)
        A = T[:3, :3]
        s = np.sqrt((A * A).sum(1))
        R = A / s[:, None]
        return {"xyz": xyz @ A.T + T[:3, 3], "normal": normal @ R.T,
                "rotation": quaternion_multiply(rotation_to_quaternion(R), rot), "scaling_act": act * s}
    if center is not None:
        xyz = xyz - d(center)
    if rotation is not None:
        R = d(rotation)
        xyz, normal = xyz @ R.T, normal @ R.T
        rot = quaternion_multiply(rotation_to_quaternion(R), rot)
    if scale is not None:
        xyz, act = xyz * d(scale), act * d(scale)
    if offset is not None:
        xyz = xyz + d(offset)
    return {"xyz": xyz, "normal": normal, "rotation": rot, "scaling_act": act}


def set_transform(c: dict, **kw) -> dict:
    """The four raw groups after set_transform (scaling = log(exp(raw) * scale))."""
    m = moved(c, **kw)
    return {"xyz": m["xyz"], "scaling": np.log(m["scaling_act"]), "rotation": m["rotation"], "normal": m["normal"]}


# ---- scene composition -----------------------------------------------------------------------------------

def compose(objects: list) -> dict:
    """float64 fields of the ComposedScene of [(raw parameters, transform or None)]."""
    rows = []
    for c, T in objects:
        m = moved(c, transform=T) if T is not None else moved(c)
        c2 = dict(c, xyz=m["xyz"], normal=m["normal"], rotation=m["rotation"])
        o = a64.forward(c2)
        o["scaling"] = m["scaling_act"]
        o["symm_inv"] = a64.symm_inverse(o["rotation"], o["scaling"])
        o["incidents"] = np.zeros_like(o["incidents"])
        vis = np.asarray(c["visibility_rest"], np.float64)
        o["visibility_dc"] = np.asarray(c["visibility_dc"], np.float64)
        o["visibility_rest"] = np.concatenate([vis, np.zeros((vis.shape[0], 9, 1))], 1)
        del o["visibility"]
        rows.append(o)
    return {k: np.concatenate([o[k] for o in rows], 0) for k in rows[0]}


COPIES = ("shs", "incidents", "visibility_dc", "visibility_rest")


# ---- the points capture ----------------------------------------------------------------------------------

def project(xyz, view, K):
    """float64 (u, v, z) of relighting.py:90-99 from the given (float32) arrays."""
    xyz, view, K = (np.asarray(a, np.float64) for a in (xyz, view, K))
    cam = xyz @ view[:3, :3] + view[3, :3]
    h = cam @ K.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return h[:, 0] / h[:, 2], h[:, 1] / h[:, 2], cam[:, 2]


def render_points(xyz, color, view, K, H, W, bg, dtype=np.float64):
    """The header's definition, evaluated in `dtype`: (rgb [3,H,W] float32, depth [H,W] dtype, winner [H,W] int64,
    -1 where empty)."""
    xyz, view, K = (np.asarray(a, dtype) for a in (xyz, view, K))
    P = xyz.shape[0]
    cam = (xyz[:, 0:1] * view[0, :3] + xyz[:, 1:2] * view[1, :3]) + xyz[:, 2:3] * view[2, :3] + view[3, :3]
    h = [(cam[:, 0] * K[i, 0] + cam[:, 1] * K[i, 1]) + cam[:, 2] * K[i, 2] for i in range(3)]
    z = cam[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = h[0] / h[2], h[1] / h[2]
    ok = np.isfinite(u) & np.isfinite(v)
    tu, tv = np.trunc(np.where(ok, u, -1)), np.trunc(np.where(ok, v, -1))
    ok &= (tu >= 0) & (tu < W) & (tv >= 0) & (tv < H) & (z < dtype(FAR))
    idx = np.flatnonzero(ok)
    pix = tv[idx].astype(np.int64) * W + tu[idx].astype(np.int64)
    order = np.lexsort((idx, z[idx], pix))  # by pixel, then depth, then index
    pix_s, idx_s = pix[order], idx[order]
    first = np.ones(len(order), bool)
    first[1:] = pix_s[1:] != pix_s[:-1]
    winner = np.full(H * W, -1, np.int64)
    winner[pix_s[first]] = idx_s[first]
    rgb = np.empty((3, H * W), F)
    rgb[:] = np.broadcast_to(np.asarray(bg, F).reshape(-1), (3,))[:, None]
    depth = np.full(H * W, dtype(FAR), dtype)
    hit = winner >= 0
    rgb[:, hit] = np.asarray(color, F)[winner[hit]].T
    depth[hit] = z[winner[hit]]
    assert P == len(u)
    return rgb.reshape(3, H, W), depth.reshape(H, W), winner.reshape(H, W)


def draw_points_case() -> dict:
    """xyz, color [P,3], view (the transposed world-view [4,4]), K [3,3], all float32. Built backwards from
    chosen (u, v, z): fractions of u, v in [0.1, 0.9], every |z| on its own rung of a geometric ladder of ratio
    1.002 (so any two depths differ by 2e-3 relative). Groups: 256 points in pixel (20, 11); points off each of
    the four sides; u or v in (-1, 0); points behind the camera inside the image; z >= 10000; the rest spread
    over the columns below W - 6, which leaves the last columns to the groups above and some pixels empty."""
    rng = np.random.default_rng(PT_SEED)
    P, H, W = PT_P, PT_H, PT_W
    frac = lambda n: rng.uniform(0.1, 0.9, n)  # noqa: E731
    u = rng.integers(0, W - 6, P) + frac(P)
    v = rng.integers(0, H, P) + frac(P)
    z = 0.5 * 1.002 ** rng.permutation(P).astype(np.float64)  # 0.5 .. 1800
    g = np.arange(P)
    deep = g < 256
    u[deep], v[deep] = 20 + frac(256), 11 + frac(256)
    for k, (uu, vv) in enumerate([(-3.5, 5.5), (W + 2.5, 6.5), (7.5, -4.5), (8.5, H + 1.5)]):  # off the four sides
        sel = (g >= 256 + 8 * k) & (g < 264 + 8 * k)
        u[sel], v[sel] = uu, vv
    neg_u, neg_v = (g >= 288) & (g < 296), (g >= 296) & (g < 304)
    u[neg_u], v[neg_v] = -frac(8), -frac(8)       # (-1, 0): column / row 0
    u[neg_v] = W - 2 + frac(8)                     # a column that only this group reaches
    behind = (g >= 304) & (g < 320)
    z[behind] = -z[behind]
    u[behind] = np.where(np.arange(16) < 8, W - 4 + frac(16), u[behind])  # 8 alone in a column, 8 among others
    far = (g >= 320) & (g < 336)
    z[far] = 10010.0 * 1.002 ** np.arange(16)
    fx, fy, cx, cy = 60.0, 58.0, 26.25, 18.75
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    cam = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    R = draw_rotation(rng)
    t = np.array([0.3, -0.2, 4.0])
    view = np.eye(4)
    view[:3, :3], view[3, :3] = R.T, t           # cam = x @ R.T + t
    xyz = (cam - t) @ R
    color = rng.uniform(0, 1, (P, 3))
    return {"xyz": xyz.astype(F), "color": color.astype(F), "view": view.astype(F), "K": K.astype(F)}


POINT_GROUPS = {"deep": (0, 256), "off": (256, 288), "neg_u": (288, 296), "neg_v": (296, 304), "behind": (304, 320),
                "far": (320, 336)}

# golden vs this file, rounded up to two digits (make_golden_compose.py --floors); 0: copies
FLOORS = {
    "st_xyz": 2.1e-7, "st_scaling": 9.2e-8, "st_rotation": 1.5e-7, "st_normal": 1.2e-7,
    "xyz": 3.8e-7, "scaling": 5.1e-7, "rotation": 1.7e-7, "normal": 2.1e-7, "opacity": 3.8e-7, "base_color": 9.4e-8,
    "roughness": 1.0e-7, "metallic": 8.9e-8, "symm_inv": 1.7e-6,
    "shs": 0.0, "incidents": 0.0, "visibility_dc": 0.0, "visibility_rest": 0.0,
}
BARS = {k: 4.0 * v for k, v in FLOORS.items()}
