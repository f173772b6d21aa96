"""Scenes that drive the rasterizer's branches no generator of synthetic.py reaches, shared by the CPU
tests of the oracle (tests/test_ref64.py) and the GPU tests of the HIP path (tests/test_gpu_edges.py).

Each case is built from synthetic.small_scene at 96 x 64 or smaller, seeded, and carries a `covers`
check, evaluated on the oracle's forward / backward (and on ref64.tile_blend's masks where it needs
them), that the scene really exercises its branch. The oracle's forward, upstream gradients and
backward of a case are computed once per process and must be left unchanged by their users.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from relightable3dgaussian_amd import synthetic
from tests._helpers import upstream_grads

COLOURED = (0.1, 0.9, 0.4)
BLACK = (0.0, 0.0, 0.0)
WHITE = (1.0, 1.0, 1.0)


@dataclass
class Case:
    name: str
    scene: synthetic.Scene
    cam: synthetic.Camera
    S: int
    degree: int = 3
    scale_modifier: float = 1.0
    bg: tuple = WHITE
    seed: int = 1  # of the upstream gradients


def _replace(scene, **kw):
    f = dict(means3D=scene.means3D, scales=scene.scales, rotations=scene.rotations, opacity=scene.opacity,
             sh=scene.sh, features=scene.features)
    f.update(kw)
    return synthetic.Scene(**{k: np.ascontiguousarray(v, np.float32) for k, v in f.items()})


# One seed per kind of scene. Where a seed was changed, it was because the scene's f32 rounding floor (see
# tests/test_ref64.py) or its coverage check asked for another scene, never to fit the code under test.
SEEDS = {"frustum_edge": 68, "modifier": 60, "sh_low_degree": 30, "opaque": 31, "coloured_bg": 32}


def _frustum_edge_scene(seed):
    scene, cam = synthetic.small_scene(P=2500, S=11, seed=seed, width=96, height=64, scale_range=(0.05, 0.4))
    m = scene.means3D.copy()
    m[:, :2] *= 1.7 / 1.2  # small_scene fills 1.2 tan(fov / 2): now 1.7, past the clamp at 1.3
    return _replace(scene, means3D=m), cam


def clamped_xy(case):
    """(x, y) masks of the Gaussians whose t.x / t.z, t.y / t.z lie outside +-1.3 tan(fov / 2) (float64)."""
    cam = case.cam
    v = np.asarray(cam.view, np.float64)
    t = case.scene.means3D.astype(np.float64) @ v[:3, :3] + v[3, :3]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(t[:, 0] / t[:, 2]) > 1.3 * cam.tanfovx, np.abs(t[:, 1] / t[:, 2]) > 1.3 * cam.tanfovy


def _build(name):
    kind, _, arg = name.partition("-")
    if kind == "frustum_edge":
        scene, cam = _frustum_edge_scene(SEEDS[kind])
        return Case(name, scene, cam, 11, seed=11)
    if kind == "modifier":
        scene, cam = _frustum_edge_scene(SEEDS[kind])
        norms = np.random.default_rng(72).uniform(0.8, 1.25, (scene.P, 1))
        return Case(name, _replace(scene, rotations=scene.rotations * norms), cam, 11, scale_modifier=float(arg),
                    seed=12)
    if kind == "sh_low_degree":
        scene, cam = synthetic.small_scene(P=1500, S=3, seed=SEEDS[kind], width=64, height=48)
        rng = np.random.default_rng(73)
        sh = np.empty((scene.P, 16, 3), np.float32)
        sh[:, 0] = (rng.uniform(-0.3, 1.0, (scene.P, 3)) - 0.5) / 0.28209479
        sh[:, 1:] = rng.normal(0, 0.25, (scene.P, 15, 3))
        return Case(name, _replace(scene, sh=sh), cam, 3, degree=int(arg), seed=13)
    if kind == "opaque":
        scene, cam = synthetic.small_scene(P=800, S=11, seed=SEEDS[kind], width=96, height=64, scale_range=(0.1, 0.5))
        rng = np.random.default_rng(74)
        op = scene.opacity.copy()
        order = rng.permutation(scene.P)
        q = scene.P // 4
        op[order[:q]] = 1.0
        op[order[q:2 * q], 0] = rng.uniform(0.99, 1.0, q)
        return Case(name, _replace(scene, opacity=op), cam, 11, bg=COLOURED, seed=14)
    if kind == "coloured_bg":
        scene, cam = synthetic.small_scene(P=2500, S=11, seed=SEEDS[kind], width=96, height=64)
        return Case(name, scene, cam, 11, bg=BLACK if arg == "black" else COLOURED, seed=15)
    raise KeyError(name)


NAMES = ["frustum_edge", "modifier-0.6", "modifier-1.7", "sh_low_degree-0", "sh_low_degree-1", "sh_low_degree-2",
         "opaque", "coloured_bg-colour", "coloured_bg-black"]


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


@functools.lru_cache(maxsize=None)
def oracle_run(name, use_cov=False):
    """(forward, upstream gradients, backward) of the oracle on the case: shared, read-only."""
    import oracle

    c = case(name)
    sc = c.scene
    cov = oracle.cov3d(sc.scales, sc.rotations, c.scale_modifier) if use_cov else None
    o = oracle.rasterize_forward(c.cam, sc.means3D, sc.opacity, sc.features[:, :c.S], sh=sc.sh, degree=c.degree,
                                 scales=None if use_cov else sc.scales, rotations=None if use_cov else sc.rotations,
                                 cov3D_precomp=cov, bg=c.bg, scale_modifier=c.scale_modifier)
    up = upstream_grads(c.cam.height, c.cam.width, c.S, seed=c.seed)
    return o, up, oracle.rasterize_backward(o, *up)


def covers(name, o, go, blend=None):
    """Assert that the case exercises its branch. o / go: the oracle's forward / backward; blend: the
    result of ref64.tile_blend on the oracle's forward (`opaque` needs its masks)."""
    c = case(name)
    kind = name.partition("-")[0]
    vis = o["radii"] > 0
    if kind in ("frustum_edge", "modifier"):
        cx, cy = clamped_xy(c)
        live = vis & (np.abs(go["dL_dconic"]).max(1) > 0)
        nx, ny, nxy = int((cx & live).sum()), int((cy & live).sum()), int((cx & cy & live).sum())
        n = int(((cx | cy) & live).sum())
        print(f"{name}: clamped with radius > 0 and a conic gradient: {nx} in x, {ny} in y, {nxy} in both, {n} in all")
        if kind == "frustum_edge":
            assert nx >= 20 and ny >= 20 and nxy >= 1, (nx, ny, nxy)
        else:  # at 0.6 only the largest splats reach the frame from beyond 1.3 tan: fewer, on both axes still
            assert n >= 20 and nx >= 5 and ny >= 5, (n, nx, ny)
    if kind == "modifier":
        n = np.linalg.norm(c.scene.rotations, axis=1)
        assert n.min() < 0.85 and n.max() > 1.2 and c.scale_modifier != 1.0
    if kind == "sh_low_degree":
        for ch in range(3):
            cl = ((o["clamped"] >> ch) & 1).astype(bool)
            n_cl, n_un = int((cl & vis).sum()), int((~cl & vis).sum())
            print(f"{name}: channel {ch}: {n_cl} clamped, {n_un} unclamped of {int(vis.sum())} visible")
            assert n_cl >= 100 and n_un >= 100, (ch, n_cl, n_un)
        assert c.scene.sh.shape[1] == 16 and c.degree < 3
    if kind == "opaque":
        assert blend is not None
        pairs, gaussians = int(blend["capped"].sum()), int((blend["capped"] > 0).sum())
        print(f"{name}: {pairs} contributing pairs with opacity * G > 0.99, on {gaussians} Gaussians")
        assert pairs >= 100, pairs
    if kind == "coloured_bg":
        frac = float((o["final_T"] > 0.05).mean())
        print(f"{name}: final_T > 0.05 on {100 * frac:.1f} % of the pixels")
        assert frac > 0.10, frac
