"""CPU checks of the scene-composition references: tests/golden/compose.npz (the reference's own float32 torch
code) against tests/compose_ref64.py within FLOORS, the archive's byte-for-byte regeneration, the conditions that
make the points-capture case exact, and the C entry points' argument refusals (no device work, so no GPU).

`test_archive_regenerates_byte_for_byte` runs the reference's own code, so it runs where the golden files are
made: on a development machine that has the reference checkout (at make_golden_compose.DEFAULT_REFERENCE, or
where R3DG_REFERENCE points; a value that is no directory fails). A machine without the checkout, such as a GPU
test machine, skips that one test; `test_archive_bytes_depend_on_the_arrays_only` runs everywhere."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

from tests import activation_ref64 as a64
from tests import compose_ref64 as c64

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_compose as mgc  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "compose.npz")
LIB = os.path.join(ROOT, "relightable3dgaussian_amd", "lib", "libr3dg_hip.so")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_inputs_are_the_seeded_draws(golden):
    c = c64.draw_set_transform_case()
    for g in c64.MOVED:
        np.testing.assert_array_equal(golden[f"st_{g}"], c[g])
    for i, kind in enumerate(c64.KINDS):
        kw = c64.draw_kwargs(kind, 100 + i)
        got = mgc.set_transform_kwargs(golden, kind)
        assert set(got) == set(kw)
        for k in kw:
            np.testing.assert_array_equal(got[k], kw[k])
    for (c, T), (gc, gT) in zip(c64.draw_scene(), mgc.scene_objects(golden)):
        np.testing.assert_array_equal(gT, T)
        for k in mgc.SCENE_INPUTS:
            np.testing.assert_array_equal(gc[k], c[k])
    for k, v in c64.draw_points_case().items():
        np.testing.assert_array_equal(golden[f"pt_{k}"], v)


def test_transforms_meet_the_quaternion_condition(golden):
    """1 + trace(R) >= 0.5 for every rotation part, and the full transforms have three different row norms."""
    mats = [mgc.set_transform_kwargs(golden, k) for k in c64.KINDS]
    mats = [kw["transform"][:3, :3] if "transform" in kw else kw.get("rotation") for kw in mats]
    mats += [T[:3, :3] for _, T in mgc.scene_objects(golden)]
    seen = 0
    for A in mats:
        if A is None:
            continue
        A = A.astype(np.float64)
        s = np.sqrt((A * A).sum(1))
        assert 1 + np.trace(A / s[:, None]) >= 0.5
        seen += 1
    assert seen == 6
    s = np.sqrt((golden["st_transform_kw_transform"][:3, :3].astype(np.float64) ** 2).sum(1))
    assert np.all(np.abs(np.diff(np.sort(s))) > 0.1) and np.any(golden["st_transform_kw_transform"][:3, 3] != 0)


def test_golden_within_floors(golden):
    worst = mgc.measure(golden)
    assert set(worst) == set(c64.FLOORS)
    for k, v in worst.items():
        assert v <= c64.FLOORS[k], k


def test_floors_are_the_measured_ones(golden):
    """FLOORS = the measured distances rounded UP to two digits; BARS = 4 x FLOORS."""
    for k, v in mgc.measure(golden).items():
        assert v <= c64.FLOORS[k], k
        assert c64.FLOORS[k] <= v * 1.1 + 1e-300 or v == 0.0 == c64.FLOORS[k], (k, v, c64.FLOORS[k])
    assert all(abs(c64.BARS[k] - 4 * c64.FLOORS[k]) <= 1e-12 * c64.FLOORS[k] for k in c64.FLOORS)


def test_copies_and_zeros_are_exact(golden):
    ref = c64.compose(mgc.scene_objects(golden))
    for k in c64.COPIES:
        np.testing.assert_array_equal(golden[f"sc_out_{k}"], ref[k])
    assert not golden["sc_out_incidents"].any() and not golden["sc_out_visibility_rest"][:, 15:].any()
    assert golden["sc_out_visibility_rest"].shape[1:] == (24, 1) and golden["sc_out_shs"].shape[1:] == (16, 3)


def test_untouched_groups_of_a_partial_transform(golden):
    """center / scale / offset alone leave rotation and normal as they were; only scale and the full transform
    change the raw scaling."""
    for kind in ("center", "scale", "offset"):
        for g in ("rotation", "normal"):
            np.testing.assert_array_equal(golden[f"st_{kind}_{g}"], golden[f"st_{g}"])
    for kind in ("center", "rotation", "offset"):
        np.testing.assert_array_equal(golden[f"st_{kind}_scaling"], golden["st_scaling"])


def _digest(path) -> str:
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def test_archive_bytes_depend_on_the_arrays_only(golden, tmp_path):
    out = tmp_path / "compose.npz"
    mgc.write_npz(str(out), {k: golden[k] for k in golden.files})
    assert _digest(out) == _digest(GOLDEN)


def test_archive_regenerates_byte_for_byte(tmp_path):
    """Runs the reference's code again; needs the reference checkout (make_golden_compose.py --reference)."""
    given = os.environ.get("R3DG_REFERENCE")
    if given is not None and not os.path.isdir(given):
        pytest.fail(f"R3DG_REFERENCE={given} is not a directory")
    ref = given or mgc.DEFAULT_REFERENCE
    if not os.path.isdir(ref):
        pytest.skip("no reference checkout to regenerate from")
    out = tmp_path / "compose.npz"
    mgc.write_npz(str(out), mgc.generate(ref))
    assert _digest(out) == _digest(GOLDEN)


# ---- the points capture ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def points(golden):
    pt = {k: golden[f"pt_{k}"] for k in ("xyz", "color", "view", "K", "bg")}
    u, v, z = c64.project(pt["xyz"], pt["view"], pt["K"])
    rgb, depth, winner = c64.render_points(pt["xyz"], pt["color"], pt["view"], pt["K"], c64.PT_H, c64.PT_W, pt["bg"])
    return dict(pt, u=u, v=v, z=z, rgb=rgb, depth=depth, winner=winner)


def test_points_case_is_decided_far_from_every_edge(points):
    """Every one of the 4096 points: u and v at least 0.05 px from an integer, and the depths of the candidates
    of one pixel at least 1e-3 apart, relative; no depth within 1e-3 relative of 10000."""
    u, v, z = points["u"], points["v"], points["z"]
    assert len(u) == c64.PT_P and np.all(np.isfinite(u)) and np.all(np.isfinite(v))
    for a in (u, v):
        assert np.all(np.abs(a - np.rint(a)) >= 0.05)
    assert np.all(np.abs(z - c64.FAR) >= 1e-3 * c64.FAR)
    H, W = c64.PT_H, c64.PT_W
    tu, tv = np.trunc(u), np.trunc(v)
    inside = (tu >= 0) & (tu < W) & (tv >= 0) & (tv < H)
    pix = (tv * W + tu)[inside].astype(np.int64)
    zi = z[inside]
    order = np.lexsort((zi, pix))
    same = pix[order][1:] == pix[order][:-1]
    gap = np.diff(zi[order])[same] / np.maximum(np.abs(zi[order][1:]), np.abs(zi[order][:-1]))[same]
    assert same.sum() > 1000 and np.all(gap >= 1e-3)


def test_points_case_holds_every_situation(points):
    u, v, z, winner = points["u"], points["v"], points["z"], points["winner"]
    H, W = c64.PT_H, c64.PT_W
    G = {k: slice(*r) for k, r in c64.POINT_GROUPS.items()}
    assert np.all(np.trunc(u[G["deep"]]) == 20) and np.all(np.trunc(v[G["deep"]]) == 11)
    assert winner[11, 20] in range(*c64.POINT_GROUPS["deep"]) or z[winner[11, 20]] < z[G["deep"]].min()
    off = np.stack([u[G["off"]], v[G["off"]]], 1)
    assert np.any(off[:, 0] < -1) and np.any(off[:, 0] >= W) and np.any(off[:, 1] < -1) and np.any(off[:, 1] >= H)
    assert not np.isin(np.arange(*c64.POINT_GROUPS["off"]), winner).any()
    assert np.all((u[G["neg_u"]] > -1) & (u[G["neg_u"]] < 0)) and np.all((v[G["neg_v"]] > -1) & (v[G["neg_v"]] < 0))
    # the (-1, 0) points land in column / row 0: the neg_v group shares one pixel of a column that no other
    # group reaches, so its nearest point shows there
    assert winner[0, W - 2] == 296 + int(np.argmin(z[G["neg_v"]]))
    assert np.isin(np.arange(*c64.POINT_GROUPS["neg_u"]), winner[:, 0]).any()
    assert np.all(z[G["behind"]] < 0) and np.isin(np.arange(*c64.POINT_GROUPS["behind"]), winner).any()
    assert np.all(z[G["far"]] >= c64.FAR) and not np.isin(np.arange(*c64.POINT_GROUPS["far"]), winner).any()
    assert (winner < 0).sum() > 0


def test_points_golden_is_the_defined_result(golden, points):
    """The reference's converged loop == the definition, in float64 and in float32 arithmetic alike."""
    np.testing.assert_array_equal(golden["pt_out_rgb"], points["rgb"])
    rgb32, depth32, winner32 = c64.render_points(points["xyz"], points["color"], points["view"], points["K"],
                                                 c64.PT_H, c64.PT_W, points["bg"], dtype=np.float32)
    np.testing.assert_array_equal(winner32, points["winner"])
    np.testing.assert_array_equal(rgb32, points["rgb"])
    empty = points["winner"] < 0
    assert np.all(golden["pt_out_rgb"][:, empty] == points["bg"][:, None])


def test_points_definition_on_small_cases():
    """The tie rule, the z == 0 drop, truncation toward zero and the strict far test, on exact numbers."""
    view, K = np.eye(4, dtype=np.float32), np.array([[2, 0, 1], [0, 2, 1], [0, 0, 1]], np.float32)
    xyz = np.array([[0, 0, 2], [0.25, 0.25, 2], [0, 0, 0], [-0.25, 0, 1], [0, 0, 10000], [1, 0, 4]], np.float32)
    color = np.arange(18, dtype=np.float32).reshape(6, 3)
    rgb, depth, winner = c64.render_points(xyz, color, view, K, 2, 2, 0.5)
    # points 0 and 1 share pixel (1, 1) at z = 2: index 0 wins; point 2 has z == 0; point 3 has u = 0.5 -> (0, 1)
    # with z = 1; point 4 is not nearer than 10000; point 5: u = 1.5, v = 1 -> (1, 1) at z = 4, loses
    assert winner.tolist() == [[-1, -1], [3, 0]]
    assert depth.tolist() == [[10000, 10000], [1, 2]] and rgb[:, 0, 0].tolist() == [0.5, 0.5, 0.5]


# ---- the C entry points refuse bad arguments before any device work ---------------------------------------

@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (loads the HIP runtime before the library)

    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m relightable3dgaussian_amd.build")
    return C.CDLL(LIB)


class _Layout(C.Structure):
    _fields_ = [("P", C.c_int), ("n_groups", C.c_int), ("width", C.c_int * 16), ("xyz", C.c_int),
                ("scaling", C.c_int), ("rotation", C.c_int), ("opacity", C.c_int)]


def test_c_entry_points_refuse(lib):
    lib.r3dg_last_error.restype = C.c_char_p
    L = _Layout(P=0, n_groups=7, xyz=0, scaling=3, rotation=2, opacity=4)
    for i, w in enumerate([3, 3, 4, 3, 1, 3, 45]):
        L.width[i] = w
    call = lambda normal, flags, xf=None: lib.r3dg_set_transform(C.byref(L), normal, None, xf, flags, None)  # noqa: E731
    assert call(1, 0) == 0                       # P == 0: nothing to do
    assert call(0, 0) != 0 and b"twice" in lib.r3dg_last_error()
    assert call(4, 0) != 0 and b"width" in lib.r3dg_last_error()
    assert call(1, 64) != 0 and b"flags" in lib.r3dg_last_error()
    assert call(1, 1 | 2) != 0 and b"excludes" in lib.r3dg_last_error()
    assert call(1, 1) != 0 and b"19 floats" in lib.r3dg_last_error()
    lib.r3dg_render_points.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 7
    assert lib.r3dg_render_points(0, None, None, None, None, 4, 4, None, None, None, None, None, None, None) != 0
    assert b"null argument" in lib.r3dg_last_error()
    assert lib.r3dg_render_points(0, None, None, None, None, 0, 4, None, None, None, None, None, None, None) != 0
    assert b"bad P, H or W" in lib.r3dg_last_error()
