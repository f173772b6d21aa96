"""Scene composition and the points capture on the GPU (csrc/compose.hip, relightable3dgaussian_amd/compose.py,
GaussianTrainState.set_transform, relight.render_points) against tests/compose_ref64.py within BARS = 4 x the
reference's own float32 distance (tests/golden/compose.npz), row by row, on the golden's own draws; the points
capture against the golden exactly. Measure, draws, floors: tests/compose_ref64.py."""
from __future__ import annotations

import os

import numpy as np
import pytest

from tests import activation_ref64 as a64
from tests import compose_ref64 as c64
from tests._helpers import tt

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu
F = np.float32


def make_state(c, groups=14):
    from relightable3dgaussian_amd.trainer import GaussianTrainState

    return GaussianTrainState.from_tensors({g: tt(c[g]) for g, _ in a64.groups_of(groups)}, use_pbr=groups == 14)


def npy(t):
    return t.detach().cpu().numpy()


def within(tag, key, got, ref):
    e = a64.row_err(got, ref)
    print(f"{tag} {key:16s} {e:.3e} (bar {c64.BARS[key]:.1e})")
    assert e <= c64.BARS[key], (tag, key, e)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "compose.npz"))


@pytest.fixture(scope="module")
def st_draws():
    """groups -> the set_transform draw (the golden's for the four moved groups, whatever `groups` is)."""
    return {g: c64.draw_set_transform_case(g) for g in (14, 7)}


# ---- 1, 2: set_transform -----------------------------------------------------------------------------------

@pytest.mark.parametrize("groups", [14, 7])
@pytest.mark.parametrize("P", [1, 63, 257])
@pytest.mark.parametrize("kind", c64.KINDS)
def test_set_transform_against_ref64(st_draws, kind, P, groups):
    import torch

    c = c64.first_rows(st_draws[groups], P)
    kw = c64.draw_kwargs(kind, 100 + c64.KINDS.index(kind))
    ref = c64.set_transform(c, **kw)
    st = make_state(c, groups)
    st.exp_avg.normal_()
    st.exp_avg_sq.uniform_()
    st.param[st.total():] = 7.0  # the padding behind total()
    before, m, v = st.param.clone(), st.exp_avg.clone(), st.exp_avg_sq.clone()
    # one argument on the device, one on the CPU, one a list: none is read back
    args = {}
    for i, (k, a) in enumerate(kw.items()):
        a = a.reshape(()) if a.size == 1 else a
        args[k] = tt(a) if i % 3 == 0 else torch.from_numpy(np.array(a)) if i % 3 == 1 else a.tolist()
    st.set_transform(**args)
    tag = f"{kind} P={P} g={groups}"
    for g in c64.MOVED:
        within(tag, f"st_{g}", npy(st.view(g)), ref[g])
    touched = {"center": {"xyz"}, "offset": {"xyz"}, "scale": {"xyz", "scaling"}, "rotation": {"xyz", "rotation", "normal"}}
    for g, _ in a64.groups_of(groups):
        if g not in touched.get(kind, set(c64.MOVED)):
            assert torch.equal(st.view(g), tt(c[g])), (tag, g)
    assert torch.equal(st.param[st.total():], before[st.total():])
    assert torch.equal(st.exp_avg, m) and torch.equal(st.exp_avg_sq, v)


@pytest.mark.parametrize("form", ["transform", "rotation"])
def test_identity_transform(st_draws, form):
    import torch

    c = st_draws[14]
    st = make_state(c)
    st.set_transform(transform=torch.eye(4)) if form == "transform" else st.set_transform(rotation=np.eye(3, dtype=F))
    for g, _ in a64.groups_of(14):
        if g != "scaling" or form == "rotation":
            assert torch.equal(st.view(g), tt(c[g])), g
    if form == "transform":  # through log(exp): close, not equal
        within("identity", "st_scaling", npy(st.view("scaling")), c["scaling"].astype(np.float64))
        assert not torch.equal(st.view("scaling"), tt(c["scaling"]))


def test_set_transform_refusals_and_empty():
    import torch

    c = a64.draw_case(0, 1, 14)
    st = make_state(c)
    st.set_transform(transform=torch.eye(4, device="cuda"))  # P == 0: nothing launched
    st = make_state(a64.draw_case(5, 1, 7), 7)
    with pytest.raises(Exception):
        st.set_transform(transform=torch.eye(4, dtype=torch.float64))
    with pytest.raises(Exception):
        st.set_transform(rotation=np.eye(4, dtype=F))
    before = st.param.clone()
    st.set_transform()  # nothing given: nothing changes
    assert torch.equal(st.param, before)


# ---- 3, 4, 5: compose_scene --------------------------------------------------------------------------------

FIELDS = ("xyz", "scaling", "rotation", "normal", "opacity", "base_color", "roughness", "metallic", "shs",
          "incidents", "visibility_dc", "visibility_rest", "symm_inv")
SHAPES = {"xyz": (3,), "scaling": (3,), "rotation": (4,), "normal": (3,), "opacity": (1,), "base_color": (3,),
          "roughness": (1,), "metallic": (1,), "shs": (16, 3), "incidents": (16, 3), "visibility_dc": (1, 1),
          "visibility_rest": (24, 1), "symm_inv": (6,)}


@pytest.mark.parametrize("transform", ["none", "eye"])
def test_compose_identity_equals_activate(transform):
    """P = 63, 1, 257: the second object starts at row 63, the third at 64."""
    import torch

    from relightable3dgaussian_amd.compose import compose_scene

    objs = c64.draw_scene(identity=True)
    states = [make_state(c) for c, _ in objs]
    before = [s.param.clone() for s in states]
    sc = compose_scene([(s, None if transform == "none" else torch.eye(4)) for s in states])
    assert sc.offsets == [0, 63, 64] and sc.P == 321
    acts = [s.activate(inverse_covariance=True) for s in states]
    for k in ("xyz", "scaling", "rotation", "normal", "opacity", "base_color", "roughness", "metallic", "shs",
              "symm_inv"):
        want = torch.cat([a[k].detach() for a in acts])
        got = getattr(sc, k)
        assert got.shape == want.shape == (321, *SHAPES[k]) and got.is_contiguous() and not got.requires_grad
        assert torch.equal(got, want), k
    assert sc.incidents.shape == (321, 16, 3) and not sc.incidents.any()
    assert sc.visibility_rest.shape == (321, 24, 1) and not sc.visibility_rest[:, 15:].any()
    assert torch.equal(sc.visibility_rest[:, :15], torch.cat([s.view("visibility_rest") for s in states]))
    assert torch.equal(sc.visibility_dc, torch.cat([s.view("visibility_dc") for s in states]))
    assert sc.visibility.shape == (321, 25, 1) and torch.equal(sc.visibility[:, 1:], sc.visibility_rest)
    for s, b in zip(states, before):
        assert torch.equal(s.param, b)


def test_compose_general_transforms():
    import torch

    from relightable3dgaussian_amd.compose import compose_scene

    objs = c64.draw_scene()
    states = [make_state(c) for c, _ in objs]
    before = [s.param.clone() for s in states]
    # the transforms as a device tensor, a CPU tensor and transform.json's 16 numbers
    given = [tt(objs[0][1]), torch.from_numpy(objs[1][1].copy()), objs[2][1].reshape(-1).tolist()]
    sc = compose_scene(list(zip(states, given)))
    ref = c64.compose(objs)
    for k in FIELDS:
        got = npy(getattr(sc, k))
        assert got.shape == ref[k].shape, k
        if k in c64.COPIES:
            np.testing.assert_array_equal(got, ref[k].astype(F), err_msg=k)
        else:
            within("scene", k, got, ref[k])
    for s, b in zip(states, before):
        assert torch.equal(s.param, b)
    # the same device functions as set_transform followed by activate
    acts = []
    for s, (_, T) in zip(states, objs):
        s.set_transform(transform=tt(T))
        acts.append(s.activate(inverse_covariance=True))
    for k in ("xyz", "rotation", "normal", "opacity", "base_color", "roughness", "metallic", "shs"):
        assert torch.equal(getattr(sc, k), torch.cat([a[k].detach() for a in acts])), k


def test_compose_refusals_and_empty():
    import torch

    from relightable3dgaussian_amd.compose import compose_scene
    from relightable3dgaussian_amd.trainer import GaussianTrainState

    objs = c64.draw_scene()
    a, b = make_state(objs[0][0]), make_state(objs[2][0])
    empty = make_state(a64.draw_case(0, 3, 14))
    sc = compose_scene([(a, objs[0][1]), (empty, objs[1][1]), (b, None)], inverse_covariance=False)
    assert sc.symm_inv is None and sc.offsets == [0, 63, 63] and sc.P == 320
    two = compose_scene([(a, objs[0][1]), (b, None)], inverse_covariance=False)
    for k in FIELDS[:-1]:
        assert torch.equal(getattr(sc, k), getattr(two, k)), k
    with pytest.raises(ValueError):
        compose_scene([(a, None), (make_state(a64.draw_case(5, 1, 7), 7), None)])
    cpu = GaussianTrainState.from_tensors({g: torch.from_numpy(objs[1][0][g]) for g, _ in a64.groups_of(14)})
    with pytest.raises(Exception):
        compose_scene([(cpu, None)])
    from relightable3dgaussian_amd import _C
    from relightable3dgaussian_amd.activation import role_groups

    slots = [getattr(two, k) for k in FIELDS]
    with pytest.raises(Exception):  # fewer rows than row + P
        _C.compose_object(a.P, a.widths(), a.roles(), role_groups(a), a.param, None, 0, slots, two.P - a.P + 1)
    with pytest.raises(Exception):  # a CPU output
        _C.compose_object(a.P, a.widths(), a.roles(), role_groups(a), a.param, None, 0,
                          [two.xyz.cpu()] + slots[1:], 0)


def test_load_scene_from_ply_files(tmp_path):
    """transform.json's form: PLY paths and 16 numbers per object."""
    import torch

    from relightable3dgaussian_amd.compose import compose_scene, load_scene

    objs = c64.draw_scene()[:2]
    states = [make_state(c) for c, _ in objs]
    scene = {}
    for i, (st, (_, T)) in enumerate(zip(states, objs)):
        st.save_ply(str(tmp_path / f"o{i}.ply"))
        scene[f"o{i}"] = {"path": str(tmp_path / f"o{i}.ply"), "transform": T.reshape(-1).tolist()}
    got = load_scene(scene, inverse_covariance=True)
    want = compose_scene([(st, T) for st, (_, T) in zip(states, objs)])
    assert got.offsets == want.offsets == [0, 63] and got.P == 64
    for k in FIELDS:
        assert torch.equal(getattr(got, k), getattr(want, k)), k


# ---- 6: the call site --------------------------------------------------------------------------------------

class _ShLight:
    def __init__(self, shs):
        self.get_env_shs = shs


def test_composed_scene_feeds_the_relighting_calls():
    import torch

    from relightable3dgaussian_amd.bvh import RayTracer
    from relightable3dgaussian_amd.compose import compose_scene
    from relightable3dgaussian_amd.relight import render_equation_relight
    from relightable3dgaussian_amd.visibility import precompute_visibility

    Ns = 8
    objs = [(a64.draw_case(64, 91 + i, 14), T) for i, T in enumerate([None, np.eye(4, dtype=F)])]
    for c, _ in objs:
        c.pop("rotation_fwd")
        c["scaling"] = np.clip(c["scaling"], -4, -1)  # Gaussians of a size that rays can hit and miss
    objs[1][1][:3, 3] = [0.5, 0.25, -1.0]
    sc = compose_scene([(make_state(c), T) for c, T in objs])
    ref = {k: tt(v.astype(F)) for k, v in c64.compose(objs).items()}
    ref["visibility"] = torch.cat((ref["visibility_dc"], ref["visibility_rest"]), 1)
    campos = tt(a64.CAMPOS)
    light = _ShLight(tt(np.random.default_rng(5).normal(0, 0.3, (1, 16, 3)).astype(F)))

    def run(s):
        get = (lambda k: getattr(s, k)) if not isinstance(s, dict) else s.__getitem__
        rt = RayTracer(get("xyz"), get("scaling"), get("rotation"))
        vis = precompute_visibility(rt, get("xyz"), get("symm_inv"), get("opacity")[:, 0], get("normal"), Ns)
        viewdirs = torch.nn.functional.normalize(campos - get("xyz"), dim=-1)
        feats = render_equation_relight(get("base_color"), get("roughness"), get("metallic"), get("normal"), viewdirs,
                                        get("incidents"), light, get("visibility"), Ns, False, vis)[2]
        rows = [get(k) for k in ("base_color", "roughness", "metallic", "normal", "incidents", "visibility")]
        return feats, [r.reshape(r.shape[0], -1) for r in rows + [viewdirs, vis]]

    got, rows_a = run(sc)
    want, rows_b = run(ref)
    assert got.shape == (128, 21) and torch.isfinite(got).all()
    # the render equation is a function of a Gaussian's own row of these arrays
    same = torch.stack([(a == b).all(1) for a, b in zip(rows_a, rows_b)]).all(0)
    print("rows with bit-equal inputs:", int(same.sum()), "of 128")
    assert same.any()
    assert torch.equal(got[same], want[same])

    # Few rows qualify above (float32 activations rarely equal the rounded float64 ones in every component), so
    # EVERY row is also held, exactly, against the same calls fed from each state's own activate(): with no
    # transform and with a pure translation (s = 1, R = I, q_T = (1, 0, 0, 0)) the composed arrays are activate's
    # bit for bit, xyz moved by one rounded addition per component, which torch's add reproduces.
    states = [make_state(c) for c, _ in objs]
    acts = [s.activate(inverse_covariance=True) for s in states]
    alt = {k: torch.cat([a[k].detach() for a in acts]) for k in ("xyz", "scaling", "rotation", "normal", "opacity",
                                                                  "base_color", "roughness", "metallic", "symm_inv")}
    alt["xyz"][64:] += tt(objs[1][1][:3, 3])
    alt["incidents"] = torch.zeros(128, 16, 3, device="cuda")
    rest = torch.cat([s.view("visibility_rest") for s in states])
    alt["visibility"] = torch.cat([torch.cat([s.view("visibility_dc") for s in states]), rest,
                                   torch.zeros(128, 9, 1, device="cuda")], 1)
    for k in ("xyz", "scaling", "rotation", "normal", "symm_inv"):
        assert torch.equal(alt[k], getattr(sc, k)), k
    other, _ = run(alt)
    assert torch.equal(got, other)


# ---- 7, 8: render_points -------------------------------------------------------------------------------------

def test_render_points_against_golden(golden):
    import torch

    from relightable3dgaussian_amd.relight import render_points

    a = [tt(golden[f"pt_{k}"]) for k in ("xyz", "color", "view", "K")]
    rgb, depth = render_points(*a, c64.PT_H, c64.PT_W, tt(golden["pt_bg"]), return_depth=True)
    assert rgb.shape == (3, c64.PT_H, c64.PT_W) and depth.shape == (c64.PT_H, c64.PT_W)
    np.testing.assert_array_equal(npy(rgb), golden["pt_out_rgb"])
    # the depth of the float32 restatement (same operations in the same order, no contraction)
    _, depth32, winner = c64.render_points(*[golden[f"pt_{k}"] for k in ("xyz", "color", "view", "K")], c64.PT_H,
                                           c64.PT_W, golden["pt_bg"], dtype=np.float32)
    np.testing.assert_array_equal(npy(depth), depth32)
    assert (winner < 0).any() and (npy(depth)[winner < 0] == 10000).all()
    again = render_points(*a, c64.PT_H, c64.PT_W, tt(golden["pt_bg"]))
    assert torch.equal(again, rgb)


def test_render_points_specification():
    import torch

    from relightable3dgaussian_amd.relight import render_points

    view, K = np.eye(4, dtype=F), np.array([[2, 0, 1], [0, 2, 1], [0, 0, 1]], F)
    xyz = np.array([[0, 0, 2], [0.25, 0.25, 2], [0, 0, 0], [-0.25, 0, 1], [0, 0, 10000], [1, 0, 4]], F)
    color = np.arange(18, dtype=F).reshape(6, 3)
    ref_rgb, ref_depth, _ = c64.render_points(xyz, color, view, K, 2, 2, 0.5)
    for order in (np.arange(6), np.arange(6)[::-1].copy()):
        # reversed: the tie at z = 2 goes to the other point, the lower index of that order
        rgb, depth = render_points(tt(xyz[order]), tt(color[order]), tt(view), tt(K), 2, 2, 0.5, return_depth=True)
        want_rgb, want_depth, winner = c64.render_points(xyz[order], color[order], view, K, 2, 2, 0.5)
        np.testing.assert_array_equal(npy(rgb), want_rgb)
        np.testing.assert_array_equal(npy(depth), want_depth.astype(F))
        assert winner[1, 1] == min(np.flatnonzero(order == 0)[0], np.flatnonzero(order == 1)[0])
    np.testing.assert_array_equal(ref_depth, [[10000, 10000], [1, 2]])
    # P == 0: the background; bg as [3]
    rgb, depth = render_points(tt(xyz[:0]), tt(color[:0]), tt(view), tt(K), 3, 5, [0.1, 0.2, 0.3], return_depth=True)
    assert torch.equal(rgb, tt(np.array([0.1, 0.2, 0.3], F))[:, None, None].expand(3, 3, 5))
    assert (depth == 10000).all()
    # H = W = 1: points 0, 1 (z = 2) and 3 (u = 0.5, z = 1) fall into the one pixel
    K1 = np.array([[2, 0, 0], [0, 2, 0], [0, 0, 1]], F)
    rgb, depth = render_points(tt(xyz), tt(color), tt(view), tt(K1), 1, 1, 0.0, return_depth=True)
    want_rgb, want_depth, _ = c64.render_points(xyz, color, view, K1, 1, 1, 0.0)
    np.testing.assert_array_equal(npy(rgb), want_rgb)
    np.testing.assert_array_equal(npy(depth), want_depth.astype(F))
    # refusals
    with pytest.raises(Exception):
        render_points(torch.from_numpy(xyz), torch.from_numpy(color), tt(view), tt(K), 2, 2, 0.5)
    with pytest.raises(Exception):
        render_points(tt(xyz).double(), tt(color), tt(view), tt(K), 2, 2, 0.5)
    with pytest.raises(Exception):
        render_points(tt(xyz), tt(color[:5]), tt(view), tt(K), 2, 2, 0.5)


def test_render_points_is_reproducible(golden):
    """Many points per pixel (4096 into 4 x 4) in two runs: bit-identical colour and depth."""
    import torch

    from relightable3dgaussian_amd.relight import render_points

    a = [tt(golden[f"pt_{k}"]) for k in ("xyz", "color", "view")]
    K = tt(golden["pt_K"] * np.array([[0.07], [0.1], [1]], F))
    runs = [render_points(*a, K, 4, 4, 0.0, return_depth=True) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert (runs[0][1] < 10000).any()
