"""The parameter activations on the GPU (csrc/activation.hip, relightable3dgaussian_amd/activation.py,
GaussianTrainState.activate) against tests/activation_ref64.py within BARS = 4 x the reference's own float32
distance (tests/golden/activation.npz), row by row. Measure, draw, floors: tests/activation_ref64.py."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from tests import activation_ref64 as a64
from tests._helpers import tt

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_activation as mga  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SH_GROUPS = {g for pair in a64.SH.values() for g in pair}


def make_state(c, groups, rotation="rotation"):
    from relightable3dgaussian_amd.trainer import GaussianTrainState

    t = {g: tt(c[rotation if g == "rotation" else g]) for g, _ in a64.groups_of(groups)}
    return GaussianTrainState.from_tensors(t, use_pbr=groups == 14)


def activate(st, campos=True, symm=False, accumulate=False):
    return st.activate(campos=tt(a64.CAMPOS) if campos else None, inverse_covariance=symm, accumulate=accumulate)


def backward(out, ups):
    """loss = sum <out, upstream>; a missing upstream leaves the output out of the loss."""
    loss = sum((out[k] * tt(u)).sum() for k, u in ups.items())
    loss.backward()


def grads_of(st, groups):
    return {g: st.grad_view(g).cpu().numpy() for g, _ in a64.groups_of(groups)}


def check(tag, got: dict, ref: dict, prefix=""):
    """Every entry of ref within its bar; the SH copies exactly."""
    for k, r in ref.items():
        if k == "xyz" and not prefix:
            continue
        g = got[k].detach().cpu().numpy() if hasattr(got[k], "detach") else got[k]
        if k in a64.SH or k in SH_GROUPS:
            np.testing.assert_array_equal(g, r.astype(F), err_msg=f"{tag} {prefix}{k}")
            continue
        e = a64.row_err(g, r)
        print(f"{tag} {prefix}{k:12s} {e:.3e} (bar {a64.BARS[prefix + k]:.1e})")
        assert e <= a64.BARS[prefix + k], (tag, prefix + k, e)


def check_sigmoid_grads(tag, got, gref):
    """The sigmoid gradients once more, against a bar that does not come from the draw. BARS' sigmoid
    gradients are loose (grad_opacity is 4: tests/activation_ref64.py) because the reference's float32
    autograd forms 1 - s, which cancels. The kernel evaluates the slope as t / (1 + t)^2, t = expf(-|x|), with
    no cancellation; in units of 2^-24 relative: t 2 (expf within an ulp), d = 1 + t 2, d * d 5, the quotient
    2 + 5 + 1, the product with g 1 more = 9; the bar is 16 units (about 1e-6), row_err's 1e-37 covering a
    flushed t at |x| = 100."""
    for k in a64.SIGMOIDS:
        if k in got:
            e = a64.row_err(got[k], gref[k])
            assert e <= 16 * 2.0 ** -24, (tag, k, e)


def run_case(tag, c, ups, groups, campos, symm):
    """Forward on rotation_fwd, backward on rotation, both against ref64; returns the gradient state."""
    cam = a64.CAMPOS if campos else None
    st = make_state(c, groups, "rotation_fwd")
    out = activate(st, campos, symm)
    ref = a64.forward(c, cam, inverse_covariance=symm, rotation="rotation_fwd")
    assert set(out) == set(ref), (sorted(out), sorted(ref))
    for k, r in ref.items():
        assert tuple(out[k].shape) == r.shape, (k, out[k].shape)
    assert out["xyz"].data_ptr() == st.view("xyz").data_ptr()
    check(tag, out, ref)

    st = make_state(c, groups)
    st.grad.fill_(float("nan"))  # overwrite mode writes every element of [0, total) and nothing else
    out = activate(st, campos, symm)
    backward(out, ups)
    total = st.total()
    g = st.grad.cpu().numpy()
    assert not np.isnan(g[:total]).any(), tag
    # the capacity padding behind the parameters is untouched. It exists where total is no multiple of 4 (odd
    # P, and P = 2 mod 4 in the 14-group layout, whose rows are 131 floats); for the other shapes the slice is empty and nothing is checked
    assert g.size - total == (-total) % 4
    assert np.isnan(g[total:]).all(), tag
    got, gref = grads_of(st, groups), a64.backward(c, ups, cam)
    check(tag, got, gref, "grad_")
    check_sigmoid_grads(tag, got, gref)
    return st


# ---- golden cases ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "activation.npz"))


@pytest.mark.parametrize("name", sorted(mga.CASES))
def test_golden_cases(hip_ext, golden, name):
    kw = mga.CASES[name]
    c, ups, campos = mga.case_inputs(golden, name)
    run_case(name, c, ups, kw["groups"], kw["campos"], True)


# ---- alignment and tail shapes ----------------------------------------------------------------------------

@pytest.mark.parametrize("groups", [7, 14])
@pytest.mark.parametrize("P", [1, 2, 3, 63, 64, 65, 255, 257, 1025])
def test_alignment_and_tails(hip_ext, P, groups):
    """Group g starts at float P * sum(width[<g]): for odd P every block behind the first is misaligned, for
    P = 2 mod 4 every second one; P % 4 != 0 leaves a tail lane; P = 1025 crosses a workgroup in both launches
    (1024 Gaussians per 256 lanes of four; 16 and 48 rows per SH workgroup)."""
    c = a64.draw_case(P, 100 + P, groups)
    for campos in (True, False):
        ups = a64.draw_upstreams(P, 200 + P, groups, campos)
        for symm in (True, False):
            run_case(f"P={P} g={groups} cam={int(campos)} inv={int(symm)}", c, ups, groups, campos, symm)


@pytest.mark.parametrize("groups", [7, 14])
def test_no_gaussians(hip_ext, groups):
    import torch

    c = a64.draw_case(0, 1, groups)
    st = make_state(c, groups)
    out = activate(st, True, True)
    ref = a64.forward(c, a64.CAMPOS, inverse_covariance=True)
    assert set(out) == set(ref)
    for k, r in ref.items():
        assert tuple(out[k].shape) == r.shape and out[k].dtype == torch.float32, k
    backward(out, a64.draw_upstreams(0, 2, groups, True))
    assert float(st.grad.abs().sum()) == 0.0


# ---- modes ------------------------------------------------------------------------------------------------

def test_accumulate_sums_two_backwards(hip_ext):
    """The second upstream of row p is the first times a positive factor a_p of its own. Every group's
    gradient of row p is linear in row p's upstreams, so the two float32 addends of every element have one
    sign, and their float32 sum is as close to the exact sum as the addends are to theirs (plus 2^-24).
    Two independent draws would cancel in some rows: the buffer then holds the rounding of each addend
    against a small sum, which no float32 accumulation can avoid (2.8e-6 seen on grad_scaling, bar 3.5e-7)."""
    P, groups = 257, 14
    c = a64.draw_case(P, 7, groups)
    u1 = a64.draw_upstreams(P, 8, groups, True)
    a = np.random.default_rng(9).uniform(0.25, 2.0, P).astype(F)
    u2 = {k: v * a.reshape(P, *([1] * (v.ndim - 1))) for k, v in u1.items()}
    del u2["normal"], u2["incidents"]  # a missing upstream adds nothing
    st = make_state(c, groups)
    backward(activate(st), u1)                   # overwrite
    backward(activate(st, accumulate=True), u2)  # add
    g1, g2 = a64.backward(c, u1, a64.CAMPOS), a64.backward(c, u2, a64.CAMPOS)
    got = grads_of(st, groups)
    for k in g1:
        if k in SH_GROUPS:  # float32 sums of two float32 values: exact
            want = g1[k].astype(F) + g2[k].astype(F)
            np.testing.assert_array_equal(got[k], want, err_msg=k)
        else:
            e = a64.row_err(got[k], g1[k] + g2[k])
            print(f"accumulate grad_{k:12s} {e:.3e}")
            assert e <= a64.BARS["grad_" + k], k


def test_accumulate_independent_upstreams_is_the_float32_sum(hip_ext):
    """Two independent upstream draws, every output in both. Accumulate mode computes the second gradient
    with the instructions of overwrite mode and adds it to what is there, so the buffer must hold, bit for
    bit, the float32 sum of the two gradients computed separately in overwrite mode (each of which the
    other tests hold against ref64). Rows where the two cancel are in."""
    P, groups = 257, 14
    c = a64.draw_case(P, 7, groups)
    u1, u2 = a64.draw_upstreams(P, 8, groups, True), a64.draw_upstreams(P, 21, groups, True)
    st = make_state(c, groups)
    total = st.total()
    backward(activate(st), u2)
    g2 = st.grad[:total].cpu().numpy()
    backward(activate(st), u1)
    g1 = st.grad[:total].cpu().numpy()
    assert not np.array_equal(g1, g2)
    backward(activate(st, accumulate=True), u2)
    np.testing.assert_array_equal(st.grad[:total].cpu().numpy(), g1 + g2)


def test_missing_upstreams_are_exact_zeros(hip_ext):
    P, groups = 65, 14
    c = a64.draw_case(P, 11, groups)
    st = make_state(c, groups)
    st.grad.fill_(float("nan"))
    out = activate(st, True, True)
    assert not out["symm_inv"].requires_grad and out["symm_inv"].grad_fn is None
    assert all(v.requires_grad for k, v in out.items() if k != "symm_inv")
    backward(out, {"opacity": a64.draw_upstreams(P, 12, groups)["opacity"]})
    got = grads_of(st, groups)
    for k, v in got.items():
        if k != "opacity":
            assert np.all(v == 0), k
    assert np.abs(got["opacity"]).max() > 0


def test_no_grad_runs_the_forward_only(hip_ext):
    import torch

    st = make_state(a64.draw_case(65, 13, 14), 14)
    with torch.no_grad():
        out = activate(st, True, True)
    assert all(not v.requires_grad and v.grad_fn is None for v in out.values())
    assert not st.param.requires_grad and st.param.grad_fn is None


def test_cpu_tensors_and_other_dtypes_raise(hip_ext):
    import torch

    st = make_state(a64.draw_case(5, 14, 7), 7)
    lay = (st.P, st.widths(), st.roles(), [1, 5, 6] + [-1] * 7)
    with pytest.raises(Exception):
        hip_ext.activate_forward(*lay, st.param.cpu(), None, False)
    with pytest.raises(Exception):
        hip_ext.activate_forward(*lay, st.param.double(), None, False)
    ups = [None] * 12
    ups[4] = torch.zeros(5, 1)  # a CPU upstream
    with pytest.raises(Exception):
        hip_ext.activate_backward(*lay, st.param, None, ups, st.grad, False)
    ups[4] = torch.zeros(5, 1, device="cuda", dtype=torch.float64)
    with pytest.raises(Exception):
        hip_ext.activate_backward(*lay, st.param, None, ups, st.grad, False)


# ---- strided upstreams ------------------------------------------------------------------------------------

def test_strided_upstreams_are_bit_identical(hip_ext):
    """g_xyz, g_opacity, g_scaling, g_rotation as column blocks of one [P, 22] array (the dense array of
    rasterize_gaussians_backward_chunked_packed starts so) and the feature gradients as slices of one [P, 11]
    array, through `_C.activate_backward` itself: the same bits as the same values passed contiguously."""
    import torch

    from relightable3dgaussian_amd.activation import UPSTREAM_SLOTS, role_groups

    P, groups = 257, 14
    st = make_state(a64.draw_case(P, 15, groups), groups)
    rng = np.random.default_rng(16)
    dense, feat = tt(rng.normal(size=(P, 22)).astype(F)), tt(rng.normal(size=(P, 11)).astype(F))
    views = {"xyz": dense[:, 0:3], "opacity": dense[:, 3:4], "scaling": dense[:, 4:7], "rotation": dense[:, 7:11],
             "roughness": feat[:, 0:1], "metallic": feat[:, 1:2], "normal": feat[:, 5:8], "base_color": feat[:, 8:11]}
    assert not any(v.is_contiguous() for v in views.values())
    lay = (st.P, st.widths(), st.roles(), role_groups(st))
    res = []
    for make in (lambda v: v, lambda v: v.contiguous()):
        grad = torch.full_like(st.grad, float("nan"))
        hip_ext.activate_backward(*lay, st.param, None, [make(views[n]) if n in views else None for n in UPSTREAM_SLOTS],
                                  grad, False)
        res.append(grad[:st.total()].cpu().numpy())
    assert not np.isnan(res[0]).any()
    np.testing.assert_array_equal(res[0], res[1])
    assert np.abs(res[0]).max() > 0


# ---- branches ---------------------------------------------------------------------------------------------

def test_normal_opacity_and_quaternion_branches(hip_ext):
    P, groups = 257, 14
    c = a64.draw_case(P, 17, groups)
    c["rotation"][5] = 0.0  # a zero quaternion: a zero rotation row; its symm_inv row is 0 / 0, not asserted
    ups = a64.draw_upstreams(P, 18, groups, True)
    reg = a64.normal_regions(P)
    st = make_state(c, groups)
    out = activate(st, True, True)
    backward(out, ups)
    z = reg["zero"]
    assert np.all(c["normal"][z] == 0)
    normal, gn = out["normal"].detach().cpu().numpy(), st.grad_view("normal").cpu().numpy()
    np.testing.assert_array_equal(normal[z], 0.0)
    np.testing.assert_array_equal(gn[z], ups["normal"][z] / F(1e-3))
    ref, gref = a64.forward(c, a64.CAMPOS), a64.backward(c, ups, a64.CAMPOS)
    for name in ("below", "above"):
        r = reg[name]
        assert len(r) >= 10
        assert a64.row_err(normal[r], ref["normal"][r]) <= a64.BARS["normal"], name
        assert a64.row_err(gn[r], gref["normal"][r]) <= a64.BARS["grad_normal"], name
    np.testing.assert_array_equal(out["rotation"].detach().cpu().numpy()[5], 0.0)
    op, gop = out["opacity"].detach().cpu().numpy(), st.grad_view("opacity").cpu().numpy()
    np.testing.assert_array_equal(c["opacity"][:4, 0], [-100, 100, -20, 20])
    assert np.all(np.isfinite(op)) and op.min() >= 0 and op.max() <= 1
    assert np.all(np.abs(gop[:2]) <= 1e-37)
    assert np.all(np.isfinite(gop))


# ---- wiring through autograd ----------------------------------------------------------------------------

def scene_state(P=2000, seed=3):
    """synthetic.small_scene + brdf_inputs as the RAW parameters of a 14-group state."""
    from relightable3dgaussian_amd import synthetic

    scene, cam = synthetic.small_scene(P=P, S=11, seed=seed)
    b = synthetic.brdf_inputs(P, seed=seed + 1, S=16)
    logit = lambda x: np.log(x / (1 - x))  # noqa: E731
    rng = np.random.default_rng(seed + 2)
    c = {"xyz": scene.means3D, "normal": b["normals"] * rng.uniform(0.5, 2, (P, 1)),
         "rotation": scene.rotations * rng.uniform(0.5, 2, (P, 1)), "scaling": np.log(scene.scales),
         "opacity": logit(scene.opacity), "f_dc": scene.sh[:, :1], "f_rest": scene.sh[:, 1:],
         "base_color": logit(np.clip(b["base"], 0.02, 0.98)), "roughness": logit(np.clip(b["rough"], 0.02, 0.98)),
         "metallic": logit(np.clip(b["metal"], 0.02, 0.98)), "incidents_dc": b["incidents"][:, :1],
         "incidents_rest": b["incidents"][:, 1:], "visibility_dc": b["visibility"][:, :1],
         "visibility_rest": b["visibility"][:, 1:]}
    c = {k: np.ascontiguousarray(v, F) for k, v in c.items()}
    return c, cam, b["env"]


def test_training_step_through_autograd(hip_ext):
    """activate -> RenderEquation (training form) -> feature cat -> GaussianRasterizer -> a fixed linear
    functional -> backward: st.grad is the ref64 backward of the upstreams autograd delivered (retain_grad), so
    the activation and autograd's summing of the two paths into base_color, roughness, metallic and xyz hold;
    the rasterizer is not re-tested. Then one optimizer step from st.grad as it stands."""
    import types

    import torch

    from relightable3dgaussian_amd.r3dg_rasterization import GaussianRasterizer, RenderEquation, settings_from_camera

    c, cam, env = scene_state()
    P = c["xyz"].shape[0]
    st = make_state(c, 14)
    campos = tt(cam.campos)
    out = st.activate(campos=campos)
    for v in out.values():
        v.retain_grad()
    pbr, _, _ = RenderEquation(out["base_color"], out["roughness"], out["metallic"], out["normal"].detach(),
                               out["viewdirs"], out["incidents"], tt(env), out["visibility"], 4, True)
    features = torch.cat([out["roughness"], out["metallic"], pbr, out["normal"], out["base_color"]], dim=-1)
    means2D = torch.zeros_like(out["xyz"], requires_grad=True)
    res = GaussianRasterizer(settings_from_camera(cam, (1.0, 1.0, 1.0)))(
        means3D=out["xyz"], means2D=means2D, shs=out["shs"], colors_precomp=None, opacities=out["opacity"],
        scales=out["scaling"], rotations=out["rotation"], cov3D_precomp=None, features=features)
    gen = torch.Generator(device="cuda").manual_seed(5)
    loss = sum((res[i] * torch.randn(res[i].shape, device="cuda", generator=gen)).sum() for i in (2, 3, 6))
    st.grad.fill_(float("nan"))
    loss.backward()

    ups = {k: v.grad.cpu().numpy() for k, v in out.items() if v.grad is not None}
    for k in ("xyz", "viewdirs", "base_color", "roughness", "metallic", "scaling", "rotation", "opacity", "shs",
              "normal", "incidents", "visibility"):
        assert k in ups and np.abs(ups[k]).max() > 0, k
    gref = a64.backward(c, ups, cam.campos)
    assert not np.isnan(st.grad[:st.total()].cpu().numpy()).any()
    check("wiring", grads_of(st, 14), gref, "grad_")
    st.add_densification_stats(means2D.grad, res[-1], normal_grad=st.grad_view("normal"))
    assert float(st.normal_gradient_accum.abs().sum()) > 0

    before = st.param[:st.total()].clone()
    st.training_setup(types.SimpleNamespace(
        percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
        position_lr_max_steps=30000, normal_lr=0.01, rotation_lr=0.001, scaling_lr=0.005, opacity_lr=0.05,
        sh_lr=0.0025, base_color_lr=0.01, roughness_lr=0.01, metallic_lr=0.01, light_lr=0.002, light_rest_lr=-1.0,
        visibility_lr=0.0025, visibility_rest_lr=-1.0))
    kept = st.grad.clone()
    st.step(zero_grad=False)
    assert torch.equal(st.grad[:st.total()], kept[:st.total()])
    moved = (st.param[:st.total()] != before)
    for g, _ in a64.groups_of(14):
        assert bool(st._view(moved, g).any()), g
    assert bool(torch.isfinite(st.param).all())
    assert P == st.P


def test_after_densification(hip_ext):
    """`activate` keeps nothing of the state: after densify_and_prune has changed P and replaced the buffers,
    the next call follows the new ones."""
    import torch

    c, cam, _ = scene_state(P=1000, seed=9)
    st = make_state(c, 14)
    st.percent_dense = 0.01
    P0 = st.P
    out = activate(st, True, True)
    assert out["scaling"].shape[0] == P0
    st.xyz_gradient_accum[::3] = 1.0  # every third Gaussian over the gradient threshold: cloned or split
    st.denom.fill_(1.0)
    st.densify_and_prune(0.5, 0.3, 1.0, None, 10.0)
    assert st.P != P0
    groups = a64.groups_of(14)
    cn = {g: st.view(g).cpu().numpy().copy() for g, _ in groups}
    ups = a64.draw_upstreams(st.P, 19, 14, True)
    out = activate(st, True, True)
    ref = a64.forward(cn, a64.CAMPOS, inverse_covariance=True)
    for k, r in ref.items():
        assert tuple(out[k].shape) == r.shape, k
    assert out["xyz"].data_ptr() == st.view("xyz").data_ptr()
    check("densified", out, ref)
    backward(out, ups)
    check("densified", grads_of(st, 14), a64.backward(cn, ups, a64.CAMPOS), "grad_")
    assert torch.isfinite(st.grad).all()
