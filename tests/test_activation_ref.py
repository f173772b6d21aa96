"""CPU checks of the parameter-activation references: tests/golden/activation.npz (the reference's own
float32 torch code) against tests/activation_ref64.py within FLOORS, the ref64 backward against a float64 central
difference of the ref64 forward, and the C entry points' struct_size refusal (no device work, so no GPU)."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import pytest

from tests import activation_ref64 as a64

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_activation as mga  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "activation.npz"))


@pytest.fixture(scope="module")
def refs(golden):
    """case -> (ref64 forward, ref64 backward), computed once."""
    out = {}
    for name in mga.CASES:
        c, ups, campos = mga.case_inputs(golden, name)
        out[name] = (a64.forward(c, campos, inverse_covariance=True, rotation="rotation_fwd"),
                     a64.backward(c, ups, campos))
    return out


@pytest.mark.parametrize("name", sorted(mga.CASES))
def test_golden_within_floors(golden, refs, name):
    fwd, bwd = refs[name]
    kw = mga.CASES[name]
    assert set(bwd) == {g for g, _ in a64.groups_of(kw["groups"])}
    assert ("viewdirs" in fwd) == kw["campos"] and "symm_inv" in fwd
    for k, ref in list(fwd.items()) + [(f"grad_{g}", v) for g, v in bwd.items()]:
        if k == "xyz":
            continue
        got = golden[f"{name}_{'out_' if not k.startswith('grad_') else ''}{k}"]
        e = a64.row_err(got, ref)
        print(f"{name} {k:22s} {e:.3e} (floor {a64.FLOORS[k]:.1e})")
        assert e <= a64.FLOORS[k], k


@pytest.mark.parametrize("name", sorted(mga.CASES))
def test_sh_concatenations_are_copies(golden, refs, name):
    fwd, bwd = refs[name]
    for out, (dc, rest) in a64.SH.items():
        if out not in fwd:
            continue
        np.testing.assert_array_equal(golden[f"{name}_out_{out}"], fwd[out])
        np.testing.assert_array_equal(golden[f"{name}_grad_{dc}"], bwd[dc])
        np.testing.assert_array_equal(golden[f"{name}_grad_{rest}"], bwd[rest])
        assert fwd[out].shape[1] == 16


def test_floors_are_the_measured_ones(golden):
    """FLOORS = the measured distances rounded UP to two digits: none below its measurement, none more than
    one two-digit step above it."""
    for k, v in mga.measure(golden).items():
        assert v <= a64.FLOORS[k], k
        assert a64.FLOORS[k] <= v * 1.1 + 1e-300 or v == 0.0 == a64.FLOORS[k], (k, v, a64.FLOORS[k])
    assert all(abs(a64.BARS[k] - 4 * a64.FLOORS[k]) <= 1e-12 * a64.FLOORS[k] for k in a64.FLOORS)


# ---- ref64 backward against a central difference of the ref64 forward ------------------------------------
#
# Every output row depends on the same row of the parameters only, so the check runs per row and per
# (parameter group, output) pair: phi(x) = <out(x), g> with the other groups fixed, numerically
# (phi(x + h e_j) - phi(x - h e_j)) / 2h. The step is RELATIVE to the row's own scale, h = DELTA * scale:
# |x| for a vector that is normalised (|campos - xyz| for the view direction), max(|x|, 1) for exp and sigmoid.
# A fixed absolute step above the shortest normals (5e-5) would straddle eps = 1e-3; with DELTA = 1e-5 and no
# normal within 1 % of eps, x +- h stays on x's side. A relative step of the zero normal is zero, so for that
# row the backward's g / eps branch is tested directly (the next test).
#
# Bar per row, absolute, then put through row_err's denominator max(max_c |ref|, 1e-37):
#   truncation  h^2 / 6 * M3, M3 a bound on |phi'''| along the step:
#       normalise  phi = g . x / |x| is homogeneous of degree 0: |phi'''| <= 15 |g| / |x|^3
#                  (x / eps below eps is linear: 0)
#       exp        |g| e^x e^h            sigmoid   |s'''| = |s' (1 - 6 s (1 - s))| <= s', so |g| s (1 - s) * 2
#                                                    (the factor 2 covers the move of s' over h <= 1e-3)
#       SH copies, xyz passthrough: linear, 0
#   roundoff    the two phi values carry 4 eps64 (|phi| + |g|_1 max|out|) each: 8 eps64 (...) / 2h
# At opacity +100 the difference of two values that both round to 1 is 0 against a derivative of 3.7e-44 g:
# the roundoff term says so and the 1e-37 of row_err forgives it, as it forgives the flushed denormal.
DELTA = 1e-5
EPS64 = np.finfo(np.float64).eps


def _fd_rows(P):
    reg = a64.normal_regions(P)
    rows = {k: v[:10] for k, v in reg.items() if k != "zero"}
    rows["saturated_opacity"] = np.arange(4)
    return rows


def _check_pair(c, ups, campos, gref, group, out_name, row, scale, m3):
    """Central difference of group -> out_name at `row`; returns (row error, allowed row error)."""
    one = {k: v[row:row + 1] for k, v in c.items()}
    g = ups[out_name][row:row + 1]
    h = DELTA * scale
    num = np.zeros(one[group].size)
    mag = 0.0
    for j in range(num.size):
        vals = []
        for s in (+1, -1):
            x = one[group].copy()
            x.reshape(-1)[j] += s * h
            out = a64.forward(dict(one, **{group: x}), campos)[out_name]
            vals.append(float((out * g).sum()))
            mag = max(mag, abs(vals[-1]) + float(np.abs(g).sum() * np.abs(out).max()))
        num[j] = (vals[0] - vals[1]) / (2 * h)
    ref = gref.reshape(-1)
    allowed_abs = h * h / 6 * m3 + 8 * EPS64 * mag / (2 * h)
    den = max(np.abs(ref).max(), 1e-37)
    return float(np.abs(num - ref).max() / den), float(allowed_abs / den)


def test_ref64_backward_is_the_central_difference():
    P = 257
    c = {k: v.astype(np.float64) for k, v in a64.draw_case(P, 41, 14).items() if k != "rotation_fwd"}
    ups = {k: v.astype(np.float64) for k, v in a64.draw_upstreams(P, 1041, 14, True).items()}
    campos = a64.CAMPOS.astype(np.float64)
    checked = 0
    for regime, rows in _fd_rows(P).items():
        assert len(rows) >= (4 if regime == "saturated_opacity" else 10), regime
        for row in rows:
            one = lambda out_name: a64.backward(  # noqa: E731  (the gradient through ONE output)
                {k: v[row:row + 1] for k, v in c.items()}, {out_name: ups[out_name][row:row + 1]}, campos)
            norm3 = lambda x, g: 15 * np.linalg.norm(g) / np.linalg.norm(x) ** 3  # noqa: E731
            n, q, v = c["normal"][row], c["rotation"][row], campos - c["xyz"][row]
            below = np.linalg.norm(n) < a64.EPS_NORMAL
            pairs = [("normal", "normal", np.linalg.norm(n), 0.0 if below else norm3(n, ups["normal"][row])),
                     ("rotation", "rotation", np.linalg.norm(q), norm3(q, ups["rotation"][row])),
                     ("xyz", "viewdirs", np.linalg.norm(v), norm3(v, ups["viewdirs"][row])),
                     ("xyz", "xyz", 1.0, 0.0), ("f_rest", "shs", 1.0, 0.0), ("visibility_dc", "visibility", 1.0, 0.0)]
            x = c["scaling"][row]
            scale = max(np.abs(x).max(), 1.0)
            pairs.append(("scaling", "scaling", scale,
                          float((np.abs(ups["scaling"][row]) * np.exp(x)).max() * np.exp(DELTA * scale))))
            for name in a64.SIGMOIDS:
                x = c[name][row]
                s = a64._sigmoid(x)
                pairs.append((name, name, max(np.abs(x).max(), 1.0),
                              float((np.abs(ups[name][row]) * s * (1 - s)).max() * 2)))
            for group, out_name, scale, m3 in pairs:
                err, allowed = _check_pair(c, ups, campos, one(out_name)[group], group, out_name, row, scale, m3)
                assert err <= allowed, (regime, row, group, out_name, err, allowed)
                checked += 1
    assert checked == 34 * 11
    # the whole backward is the sum over the outputs (xyz receives two of them)
    full = a64.backward(c, ups, campos)
    both = a64.backward(c, {"xyz": ups["xyz"]}, campos)["xyz"] + a64.backward(c, {"viewdirs": ups["viewdirs"]},
                                                                            campos)["xyz"]
    np.testing.assert_allclose(full["xyz"], both, rtol=1e-15, atol=0)


def test_ref64_zero_and_short_normals_take_the_eps_branch():
    P = 257
    c = a64.draw_case(P, 41, 14)
    ups = a64.draw_upstreams(P, 1041, 14, True)
    reg = a64.normal_regions(P)
    g = a64.backward(c, {"normal": ups["normal"]})["normal"]
    z = reg["zero"]
    assert np.all(c["normal"][z] == 0)
    np.testing.assert_array_equal(g[z], ups["normal"][z].astype(np.float64) / 1e-3)
    np.testing.assert_array_equal(g[reg["below"]], ups["normal"][reg["below"]].astype(np.float64) / 1e-3)
    np.testing.assert_array_equal(a64.forward(c)["normal"][z], 0.0)
    # above eps the gradient is tangent to the normal
    y = a64.forward(c)["normal"][reg["above"]]
    assert np.abs((g[reg["above"]] * y).sum(1)).max() <= 1e-9 * np.abs(g[reg["above"]]).max()


# ---- the C entry points refuse a wrong struct_size before any device work --------------------------------

class ParamLayout(C.Structure):  # r3dg_param_layout
    _fields_ = [("P", C.c_int), ("n_groups", C.c_int), ("width", C.c_int * 16), ("xyz", C.c_int), ("scaling", C.c_int),
                ("rotation", C.c_int), ("opacity", C.c_int)]


class ActivationIO(C.Structure):  # r3dg_activation_io
    _fields_ = ([("struct_size", C.c_size_t), ("layout", C.POINTER(ParamLayout))] +
                [(n, C.c_int) for n in ("normal", "f_dc", "f_rest", "base_color", "roughness", "metallic",
                                        "incidents_dc", "incidents_rest", "visibility_dc", "visibility_rest")] +
                [(n, C.c_void_p) for n in ("campos", "out_scaling", "out_rotation", "out_normal", "out_opacity",
                                           "out_shs", "out_base_color", "out_roughness", "out_metallic",
                                           "out_incidents", "out_visibility", "out_viewdirs", "out_symm_inv")])


class GradRows(C.Structure):  # r3dg_grad_rows
    _fields_ = [("ptr", C.c_void_p), ("stride", C.c_int64)]


class ActivationGrads(C.Structure):  # r3dg_activation_grads
    _fields_ = [("struct_size", C.c_size_t)] + [
        (n, GradRows) for n in ("xyz", "scaling", "rotation", "normal", "opacity", "shs", "base_color", "roughness",
                                "metallic", "incidents", "visibility", "viewdirs")]


def _io(layout, n_groups=14):
    io = ActivationIO()
    io.struct_size = C.sizeof(ActivationIO)
    io.layout = C.pointer(layout)
    names = [g for g, _ in a64.groups_of(n_groups)]
    for f, _ in ActivationIO._fields_[2:12]:
        setattr(io, f, names.index(f) if f in names else -1)
    return io


def _layout(P, n_groups=14):
    L = ParamLayout()
    groups = a64.groups_of(n_groups)
    names = [g for g, _ in groups]
    L.P, L.n_groups = P, n_groups
    for i, (_, s) in enumerate(groups):
        L.width[i] = int(np.prod(s))
    L.xyz, L.scaling, L.rotation, L.opacity = (names.index(n) for n in ("xyz", "scaling", "rotation", "opacity"))
    return L


def test_struct_size_checked_before_any_device_work():
    """A wrong struct_size of either struct is R3DG_ERR_ARG (-1) with P > 0 and no valid pointer anywhere: had
    a launch been attempted, it would have needed a device. The right sizes then pass the argument checks of
    a P = 0 layout (nothing launched) and refuse a layout that breaks the role rule."""
    import torch  # noqa: F401  (loads the HIP runtime the library links)

    lib = C.CDLL(os.path.join(ROOT, "relightable3dgaussian_amd", "lib", "libr3dg_hip.so"))
    lib.r3dg_last_error.restype = C.c_char_p
    lib.r3dg_activate_forward.argtypes = [C.POINTER(ActivationIO), C.c_void_p, C.c_void_p]
    lib.r3dg_activate_backward.argtypes = [C.POINTER(ActivationIO), C.c_void_p, C.POINTER(ActivationGrads),
                                           C.c_void_p, C.c_int, C.c_void_p]
    L = _layout(1000)
    good_g = ActivationGrads()
    good_g.struct_size = C.sizeof(ActivationGrads)
    for size in (0, C.sizeof(ActivationIO) - 8, C.sizeof(ActivationIO) + 8, 12345):
        io = _io(L)
        io.struct_size = size
        assert lib.r3dg_activate_forward(C.byref(io), None, None) == -1, size
        assert b"struct_size" in lib.r3dg_last_error()
        assert lib.r3dg_activate_backward(C.byref(io), None, C.byref(good_g), None, 0, None) == -1, size
        assert b"r3dg_activation_io.struct_size" in lib.r3dg_last_error()
    for size in (0, C.sizeof(ActivationGrads) - 8, C.sizeof(ActivationGrads) + 16):
        g = ActivationGrads()
        g.struct_size = size
        assert lib.r3dg_activate_backward(C.byref(_io(L)), None, C.byref(g), None, 0, None) == -1, size
        assert b"r3dg_activation_grads.struct_size" in lib.r3dg_last_error()
    # the mirrors above are the header's layout: the true sizes pass, and P = 0 launches nothing
    for n_groups in (7, 14):
        L0 = _layout(0, n_groups)
        assert lib.r3dg_activate_forward(C.byref(_io(L0, n_groups)), None, None) == 0, lib.r3dg_last_error()
        assert lib.r3dg_activate_backward(C.byref(_io(L0, n_groups)), None, C.byref(good_g), None, 0, None) == 0, \
            lib.r3dg_last_error()
    bad = _io(L)
    bad.f_rest = bad.f_dc  # a group named twice
    assert lib.r3dg_activate_forward(C.byref(bad), None, None) == -1
    short = _io(L)
    g = ActivationGrads()
    g.struct_size = C.sizeof(ActivationGrads)
    g.shs = GradRows(1, 47)  # a row stride below the row's width (never dereferenced)
    assert lib.r3dg_activate_backward(C.byref(short), None, C.byref(g), None, 0, None) == -1
    assert b"stride" in lib.r3dg_last_error()
