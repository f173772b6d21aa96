"""The relighting render equation's yardsticks and its C boundary, without a GPU.

  * tests/relight_ref64.py (the float64 restatement) reproduces tests/golden/relight.npz, the reference's
    own float32 results, within the noise floors it records -- so the HIP bars (4 x floor) cannot drift
    away from the measurement;
  * the restated nvdiffrast filter equals torch's grid_sample on the map padded circularly by one texel,
    a pin outside this project's own code;
  * include/r3dg_hip.h declares and the library exports the two entry points, and each refuses bad
    arguments with R3DG_ERR_ARG before any launch (called here with no device at all).
"""
from __future__ import annotations

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import relight_ref64 as r64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "r3dg_hip.h")
LIB = os.path.join(ROOT, "relightable3dgaussian_amd", "lib", "libr3dg_hip.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "relight.npz")
SETS = ("s24", "s384")


def golden_case(g, name, c):
    """The relight_ref64.render arguments of golden case (name, c): a baked + SH, b traced + map with a
    rotation, c traced + no light."""
    inp = {k: g[f"{name}_{k}"] for k in ["base", "rough", "metal", "normals", "viewdirs", "incidents", "visibility",
                                         "env"]}
    kw = dict(inp=inp, Ns=int(g[f"{name}_sample_num"]))
    if c == "a":
        kw.update(light_mode=r64.LIGHT_SH)
    elif c == "b":
        kw.update(light_mode=r64.LIGHT_MAP, envmap=g["envmap"], transform=g["transform"], traced=g[f"{name}_traced"])
    else:
        kw.update(light_mode=r64.LIGHT_NONE, traced=g[f"{name}_traced"])
    return kw


# directions on the lookup's edges: both poles, the tu = 0 / 1 seam (d = (-+0, -1, 0) and a hair to
# either side of it), the cube axes, and a few general ones
def edge_dirs():
    e = 1e-4
    d = [(0, 0, 1), (0, 0, -1), (0.0, -1, 0), (-0.0, -1, 0), (e, -1, 0), (-e, -1, 0), (e, -1, 0.3), (-e, -1, -0.3),
         (1, 0, 0), (-1, 0, 0), (0, 1, 0), (e, e, 1), (-e, e, -1), (0.3, -0.5, 0.8), (-0.7, 0.1, -0.2),
         (0.2, 0.9, 0.4), (-0.4, -0.4, 0.82), (0.6, 0.0, -0.8), (0.0, 0.6, 0.8), (1, 1, 1)]
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_case_list_is_complete(golden):
    for name, (P, Ns) in {"s24": (64, 24), "s384": (8, 384)}.items():
        assert golden[f"{name}_base"].shape == (P, 3) and int(golden[f"{name}_sample_num"]) == Ns
        assert golden[f"{name}_incidents"].shape == (P, 16, 3) and golden[f"{name}_visibility"].shape == (P, 25, 1)
        assert golden[f"{name}_traced"].shape == (P, Ns, 1) and golden[f"{name}_rough"].min() >= 0.05
        for c in "abc":
            for k in r64.OUTPUT_KEYS:
                assert golden[f"{name}_{c}_{k}"].shape[0] == P
    assert golden["envmap"].shape == (6, 10, 3) and golden["envmap"].max() / golden["envmap"].min() > 100
    t = golden["transform"].astype(np.float64)
    assert np.abs(t @ t.T - np.eye(3)).max() < 1e-6 and np.linalg.det(t) > 0
    assert os.path.getsize(GOLDEN) < 100 * 1024


@pytest.mark.parametrize("c", "abc")
@pytest.mark.parametrize("name", SETS)
def test_ref64_reproduces_golden(golden, name, c):
    """golden (the reference in float32) against ref64 stays within the recorded floor = bar / 4."""
    kw = golden_case(golden, name, c)
    ref = r64.render(**kw)
    floors = r64.FLOORS
    for k in r64.OUTPUT_KEYS:
        e = r64.rel_err(golden[f"{name}_{c}_{k}"], ref[k])
        print(f"{name} {c} {k}: {e:.3e} (floor {floors[k]:.1e})")
        assert e <= floors[k], (name, c, k, e)
        assert r64.BARS[k] == 4 * floors[k]
    a, b = r64.FEATURE_COLUMNS["rgb"]
    np.testing.assert_array_equal(ref["features"][:, a:b], ref["rgb"])


def test_floors_are_measured_not_padded(golden):
    """Each recorded floor is reached to within a factor 1.1 by some golden case: rounded up, not widened."""
    worst = {k: 0.0 for k in r64.OUTPUT_KEYS}
    for name in SETS:
        for c in "abc":
            ref = r64.render(**golden_case(golden, name, c))
            for k in r64.OUTPUT_KEYS:
                worst[k] = max(worst[k], r64.rel_err(golden[f"{name}_{c}_{k}"], ref[k]))
    for k in r64.OUTPUT_KEYS:
        assert worst[k] <= r64.FLOORS[k] <= 1.1 * worst[k], (k, worst[k])


def test_lookup_reproduces_golden(golden):
    worst = 0.0
    for key, tr in [("lookup_light", None), ("lookup_light_rot", golden["transform"])]:
        e = r64.rel_err(golden[key], r64.envmap_direct_light(golden["lookup_dirs"], golden["envmap"], tr))
        print(key, f"{e:.3e}")
        worst = max(worst, e)
    assert worst <= r64.ENVMAP_FLOOR <= 1.1 * worst and r64.ENVMAP_BAR == 4 * r64.ENVMAP_FLOOR


@pytest.mark.parametrize("shape", [(5, 7), (1, 1), (2, 3)])
def test_filter_equals_grid_sample(shape):
    """The restated wrap-bilinear filter against torch.nn.functional.grid_sample (bilinear,
    align_corners=False, padding_mode='border') on the map padded circularly by one texel on each side,
    at g = 2 (u n + 1) / (n + 2) - 1 with u, v reduced by their floor. Float64; measured 8e-16."""
    H, W = shape
    rng = np.random.default_rng(5)
    envmap = torch.tensor(np.exp(rng.normal(0, 1.5, (H, W, 3))))
    d = np.concatenate([edge_dirs(), rng.normal(size=(200, 3))])
    tu, tv = r64.texcoords(d / np.linalg.norm(d, axis=1, keepdims=True))
    # and texture coordinates outside [0, 1), which the filter must wrap
    tu = torch.cat([tu, torch.tensor([-0.25, 1.5, 1.0, 0.0, 2.0 - 1e-12])])
    tv = torch.cat([tv, torch.tensor([1.25, -0.5, 1.0, 0.0, 0.5])])
    got = r64.bilinear_wrap(envmap, tu, tv)
    chw = envmap.permute(2, 0, 1)[None]
    padded = torch.nn.functional.pad(chw, (1, 1, 1, 1), mode="circular")
    u, v = tu - torch.floor(tu), tv - torch.floor(tv)
    grid = torch.stack([2 * (u * W + 1) / (W + 2) - 1, 2 * (v * H + 1) / (H + 2) - 1], -1)[None, None]
    ref = torch.nn.functional.grid_sample(padded, grid, mode="bilinear", padding_mode="border",
                                          align_corners=False)[0, :, 0].T
    err = float((got - ref).abs().max() / ref.abs().max())
    print(shape, f"{err:.2e}")
    assert err < 1e-14


def test_seam_and_poles_are_continuous():
    """Across the tu = 0 / 1 seam and around each pole the lookup is continuous (the wrap in u; at a pole
    tv is 0 or 1 and every tu blends the same two rows)."""
    rng = np.random.default_rng(6)
    envmap = np.exp(rng.normal(0, 1.5, (5, 7, 3)))
    e = 1e-9
    left = r64.envmap_direct_light(np.array([[e, -1.0, 0.3]]), envmap)
    right = r64.envmap_direct_light(np.array([[-e, -1.0, 0.3]]), envmap)
    assert np.abs(left - right).max() < 1e-6 * np.abs(envmap).max()


# ---- the C boundary, no device -----------------------------------------------------------------------

FP = ctypes.c_void_p


class BrdfInputs(ctypes.Structure):  # r3dg_brdf_inputs
    _fields_ = [(n, ctypes.c_int) for n in ("P", "S_incident", "S_direct", "S_visibility", "sample_num")] + [
        (n, FP) for n in ("base_color", "roughness", "metallic", "normals", "viewdirs", "incidents_shs",
                          "direct_shs", "visibility_shs")]


class RelightInputs(ctypes.Structure):  # r3dg_relight_inputs
    _fields_ = [("struct_size", ctypes.c_size_t), ("brdf", BrdfInputs), ("light_mode", ctypes.c_int),
                ("envmap", FP), ("env_h", ctypes.c_int), ("env_w", ctypes.c_int), ("env_transform", FP),
                ("traced_visibility", FP)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m relightable3dgaussian_amd.build")
    lib = ctypes.CDLL(LIB)
    lib.r3dg_last_error.restype = ctypes.c_char_p
    lib.r3dg_render_equation_relight.restype = ctypes.c_int
    lib.r3dg_render_equation_relight.argtypes = [ctypes.POINTER(RelightInputs), FP, FP]
    lib.r3dg_envmap_direct_light.restype = ctypes.c_int
    lib.r3dg_envmap_direct_light.argtypes = [ctypes.c_int, FP, FP, ctypes.c_int, ctypes.c_int, FP, FP, FP]
    return lib


def test_header_declares_and_library_exports(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+r3dg_render_equation_relight\s*\(\s*const\s+r3dg_relight_inputs\s*\*\s*in\s*,"
                     r"\s*float\s*\*\s*features\s*,\s*r3dg_stream_t", text)
    assert re.search(r"\bint\s+r3dg_envmap_direct_light\s*\(\s*int\s+n\s*,\s*const\s+float\s*\*\s*dirs\s*,", text)
    assert re.search(r"typedef\s+struct\s+r3dg_relight_inputs\s*\{\s*size_t\s+struct_size\s*;", text)
    for n, v in [("NONE", 0), ("SH", 1), ("MAP", 2)]:
        assert re.search(rf"R3DG_LIGHT_{n}\s*=\s*{v}\b", text), n
    assert hasattr(lib, "r3dg_render_equation_relight") and hasattr(lib, "r3dg_envmap_direct_light")
    assert int(re.search(r"#define R3DG_ABI_VERSION (\d+)", text).group(1)) == 2  # additive: no struct changed


def test_argument_errors_need_no_device(lib):
    """R3DG_ERR_ARG (-1) with a message before any device work; P = 0 and n = 0 are R3DG_OK."""
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, FP)

    def inputs(**kw):
        b = BrdfInputs(P=1, S_incident=16, S_direct=16, S_visibility=25, sample_num=24, base_color=p, roughness=p,
                       metallic=p, normals=p, viewdirs=p, incidents_shs=p, direct_shs=p, visibility_shs=p)
        top = dict(struct_size=ctypes.sizeof(RelightInputs), light_mode=1)
        for k, v in kw.items():
            if k in dict(BrdfInputs._fields_):
                setattr(b, k, v)
            else:
                top[k] = v
        return RelightInputs(brdf=b, **top)

    def relight(**kw):
        return lib.r3dg_render_equation_relight(ctypes.byref(inputs(**kw)), p, None)

    bad = {"struct_size + 8": lambda: relight(struct_size=ctypes.sizeof(RelightInputs) + 8),
           "struct_size 0": lambda: relight(struct_size=0),
           "S_incident 26": lambda: relight(S_incident=26), "S_direct 26": lambda: relight(S_direct=26),
           "S_visibility 26": lambda: relight(S_visibility=26),
           "S_direct 26, no SH light": lambda: relight(S_direct=26, light_mode=0),
           "negative width": lambda: relight(S_incident=-1),
           "map without a map": lambda: relight(light_mode=2, envmap=None, env_h=4, env_w=8),
           "map with env_h 0": lambda: relight(light_mode=2, envmap=p, env_h=0, env_w=8),
           "map with env_w 0": lambda: relight(light_mode=2, envmap=p, env_h=4, env_w=0),
           "unknown light_mode": lambda: relight(light_mode=3),
           "sample_num 0": lambda: relight(sample_num=0), "negative P": lambda: relight(P=-1),
           "null input struct": lambda: lib.r3dg_render_equation_relight(None, p, None),
           "lookup without a map": lambda: lib.r3dg_envmap_direct_light(4, p, None, 4, 8, None, p, None),
           "lookup with env_h 0": lambda: lib.r3dg_envmap_direct_light(4, p, p, 0, 8, None, p, None),
           "lookup with env_w -1": lambda: lib.r3dg_envmap_direct_light(4, p, p, 4, -1, None, p, None),
           "lookup with negative n": lambda: lib.r3dg_envmap_direct_light(-1, p, p, 4, 8, None, p, None)}
    for what, call in bad.items():
        assert call() == -1, what
        assert len(lib.r3dg_last_error()) > 0, what
    assert b"25" in (relight(S_visibility=26), lib.r3dg_last_error())[1]
    assert relight(P=0) == 0 and relight(P=0, sample_num=0) == 0
    assert lib.r3dg_envmap_direct_light(0, None, p, 4, 8, None, None, None) == 0


def test_python_module_argument_errors():
    """bake=False without visibility_precompute raises ValueError before the extension is reached, as the
    reference does; a CPU tensor is refused (no CPU path, no torch fallback)."""
    from relightable3dgaussian_amd import relight

    z = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="pre-computed"):
        relight.render_equation_relight(z, z[:, :1], z[:, :1], z, z, torch.zeros(2, 16, 3), None,
                                        torch.zeros(2, 25, 1), 24, bake=False)
    with pytest.raises(RuntimeError, match="GPU"):
        relight.render_equation_relight(z, z[:, :1], z[:, :1], z, z, torch.zeros(2, 16, 3), None,
                                        torch.zeros(2, 25, 1), 24, bake=True)
    with pytest.raises(RuntimeError, match="GPU"):
        relight.EnvLight(torch.ones(2, 3, 3)).direct_light(z)
    with pytest.raises(ValueError):
        relight.EnvLight(torch.ones(2, 3))
    assert relight.FEATURE_COLUMNS == r64.FEATURE_COLUMNS
    assert math.isclose(sum(b - a for a, b in relight.FEATURE_COLUMNS.values()), 21)
