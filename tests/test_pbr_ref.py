"""CPU checks of the PBR image head and the light regulariser: tests/pbr_ref64.py against the float64 entries of
tests/golden/pbr_head.npz (torch autograd on the reference's expressions in float64), the boundary of the four
`_C.pbr` functions and of relightable3dgaussian_amd/pbr.py, and the C ABI's argument checks (no device work, so
no GPU)."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import relightable3dgaussian_amd as r
from relightable3dgaussian_amd import pbr
from tests import pbr_ref64 as p64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "r3dg_hip.h")
LIB = os.path.join(ROOT, "relightable3dgaussian_amd", "lib", "libr3dg_hip.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pbr_head.npz")
NAMES = ("r3dg_pbr_head_forward", "r3dg_pbr_head_backward", "r3dg_light_loss_forward", "r3dg_light_loss_backward")
ALLOC = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
EXACT = 1e-13  # float64 against float64: the same expressions, at most a different association


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def case(golden, name):
    return {k: golden[f"{name}/{k}"] for k in ("pbr", "opacity", "bg", "bgimg", "G", "gamma")}


# ---- the yardstick ---------------------------------------------------------------------------------------------

def test_ref64_reproduces_the_golden_float64_head(golden):
    assert set(golden["head_full"]) <= set(golden["head"]) and "r_67x131" in golden["head"]
    for name in golden["head_full"]:
        c = case(golden, name)
        for bgk in ("vec", "img"):
            bg = c["bg"] if bgk == "vec" else c["bgimg"]
            ref = {k: golden[f"{name}/{bgk}/f64/{k}"] for k in
                   ("y_gamma", "y_aces", "d_pbr_gamma", "d_opacity_gamma", "d_gamma", "d_opacity_none")}
            assert all(v.dtype == np.float64 for v in ref.values())
            assert p64.rel_err(p64.head_forward(c["pbr"], c["opacity"], bg, c["gamma"], "gamma"), ref["y_gamma"]) <= EXACT
            assert p64.rel_err(p64.head_forward(c["pbr"], c["opacity"], bg, None, "aces"), ref["y_aces"]) <= EXACT
            d_pbr, d_opacity, d_gamma = p64.head_backward(c["pbr"], c["opacity"], bg, c["G"], c["gamma"], "gamma")
            assert p64.rel_err(d_pbr, ref["d_pbr_gamma"]) <= EXACT
            assert p64.rel_err(d_opacity, ref["d_opacity_gamma"]) <= EXACT
            assert p64.rel_err(d_gamma, ref["d_gamma"]) <= EXACT
            d_pbr, d_opacity, d_gamma = p64.head_backward(c["pbr"], c["opacity"], bg, c["G"], None, "none")
            assert np.array_equal(d_pbr, c["G"].astype(np.float64)) and d_gamma is None
            assert p64.rel_err(d_opacity, ref["d_opacity_none"]) <= EXACT


def test_ref64_exact_modes_round_to_the_golden_float32(golden):
    """"none" and "clamp" are exactly rounded operations: the float32 image is the float64 one within the three
    roundings of the composite (2^-23 of the largest value covers them), and the clamp of the float32
    composite bit for bit."""
    for name in golden["head"]:
        c = case(golden, name)
        for bgk in ("vec", "img"):
            bg = c["bg"] if bgk == "vec" else c["bgimg"]
            y_none, y_clamp = golden[f"{name}/{bgk}/f32/y_none"], golden[f"{name}/{bgk}/f32/y_clamp"]
            assert y_none.dtype == np.float32 and y_clamp.dtype == np.float32
            assert p64.rel_err(y_none, p64.head_forward(c["pbr"], c["opacity"], bg, None, "none")) <= 2.0 ** -23
            assert p64.rel_err(y_clamp, p64.head_forward(c["pbr"], c["opacity"], bg, None, "clamp")) <= 2.0 ** -23
            np.testing.assert_array_equal(y_clamp, np.clip(y_none, 0, 1))


def test_ref64_gamma_edges(golden):
    """x = 1, nextafter(1, 2), lo, 0, -0.5 with opacity 1: which pass a gradient, and that the clamped ones still
    feed dL/dgamma."""
    lo = p64.LO
    for g in (0.45, 1.0, 2.2):
        c = case(golden, f"edge_g{g}")
        assert np.all(c["opacity"] == 1) and float(c["gamma"][0]) == float(np.float32(g))
        x = p64.composite(c["pbr"], c["opacity"], c["bg"])
        np.testing.assert_array_equal(x, c["pbr"].astype(np.float64))
        np.testing.assert_array_equal(x[0, :, 0], [1.0, float(np.nextafter(np.float32(1), np.float32(2))), lo, 0.0, -0.5])
        y = p64.head_forward(c["pbr"], c["opacity"], c["bg"], c["gamma"], "gamma")
        gg = float(c["gamma"][0])
        np.testing.assert_array_equal(y[0, :, 0], [1.0, 1.0, lo ** gg, lo ** gg, lo ** gg])
        d_pbr, d_opacity, d_gamma = p64.head_backward(c["pbr"], c["opacity"], c["bg"], c["G"], c["gamma"], "gamma")
        assert np.all(d_pbr[0, [0, 2]] != 0) and np.all(d_pbr[0, [1, 3, 4]] == 0)
        G = c["G"].astype(np.float64)
        want = (G[0, 2:] * lo ** gg * np.log(lo)).sum()  # the three pixels at lo; ln(1) = 0 for the two at 1
        assert abs(float(d_gamma[0]) - want) <= 1e-14 * abs(want) and want != 0


def test_ref64_reproduces_the_golden_float64_light(golden):
    for P in golden["light"]:
        d = golden[f"light_{P}/d"]
        assert d.shape == (P, 3) and d.dtype == np.float32
        np.testing.assert_array_equal(d, p64.draw_light(int(P), int(P)))
        v = float(golden[f"light_{P}/f64/value"])
        assert abs(p64.light_loss(d) - v) <= EXACT * abs(v)
        assert p64.rel_err(p64.light_loss_backward(d), golden[f"light_{P}/f64/grad"]) <= EXACT
        assert p64.ambiguous_sign(d).mean() <= p64.MAX_LEFT_OUT
    d = p64.draw_light(1025, 1025)
    g = p64.light_loss_backward(d)
    np.testing.assert_array_equal(g[1], 0.0)                       # equal channels
    np.testing.assert_array_equal(g[0] * d.size, [-1.0, 0.0, 1.0])  # (1, 2, 3): the middle channel is the mean
    assert p64.light_loss(np.zeros((0, 3), np.float32)) == 0.0


def test_floors_and_bars(golden):
    floors = {k: float(v) for k, v in golden.items() if "/floor/" in k}
    assert len(floors) >= 6 * len(golden["head"]) + 2 * (len(golden["light"]) + 1) + 3
    assert all(np.isfinite(v) and 0 <= v < 1e-3 for v in floors.values()), floors
    assert p64.bar(0.0) == 4 * 2.0 ** -24 and p64.bar(1e-6) == 4e-6


# ---- the boundary ----------------------------------------------------------------------------------------------

def test_binding_is_a_submodule_and_refuses_host_tensors():
    sub = r._C.pbr
    assert not callable(sub)
    assert {n for n in dir(sub) if callable(getattr(sub, n)) and not n.startswith("_")} == {
        "head_forward", "head_backward", "light_loss_forward", "light_loss_backward"}
    p, o, b, g = torch.zeros(4, 5, 3), torch.zeros(4, 5, 1), torch.zeros(3), torch.ones(1)
    d = torch.zeros(7, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sub.head_forward(p, o, b, None, 0, True)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sub.head_forward(p.permute(2, 0, 1).contiguous(), o.permute(2, 0, 1).contiguous(), torch.zeros(3, 4, 5), g, 1, False)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sub.head_backward(p, o, b, g, 1, True, p, 7)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sub.light_loss_forward(d)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sub.light_loss_backward(d, torch.ones(1))
    with pytest.raises(RuntimeError, match="float32"):
        sub.head_forward(p.double(), o, b, None, 0, True)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        sub.head_forward(p, o, b, None, 0, False)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        sub.head_forward(p, torch.zeros(4, 4, 1), b, None, 0, True)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        sub.head_forward(p, o, torch.zeros(4), None, 0, True)
    with pytest.raises(RuntimeError, match="gamma"):
        sub.head_forward(p, o, b, None, 1, True)
    with pytest.raises(RuntimeError, match="forward only"):
        sub.head_backward(p, o, b, None, 3, True, p, 3)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        sub.light_loss_forward(torch.zeros(7, 4))


def test_python_module_argument_errors():
    p, o, b, g = torch.zeros(4, 5, 3), torch.zeros(4, 5, 1), torch.zeros(3), torch.ones(1)
    bad = [(dict(image_layout="nhwc"), "pbr_image: image_layout"), (dict(tone="filmic"), "pbr_image: tone"),
           (dict(pbr=p.double()), "pbr_image: pbr"), (dict(pbr=torch.zeros(4, 5, 4)), "pbr_image: shape mismatch"),
           (dict(opacity=torch.zeros(4, 6, 1)), "pbr_image: shape mismatch"),
           (dict(image_layout="chw"), "pbr_image: shape mismatch"),
           (dict(bg=torch.zeros(4)), "pbr_image: shape mismatch"),
           (dict(bg=b.clone().requires_grad_(True)), "pbr_image: no gradient with respect to bg"),
           (dict(tone="gamma"), "pbr_image: gamma"), (dict(gamma=g), "pbr_image: gamma"),
           (dict(tone="gamma", gamma=torch.ones(2)), "pbr_image: gamma"),
           (dict(tone="gamma", gamma=torch.ones(1, device="meta")), "pbr_image: gamma is on"),
           (dict(bg=torch.zeros(3, device="meta")), "pbr_image: bg is on"),
           (dict(tone="aces", pbr=p.clone().requires_grad_(True)), "pbr_image: tone 'aces' is forward only"),
           (dict(tone="clamp", opacity=o.clone().requires_grad_(True)), "pbr_image: tone 'clamp' is forward only")]
    for kw, msg in bad:
        args = dict(pbr=p, opacity=o, bg=b)
        args.update(kw)
        with pytest.raises(ValueError, match=re.escape(msg)):
            pbr.pbr_image(**args)
    with pytest.raises(ValueError, match="light_loss: shape mismatch"):
        pbr.light_loss(torch.zeros(7, 4))
    with pytest.raises(ValueError, match="light_loss: diffuse_light"):
        pbr.light_loss(torch.zeros(7, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU tensor"):  # no torch fallback
        pbr.pbr_image(p, o, b)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pbr.light_loss(torch.zeros(7, 3))


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(LIB)
    lib.r3dg_last_error.restype = ctypes.c_char_p
    ci, vp = ctypes.c_int, ctypes.c_void_p
    lib.r3dg_pbr_head_forward.argtypes = [ci, ci, ci, ci, vp, vp, vp, ci, vp, vp, vp]
    lib.r3dg_pbr_head_backward.argtypes = [ci, ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, ALLOC, vp, vp]
    lib.r3dg_light_loss_forward.argtypes = [ci, vp, vp, ALLOC, vp, vp]
    lib.r3dg_light_loss_backward.argtypes = [ci, vp, vp, vp, vp]
    for n in NAMES:
        getattr(lib, n).restype = ci
    return lib


def test_header_declares_and_library_exports(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert hasattr(lib, n), n
    assert int(re.search(r"#define R3DG_ABI_VERSION (\d+)", text).group(1)) == 2  # additive: no struct changed


def test_argument_errors_need_no_device(lib):
    """R3DG_ERR_ARG (-1) with a message before any device work or allocation; P = 0 is R3DG_OK."""
    calls = []

    @ALLOC
    def never(ctx, nbytes):
        calls.append(nbytes)
        return None

    no_alloc = ctypes.cast(None, ALLOC)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(H=2, W=2, layout=1, tone=0, pbr=p, opacity=p, bg=p, gamma=None, image=p):
        return lib.r3dg_pbr_head_forward(H, W, layout, tone, pbr, opacity, bg, 0, gamma, image, None)

    def bwd(H=2, W=2, layout=1, tone=1, pbr=p, opacity=p, bg=p, gamma=p, up=p, d_pbr=p, d_gamma=p, alloc=never):
        return lib.r3dg_pbr_head_backward(H, W, layout, tone, pbr, opacity, bg, 0, gamma, up, d_pbr, None, d_gamma,
                                          alloc, None, None)

    bad = {"fwd H 0": lambda: fwd(H=0), "fwd W 0": lambda: fwd(W=0), "fwd negative H": lambda: fwd(H=-1),
           "fwd layout": lambda: fwd(layout=2), "fwd tone": lambda: fwd(tone=4), "fwd negative tone": lambda: fwd(tone=-1),
           "fwd null pbr": lambda: fwd(pbr=None), "fwd null opacity": lambda: fwd(opacity=None),
           "fwd null bg": lambda: fwd(bg=None), "fwd null image": lambda: fwd(image=None),
           "fwd gamma without gamma": lambda: fwd(tone=1), "fwd beyond int32": lambda: fwd(H=65536, W=65536),
           "bwd H 0": lambda: bwd(H=0), "bwd layout": lambda: bwd(layout=-1), "bwd aces": lambda: bwd(tone=2),
           "bwd clamp": lambda: bwd(tone=3), "bwd null bg": lambda: bwd(bg=None), "bwd null upstream": lambda: bwd(up=None),
           "bwd null pbr": lambda: bwd(pbr=None), "bwd null gamma": lambda: bwd(gamma=None),
           "bwd d_gamma with none": lambda: bwd(tone=0), "bwd null scratch_alloc": lambda: bwd(alloc=no_alloc),
           "light fwd negative P": lambda: lib.r3dg_light_loss_forward(-1, p, p, never, None, None),
           "light fwd null d": lambda: lib.r3dg_light_loss_forward(4, None, p, never, None, None),
           "light fwd null loss": lambda: lib.r3dg_light_loss_forward(4, p, None, never, None, None),
           "light fwd null scratch_alloc": lambda: lib.r3dg_light_loss_forward(4, p, p, no_alloc, None, None),
           "light bwd negative P": lambda: lib.r3dg_light_loss_backward(-1, p, p, p, None),
           "light bwd null upstream": lambda: lib.r3dg_light_loss_backward(4, p, None, p, None),
           "light bwd null grad": lambda: lib.r3dg_light_loss_backward(4, p, p, None, None)}
    for what, call in bad.items():
        assert call() == -1, what
        assert len(lib.r3dg_last_error()) > 0, what
    assert lib.r3dg_light_loss_forward(0, None, None, no_alloc, None, None) == 0
    assert lib.r3dg_light_loss_backward(0, None, None, None, None) == 0
    assert bwd(d_pbr=None, d_gamma=None) == 0  # no gradient wanted: nothing to do
    assert calls == []
