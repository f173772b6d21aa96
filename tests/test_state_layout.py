"""What the rasterizer's forward and backward request from their allocators.

Both entry points size every state buffer and call the caller's allocators before their first HIP
call, and return R3DG_ERR_ALLOC when an allocator returns NULL. An allocator that records
(which, nbytes) and returns NULL therefore reads the whole memory layout out without a kernel: the
geometry state with its tail (working copies, blur snapshot, shader and intermediate records,
prepared sums), the image state with or without the binning counts, and the transient scratch.

The expected byte counts were recorded from the tree before the forward was split into a layout
plan and stages (commit ea7798b); the packing is part of what later changes must not move by
accident: floats packed, shader records 16-byte aligned, the tail padded to 256, the sums after it,
the binning counts rounded to 256 before the records in scratch.
"""
from __future__ import annotations

import ctypes
import os

import pytest

from tests import _abi_ctypes as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "relightable3dgaussian_amd", "lib", "libr3dg_hip.so")
R3DG_ERR_ALLOC = -4
FAKE = 0x1000  # a non-null pointer the library never dereferences on the host


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m relightable3dgaussian_amd.build")
    import torch  # noqa: F401  (loads torch's libamdhip64 first, as the package does)

    return A.bind(ctypes.CDLL(LIB))


class _Options:
    """r3dg_set_options for the duration of a with block."""

    def __init__(self, lib, **kw):
        self.lib, self.kw = lib, kw

    def __enter__(self):
        self.cur = A.new(A.Options)
        assert self.lib.r3dg_get_options(ctypes.byref(self.cur)) == 0, self.lib.r3dg_last_error()
        new = A.new(A.Options)
        ctypes.memmove(ctypes.byref(new), ctypes.byref(self.cur), ctypes.sizeof(A.Options))
        # the tables below are for the atomic flush unless a case says otherwise (the environment may
        # seed bwd_reduce)
        new.bwd_reduce = 0
        for k, v in self.kw.items():
            setattr(new, k, v)
        assert self.lib.r3dg_set_options(ctypes.byref(new)) == 0, self.lib.r3dg_last_error()

    def __exit__(self, *exc):
        assert self.lib.r3dg_set_options(ctypes.byref(self.cur)) == 0


def _recorder():
    """Allocators for "geom", "binning", "image", "scratch" that record the request and fail."""
    log = []

    def make(which):
        def alloc(ctx, n):
            log.append((which, n))
            return None
        return A.ALLOC(alloc)

    return log, {w: make(w) for w in ("geom", "binning", "image", "scratch")}


def forward_requests(lib, P, S, H, W, *, scratch=True, sh=False, M=0, D=0, **settings):
    """[(which, nbytes)] of one r3dg_rasterize_gaussians_ex call with failing allocators."""
    s = A.new(A.RasterSettings, P=P, S=S, H=H, W=W, M=M, D=D, tan_fovx=1.0, tan_fovy=1.0, scale_modifier=1.0,
              bg=FAKE, viewmatrix=FAKE, viewmatrix_inv=FAKE, projmatrix=FAKE, projmatrix_inv=FAKE, campos=FAKE,
              **settings)
    g = A.Gaussians(means3D=FAKE, opacity=FAKE, scales=FAKE, rotations=FAKE)
    if S > 0:
        g.features = FAKE
    if sh:
        g.sh = FAKE
    else:
        g.colors_precomp = FAKE
    out = A.ForwardOutputs(**{n: FAKE for n, _ in A.ForwardOutputs._fields_})
    log, al = _recorder()
    nr = ctypes.c_int(-1)
    rc = lib.r3dg_rasterize_gaussians_ex(ctypes.byref(s), ctypes.byref(g), ctypes.byref(out), al["geom"], None,
                                         al["binning"], None, al["image"], None,
                                         al["scratch"] if scratch else A.ALLOC(0), None, ctypes.byref(nr), None)
    assert rc == R3DG_ERR_ALLOC, (rc, lib.r3dg_last_error())
    assert b"allocation failed" in lib.r3dg_last_error()
    return log


def backward_requests(lib, P, S, L):
    s = A.new(A.RasterSettings, P=P, S=S, H=40, W=56, tan_fovx=1.0, tan_fovy=1.0, scale_modifier=1.0, bg=FAKE,
              viewmatrix=FAKE, projmatrix=FAKE, campos=FAKE)
    g = A.Gaussians(means3D=FAKE, opacity=FAKE, scales=FAKE, rotations=FAKE, colors_precomp=FAKE)
    if S > 0:
        g.features = FAKE
    gr = A.BackwardGrads(dL_dout_color=FAKE)
    out = A.new(A.BackwardOutputs)
    log, al = _recorder()
    # a geometry state address no forward of this process has used: no prepared sums behind it
    rc = lib.r3dg_rasterize_gaussians_backward(ctypes.byref(s), ctypes.byref(g), None, ctypes.byref(gr), 0x7000000,
                                               FAKE, FAKE, L, 1, al["scratch"], None, ctypes.byref(out), None)
    assert rc == R3DG_ERR_ALLOC, (rc, lib.r3dg_last_error())
    assert b"scratch allocation failed" in lib.r3dg_last_error()
    return log


# (P, S, H, W, options, call keywords) -> bytes requested (geometry, image, scratch or None)
FORWARD_CASES = [
    ((1, 0, 16, 16, {}, {}), (3968, 7680, 1280)),
    ((300, 11, 40, 56, {}, {}), (99584, 23552, 12544)),
    ((300, 11, 40, 56, {}, dict(scratch=False)), (99584, 36096, None)),
    ((300, 11, 40, 56, dict(bwd_reduce=1), {}), (61184, 23552, 12544)),
    ((257, 21, 33, 17, {}, {}), (132352, 10240, 6400)),
    ((257, 21, 33, 17, dict(test_bwd_srs=40), {}), (115904, 10240, 6400)),
    # 36864 tiles: the last size with LDS binning
    ((1000, 3, 2304, 4096, {}, {}), (294400, 76533760, 8262400)),
    # more tiles: the atomic-binning fallback
    ((1000, 3, 2400, 4096, {}, dict(scratch=False)), (294400, 79727360, None)),
    ((300, 32, 16, 16, dict(test_bwd_dpp=1), dict(sh=True, M=16, D=3)), (85248, 7680, 1280)),
]


@pytest.mark.parametrize("case,want", FORWARD_CASES, ids=[f"P{c[0]}_S{c[1]}_{c[2]}x{c[3]}_{i}"
                                                          for i, (c, _) in enumerate(FORWARD_CASES)])
def test_forward_requests(lib, case, want):
    P, S, H, W, opts, kw = case
    with _Options(lib, **opts):
        log = forward_requests(lib, P, S, H, W, **kw)
    print("forward", case, log)
    geom, image, scratch = want
    expect = [("geom", geom), ("image", image)] + ([("scratch", scratch)] if scratch is not None else [])
    assert log == expect  # the binning state is sized after num_rendered is known: not requested here


# (P, S, L, options) -> scratch bytes requested
BACKWARD_CASES = [
    ((300, 11, 700, {}), 38400),
    ((300, 11, 700, dict(bwd_reduce=1)), 297600),
    ((257, 21, 0, dict(test_bwd_dpp=1)), 41120),
    ((257, 21, 5, dict(test_bwd_srs=40)), 49344),
    ((1, 0, 1, {}), 128),
]


@pytest.mark.parametrize("case,want", BACKWARD_CASES, ids=[f"P{c[0]}_S{c[1]}_L{c[2]}_{i}"
                                                           for i, (c, _) in enumerate(BACKWARD_CASES)])
def test_backward_requests(lib, case, want):
    P, S, L, opts = case
    with _Options(lib, **opts):
        log = backward_requests(lib, P, S, L)
    print("backward", case, log)
    assert log == [("scratch", want)]


# ---------------------------------------------------------------------------------------------
# shader path: the managers need hipMalloc, the layout read-out itself launches nothing
# ---------------------------------------------------------------------------------------------
SHADER_P, SHADER_S, SHADER_H, SHADER_W = 300, 21, 56, 40
# case -> bytes requested (geometry, image, scratch or None)
SHADER_CASES = {
    "a_scratch": (193792, 23552, 50944),
    "a_no_scratch": (232192, 36096, None),
    "b_invert": (75520, 23552, 17344),
    "c_wireframe": (75520, 23552, 50944),
}


def _handle(lib, kind, name):
    lib.r3dg_shader_name.restype = ctypes.c_char_p
    lib.r3dg_shader_handle.restype = ctypes.c_int64
    for i in range(lib.r3dg_shader_count(kind)):
        if lib.r3dg_shader_name(kind, i) == name.encode():
            return lib.r3dg_shader_handle(kind, i)
    raise KeyError(name)


def _manager(lib, kind, names):
    """A shader manager whose splat i runs names[i % len(names)]."""
    hs = [_handle(lib, kind, n) for n in names]
    arr = (ctypes.c_int64 * SHADER_P)(*[hs[i % len(hs)] for i in range(SHADER_P)])
    m = ctypes.c_int64(0)
    assert lib.r3dg_create_shader_manager(kind, SHADER_P, arr, ctypes.byref(m), None) == 0, lib.r3dg_last_error()
    return m.value


@pytest.fixture(scope="module")
def shader_setup(lib):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    SH, SPLAT, POST = 0, 1, 2
    # an empty texture manager: every name resolves to the error texture (TextureManager::GetTexture)
    px = torch.ones(1, 1, 1, device="cuda")
    tex, tm = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.r3dg_texture_create(ctypes.c_void_p(px.data_ptr()), 1, 1, 10, 1, 1, 1, ctypes.byref(tex), None) == 0
    assert lib.r3dg_texture_manager_create(0, None, None, tex, ctypes.byref(tm)) == 0, lib.r3dg_last_error()
    post = lambda *names: (ctypes.c_int64 * len(names))(*[_handle(lib, POST, n) for n in names])  # noqa: E731
    return {
        # SH shaders that write positions, scales, opacity and sh0; Crack reads the intermediate depth,
        # RoughnessOnly writes features; BlurLighting snapshots the incident light
        "a": dict(sh_shader_manager=_manager(lib, SH, ["ShDefault", "ExpPos", "GaussDissolve"]),
                  splat_shader_manager=_manager(lib, SPLAT, ["SplatDefault", "Crack", "RoughnessOnly"]),
                  texture_manager=tm.value, passes=post("BlurLighting")),
        "b": dict(passes=post("Invert")),
        "c": dict(splat_shader_manager=_manager(lib, SPLAT, ["SplatDefault", "Wireframe"]), passes=None),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(SHADER_CASES))
def test_forward_requests_shader_path(lib, shader_setup, case):
    cfg = dict(shader_setup[case[0]])
    passes = cfg.pop("passes")
    if passes is not None:
        cfg["post_passes"] = ctypes.cast(passes, ctypes.c_void_p)
        cfg["n_post_passes"] = len(passes)
    with _Options(lib):
        log = forward_requests(lib, SHADER_P, SHADER_S, SHADER_H, SHADER_W, scratch=case != "a_no_scratch", sh=True,
                               M=16, D=3, **cfg)
    print("shader path", case, log)
    geom, image, scratch = SHADER_CASES[case]
    expect = [("geom", geom), ("image", image)] + ([("scratch", scratch)] if scratch is not None else [])
    assert log == expect
