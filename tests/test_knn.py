"""distCUDA2 (csrc/knn.hip, the reference's simple_knn._C): the mean squared distance to the three
nearest neighbours, bit for bit against a numpy-f32 brute force, through the torch binding, the raw C
ABI and GaussianTrainState.create_from_pcd; plus the CPU checks of the boundary (header, exports,
argument errors, the `simple_knn` import aliases)."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "r3dg_hip.h")
LIB = os.path.join(ROOT, "relightable3dgaussian_amd", "lib", "libr3dg_hip.so")
FLT_MAX = np.finfo(np.float32).max
ALLOC = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)


# ---- reference -----------------------------------------------------------------------------------

def brute_force(x: np.ndarray, chunk: int = 128) -> np.ndarray:
    """((b0 + b1) + b2) / 3 over the three smallest d2(i, j), j != i, d2 = (dx dx + dy dy) + dz dz with
    d = p_j - p_i: every operation a separate f32 numpy operation (no FMA), missing neighbours FLT_MAX."""
    x = np.ascontiguousarray(x, np.float32)
    P = x.shape[0]
    out = np.empty(P, np.float32)
    cols = [np.ascontiguousarray(x[:, a]) for a in range(3)]
    row = np.full((chunk, P + 3), FLT_MAX, np.float32)  # the [n, P] matrix of d2 and three FLT_MAX columns
    tmp = np.empty((chunk, P), np.float32)
    with np.errstate(over="ignore"):
        for s in range(0, P, chunk):
            n = min(chunk, P - s)
            d2, t = row[:n, :P], tmp[:n]
            np.subtract(cols[0][None, :], cols[0][s:s + n, None], out=d2)  # dx = p_j.x - p_i.x
            np.multiply(d2, d2, out=d2)
            np.subtract(cols[1][None, :], cols[1][s:s + n, None], out=t)
            np.multiply(t, t, out=t)
            np.add(d2, t, out=d2)                                          # dx*dx + dy*dy
            np.subtract(cols[2][None, :], cols[2][s:s + n, None], out=t)
            np.multiply(t, t, out=t)
            np.add(d2, t, out=d2)                                          # (...) + dz*dz
            d2[np.arange(n), s + np.arange(n)] = FLT_MAX  # exclusion by index
            b = np.sort(np.partition(row[:n], 2, axis=1)[:, :3], axis=1)
            out[s:s + n] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3)
    return out


def bits_equal(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    if not bits_equal(got, ref):
        bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32)) if got.shape == ref.shape else []
        raise AssertionError(f"{what}: {len(bad)} of {ref.size} differ, first {bad[:5]}: "
                             f"got {got[bad[:5]] if len(bad) else got.shape} ref {ref[bad[:5]] if len(bad) else ref.shape}")


def uniform(P, seed=0):
    return np.random.default_rng(seed).random((P, 3), dtype=np.float32)


def _planar():
    x = uniform(4096, 1)
    x[:, 2] = 0.25
    return x


def _collinear():
    t = np.random.default_rng(2).random(4096, dtype=np.float32)
    return np.stack([t, np.float32(2) * t, -t], axis=1).astype(np.float32)


def _anisotropic():
    return uniform(4096, 3) * np.array([1e3, 1.0, 1e-3], np.float32)


def _lattice():
    g = np.stack(np.meshgrid(*[np.arange(16, dtype=np.float32)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return g[np.random.default_rng(4).permutation(len(g))]


def _duplicates():
    x = np.repeat(uniform(1024, 5), 4, axis=0)
    return x[np.random.default_rng(6).permutation(len(x))]


def _clusters():
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(7)
    a = (g * 1e-2 + rng.random(g.shape) * 1e-3).astype(np.float32)
    b = (g * 1e-2 + rng.random(g.shape) * 1e-3).astype(np.float32)
    b[:, 0] += np.float32(1e4)
    x = np.concatenate([a, b])
    return x[rng.permutation(len(x))]


def _outlier():
    x = uniform(4096, 8)
    x[1234] = (50.0, 50.0, 50.0)
    return x


def _medium():
    rng = np.random.default_rng(9)
    centres = rng.random((8, 3))
    blobs = centres[rng.integers(0, 8, 10000)] + rng.normal(0.0, 0.01, (10000, 3))
    x = np.concatenate([rng.random((10000, 3)), blobs]).astype(np.float32)
    return x[rng.permutation(len(x))]


def _supers():
    """517 boxes of 64 points in nine super-boxes of 64 boxes (the last box holds one point, the last
    super-box five boxes): waves of the middle super-boxes walk outward in both directions."""
    return uniform(8 * 64 * 64 + 257, 10)


DISTRIBUTIONS = {"planar": _planar, "collinear": _collinear, "anisotropic": _anisotropic, "lattice": _lattice,
                 "duplicates": _duplicates, "clusters": _clusters, "outlier": _outlier, "medium": _medium,
                 "supers": _supers}
_CACHE: dict = {}


def case(name):
    """(points, reference) of a named input, computed once per session and never modified."""
    if name not in _CACHE:
        x = DISTRIBUTIONS[name]() if name in DISTRIBUTIONS else uniform(int(name), seed=100 + int(name))
        ref = brute_force(x)
        x.setflags(write=False)
        ref.setflags(write=False)
        _CACHE[name] = (x, ref)
    return _CACHE[name]


def test_brute_force_reference_on_known_values():
    """The reference itself: the padding rule and two hand-checked values."""
    assert np.isposinf(brute_force(np.zeros((1, 3), np.float32))).all()
    assert np.isposinf(brute_force(uniform(2))).all()
    three = brute_force(np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32))
    assert bits_equal(three, ((np.float32([1, 1, 4]) + np.float32([4, 5, 5])) + FLT_MAX) / np.float32(3))
    four = brute_force(np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]], np.float32))
    assert bits_equal(four, np.float32([14, 16, 22, 32]) / np.float32(3))


# ---- CPU: the boundary -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m relightable3dgaussian_amd.build")
    import torch  # noqa: F401  (loads torch's libamdhip64 first, as the package does)

    lib = ctypes.CDLL(LIB)
    lib.r3dg_last_error.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+r3dg_knn_mean_dist2\s*\(\s*int\s+P\s*,\s*const\s+float\s*\*\s*points", text)
    assert hasattr(lib, "r3dg_knn_mean_dist2")
    ver = int(re.search(r"#define R3DG_ABI_VERSION (\d+)", text).group(1))
    assert ver == 2  # additive: no struct changed


def test_argument_errors_need_no_device(lib):
    """R3DG_ERR_ARG (-1) with a message before any device work; P == 0 is R3DG_OK without a launch."""
    calls = []

    @ALLOC
    def never(ctx, nbytes):
        calls.append(nbytes)
        return None

    pts, out = (ctypes.c_float * 15)(), (ctypes.c_float * 5)()
    fn = lib.r3dg_knn_mean_dist2
    fn.restype = ctypes.c_int
    bad = {"negative P": (ctypes.c_int(-1), pts, out, never, None, None),
           "null points": (ctypes.c_int(5), None, out, never, None, None),
           "null mean_dist2": (ctypes.c_int(5), pts, None, never, None, None),
           "null scratch_alloc": (ctypes.c_int(5), pts, out, None, None, None)}
    for what, args in bad.items():
        assert fn(*args) == -1, what
        assert len(lib.r3dg_last_error()) > 0, what
    assert fn(ctypes.c_int(0), None, None, None, None, None) == 0
    assert fn(ctypes.c_int(0), pts, out, never, None, None) == 0
    assert calls == []


def test_torch_binding_rejects_bad_input():
    import torch

    import relightable3dgaussian_amd as r

    assert callable(r._C.distCUDA2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        r._C.distCUDA2(torch.zeros(8, 3))
    with pytest.raises(RuntimeError, match=r"\[P,3\]"):
        r._C.distCUDA2(torch.zeros(8, 2))
    with pytest.raises(RuntimeError, match="float32"):
        r._C.distCUDA2(torch.zeros(8, 3, dtype=torch.float64))


def test_reference_import_resolves_with_integration_on_path():
    """scene/gaussian_model.py:13 `from simple_knn._C import distCUDA2`, unchanged, in a fresh process."""
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "integration"), ROOT] +
                                        [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    code = ("from simple_knn._C import distCUDA2\n"
            "import simple_knn, relightable3dgaussian_amd as r\n"
            "assert distCUDA2 is r._C.distCUDA2 and simple_knn.distCUDA2 is distCUDA2\n"
            "assert simple_knn.__file__.replace('\\\\', '/').endswith('integration/simple_knn/__init__.py')\n"
            "print('ok')\n")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout + res.stderr


def test_install_alias_registers_simple_knn():
    import relightable3dgaussian_amd as r
    from relightable3dgaussian_amd import simple_knn as ours

    r.install_alias()
    from simple_knn._C import distCUDA2

    assert distCUDA2 is r._C.distCUDA2 and ours.distCUDA2 is distCUDA2
    assert sys.modules["simple_knn._C"] is r._C


# ---- GPU ---------------------------------------------------------------------------------------------

def _run(ext, x):
    import torch

    return ext.distCUDA2(torch.from_numpy(np.array(x, np.float32)).cuda()).cpu().numpy()


# the FLT_MAX padding, the +-3 seed window at both ends, the first / last partial box (64 points: B - 1, B,
# B + 1, 2 B + 1) and the second super-box (64 boxes: 4097)
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 129, 255, 256, 257, 513, 1023, 1024, 1025, 2049, 4097, 5000]


@pytest.mark.gpu
@pytest.mark.parametrize("P", SIZES)
def test_sizes_bit_exact(hip_ext, P):
    x, ref = case(str(P))
    got = _run(hip_ext, x)
    if P <= 2:
        assert np.isposinf(got).all()
    assert_bits(got, ref, f"P={P}")


@pytest.mark.gpu
def test_empty_input(hip_ext):
    import torch

    out = hip_ext.distCUDA2(torch.zeros((0, 3), device="cuda"))
    assert out.shape == (0,) and out.dtype == torch.float32 and out.is_cuda


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["planar", "collinear", "anisotropic", "lattice", "duplicates", "clusters",
                                  "outlier", "medium", "supers"])
def test_distributions_bit_exact(hip_ext, name):
    x, ref = case(name)
    assert x.shape[0] == {"medium": 20000, "supers": 33025}.get(name, 4096)
    got = _run(hip_ext, x)
    assert np.isfinite(ref).all()
    if name == "lattice":
        assert (ref == 1.0).all()
    if name == "duplicates":
        assert (ref == 0.0).all()  # exclusion is by index: the three copies count
    assert_bits(got, ref, name)


@pytest.mark.gpu
def test_permutation_equivariance_and_determinism(hip_ext):
    x, ref = case("5000")
    perm = np.random.default_rng(11).permutation(len(x))
    a = _run(hip_ext, x)
    assert_bits(_run(hip_ext, x), a, "second call")
    assert_bits(_run(hip_ext, x[perm]), a[perm], "permuted input")
    assert_bits(a, ref, "reference")


@pytest.mark.gpu
def test_non_contiguous_input(hip_ext):
    import torch

    x, ref = case("2049")
    wide = torch.zeros((len(x), 4), device="cuda")
    wide[:, 1:] = torch.from_numpy(np.array(x)).cuda()
    sl = wide[:, 1:]
    assert not sl.is_contiguous()
    got = hip_ext.distCUDA2(sl)
    assert got.shape == (len(x),) and got.dtype == torch.float32 and got.device == wide.device
    assert_bits(got.cpu().numpy(), hip_ext.distCUDA2(sl.contiguous()).cpu().numpy(), "slice vs copy")
    assert_bits(got.cpu().numpy(), ref, "reference")


@pytest.mark.gpu
def test_other_stream(hip_ext):
    import torch

    x, ref = case("5000")
    xt = torch.from_numpy(np.array(x)).cuda()
    base = hip_ext.distCUDA2(xt)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = hip_ext.distCUDA2(xt)
    s.synchronize()
    assert_bits(other.cpu().numpy(), base.cpu().numpy(), "side stream vs default")
    assert_bits(other.cpu().numpy(), ref, "reference")


@pytest.mark.gpu
def test_raw_c_abi(hip_ext, lib):
    """r3dg_knn_mean_dist2 through ctypes on device pointers, scratch from a torch-backed callback."""
    import torch

    x, ref = case("5000")
    pts = torch.from_numpy(np.array(x)).cuda()
    out = torch.empty(len(x), device="cuda")
    keep = []

    @ALLOC
    def torch_alloc(ctx, nbytes):
        t = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        keep.append(t)
        return t.data_ptr()

    lib.r3dg_knn_mean_dist2.restype = ctypes.c_int
    rc = lib.r3dg_knn_mean_dist2(ctypes.c_int(len(x)), ctypes.c_void_p(pts.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                 torch_alloc, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.r3dg_last_error()
    torch.cuda.synchronize()
    assert len(keep) == 1 and keep[0].numel() >= 32 * len(x)
    assert_bits(out.cpu().numpy(), ref, "raw ABI")


def _opt_args():
    return types.SimpleNamespace(
        percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
        position_lr_max_steps=30000, normal_lr=0.01, rotation_lr=0.001, scaling_lr=0.005, opacity_lr=0.05,
        sh_lr=0.0025, base_color_lr=0.01, roughness_lr=0.01, metallic_lr=0.01, light_lr=0.002, light_rest_lr=-1.0,
        visibility_lr=0.0025, visibility_rest_lr=-1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("as_numpy", [True, False])
def test_create_from_pcd(hip_ext, as_numpy):
    """GaussianModel.create_from_pcd (gaussian_model.py:537-580) into the flat buffer, group by group."""
    import torch

    from relightable3dgaussian_amd import trainer

    P = 1000
    rng = np.random.default_rng(12)
    pts, col = rng.random((P, 3), dtype=np.float32), rng.random((P, 3), dtype=np.float32)
    nrm = rng.normal(size=(P, 3)).astype(np.float32)
    args = (pts, col, nrm) if as_numpy else tuple(torch.from_numpy(a) for a in (pts, col, nrm))
    st = trainer.GaussianTrainState.create_from_pcd(*args, spatial_lr_scale=2.5)

    xyz, color = torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda()
    d2 = hip_ext.distCUDA2(xyz)
    assert_bits(d2.cpu().numpy(), brute_force(pts), "distCUDA2")
    opac = 0.1 * torch.ones((P, 1), dtype=torch.float, device="cuda")
    expect = {"xyz": xyz, "normal": torch.from_numpy(nrm).cuda(),
              "rotation": torch.tensor([1.0, 0.0, 0.0, 0.0], device="cuda").repeat(P, 1),
              "scaling": torch.log(torch.sqrt(torch.clamp_min(d2, 0.0000001)))[..., None].repeat(1, 3),
              "opacity": torch.log(opac / (1 - opac)),
              "f_dc": ((color - 0.5) / 0.28209479177387814)[:, None, :],
              "f_rest": torch.zeros((P, 15, 3), device="cuda")}
    expect.update({n: torch.zeros((P, *s), device="cuda") for n, s in trainer.PBR_GROUPS})
    ref = trainer.GaussianTrainState.from_tensors(expect, use_pbr=True)
    assert st.P == ref.P == P and st.groups == ref.groups == trainer.BASE_GROUPS + trainer.PBR_GROUPS
    assert st.param.shape == ref.param.shape and st.exp_avg.shape == ref.exp_avg.shape
    for n, s in st.groups:
        v = st.view(n)
        assert tuple(v.shape) == (P, *s), n
        assert_bits(v.cpu().numpy().reshape(-1), expect[n].cpu().numpy().reshape(-1), n)
    assert torch.isfinite(st.view("scaling")).all()
    for stat in ("xyz_gradient_accum", "normal_gradient_accum", "denom", "max_radii2D"):
        a, b = getattr(st, stat), getattr(ref, stat)
        assert a.shape == b.shape and not a.any(), stat
    assert not st.exp_avg.any() and not st.exp_avg_sq.any() and st.step_count == 0

    base = trainer.GaussianTrainState.create_from_pcd(*args, use_pbr=False)
    assert base.groups == trainer.BASE_GROUPS and base.spatial_lr_scale == 1.0
    assert_bits(base.view("scaling").cpu().numpy().reshape(-1), expect["scaling"].cpu().numpy().reshape(-1), "no pbr")

    # the stored spatial_lr_scale reaches training_setup; one optimizer step runs
    st.training_setup(_opt_args())
    names = [n for n, _ in st.groups]
    assert st.lrs[names.index("xyz")] == pytest.approx(0.00016 * 2.5)
    before = st.param[:st.total()].clone()
    st.grad[:st.total()] = 1.0
    st.step()
    after = st.param[:st.total()]
    assert torch.isfinite(after).all() and (after != before).all()
