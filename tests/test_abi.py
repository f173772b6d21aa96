"""CPU tests of the drop-in boundary: the C-ABI library (include/r3dg_hip.h) and the `_C` module
that mirrors the reference's pybind surface. No kernels run here (no GPU in the build container);
the compute entry points are exercised by the -m gpu parity tests."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "r3dg_hip.h")
LIB = os.path.join(ROOT, "relightable3dgaussian_amd", "lib", "libr3dg_hip.so")

# the reference's pybind module (r3dg-rasterization/ext.cpp via setup.py "r3dg_rasterization._C")
REFERENCE_C_FUNCTIONS = [
    "rasterize_gaussians", "rasterize_gaussians_backward", "render_equation_forward",
    "render_equation_forward_complex", "render_equation_backward", "mark_visible", "GetSplatShaderAddressMap",
    "GetShShaderAddressMap", "GetPostProcessShaderAddressMap", "PreprocessModel", "EncodeTextureMode",
    "EncodeWrapMode", "AllocateTexture", "UploadTexturesToDevice",
]


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(r3dg_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m relightable3dgaussian_amd.build")
    import torch  # noqa: F401  (loads torch's libamdhip64 first, as the package does)

    return ctypes.CDLL(LIB)


def test_library_exports_every_declared_symbol(lib):
    names = _declared()
    assert len(names) >= 20
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_abi_version_and_error_string(lib):
    lib.r3dg_abi_version.restype = ctypes.c_int
    text = open(HEADER).read()
    ver = int(re.search(r"#define R3DG_ABI_VERSION (\d+)", text).group(1))
    assert lib.r3dg_abi_version() == ver
    lib.r3dg_last_error.restype = ctypes.c_char_p
    assert isinstance(lib.r3dg_last_error(), bytes)


@pytest.mark.parametrize("S,groups", [(21, [1, 1, 1, 3, 3, 3, 3, 3, 3]), (11, [1, 1, 3, 3, 3]), (0, []),
                                      (3, [1, 1, 1]), (16, [1] * 16)])
def test_feature_groups(lib, S, groups):
    """forward.cu:537-558 channel grouping of the feature output (S=21 reference layout)."""
    buf = (ctypes.c_int * 32)()
    n = lib.r3dg_feature_groups(S, buf)
    assert list(buf[:n]) == groups
    import oracle

    a, m = oracle.feature_layout(S, 7 * 5)
    # layout derived from the groups: group g occupies [H,W,g] after the previous groups
    off, exp_a, exp_m = 0, [], []
    for gsz in groups:
        for k in range(gsz):
            exp_a.append(off + k)
            exp_m.append(gsz)
        off += gsz * 35
    assert list(a) == exp_a and list(m) == exp_m


def test_shader_registry(lib):
    """Name -> handle maps (ShShader.cu:201-230, splatShader.cu:284-333, postProcessShader.cu)."""
    lib.r3dg_shader_name.restype = ctypes.c_char_p
    lib.r3dg_shader_handle.restype = ctypes.c_int64
    seen = set()
    for kind, default in [(0, b"ShDefault"), (1, b"SplatDefault"), (2, None)]:
        n = lib.r3dg_shader_count(kind)
        assert n > 0
        names = [lib.r3dg_shader_name(kind, i) for i in range(n)]
        assert names == sorted(names)  # std::map iteration order, as pybind returns the dict
        if default:
            assert default in names
        for i in range(n):
            h = lib.r3dg_shader_handle(kind, i)
            assert h != 0 and h not in seen
            seen.add(h)
    assert lib.r3dg_shader_count(7) < 0 or lib.r3dg_shader_count(7) == 0


def test_encode_modes(lib):
    assert lib.r3dg_encode_texture_mode(b"RGB") == 3
    assert lib.r3dg_encode_texture_mode(b"nope") == -1
    assert lib.r3dg_encode_wrap_mode(b"Wrap") >= 0
    assert lib.r3dg_encode_wrap_mode(b"nope") == -1


def test_torch_module_mirrors_reference_surface():
    import relightable3dgaussian_amd as r

    for name in REFERENCE_C_FUNCTIONS:
        assert hasattr(r._C, name), name
    assert r._C.abi_version() == ctypes.CDLL(LIB).r3dg_abi_version()
    sh = r._C.GetShShaderAddressMap()
    assert "ShDefault" in sh and "ExpPos" in sh
    assert "SplatDefault" in r._C.GetSplatShaderAddressMap()
    assert r._C.EncodeTextureMode("RGBA") == 4
    assert r._C.feature_groups(11) == [1, 1, 3, 3, 3]


def test_alias_makes_reference_import_work():
    """`import r3dg_rasterization` (gaussian_renderer/__init__.py) resolves to this build."""
    import sys

    import relightable3dgaussian_amd as r

    r.install_alias()
    import r3dg_rasterization

    assert r3dg_rasterization is sys.modules["r3dg_rasterization"]
    for name in ["GaussianRasterizationSettings", "GaussianRasterizer", "RenderEquation", "RenderEquation_complex"]:
        assert hasattr(r3dg_rasterization, name), name
    assert r3dg_rasterization._C is r._C


# gaussian_renderer/r3dg_rasterization.py:198-222, the NamedTuple's 24 fields in order
REFERENCE_SETTINGS_FIELDS = (
    "image_height", "image_width", "tanfovx", "tanfovy", "cx", "cy", "bg", "scale_modifier", "viewmatrix",
    "viewmatrix_inv", "projmatrix", "projmatrix_inv", "sh_degree", "campos", "prefiltered", "backward_geometry",
    "computer_pseudo_normal", "debug", "h_shShaderManager_ptr", "h_splatShaderManager_ptr", "time", "dt",
    "d_textureManager_ptr", "postProcessingPasses")


def test_settings_fields_match_reference():
    """GaussianRasterizationSettings: the reference's 24 fields, same names, same order (neilf.py
    constructs it by keyword, _RasterizeGaussians reads it by attribute)."""
    from relightable3dgaussian_amd.r3dg_rasterization import GaussianRasterizationSettings

    assert GaussianRasterizationSettings._fields == REFERENCE_SETTINGS_FIELDS


# bound names that take no tensor, and the two that take host data by design
NO_TENSOR_FUNCTIONS = {
    "GetSplatShaderAddressMap", "GetShShaderAddressMap", "GetPostProcessShaderAddressMap", "EncodeTextureMode",
    "EncodeWrapMode", "UploadTexturesToDevice", "feature_groups", "shader_manager_info", "abi_version", "get_options",
    "set_options", "image_loss_window", "profile_enable", "profile_read"}
HOST_DATA_FUNCTIONS = {"AllocateTexture", "create_shader_manager"}


def _host_calls():
    """{bound name: a well-shaped argument list, every tensor on the host}."""
    import torch

    P, H, W, S, M, Ns, R = 4, 8, 8, 3, 16, 6, 5

    def f(*shape):
        return torch.zeros(*shape)

    def i32(*shape):
        return torch.zeros(*shape, dtype=torch.int32)

    eye, state = torch.eye(4), torch.zeros(256, dtype=torch.uint8)
    backward = (f(3), f(P, 3), f(P, S), i32(P), f(0), f(P, 3), f(P, 4), 1.0, f(0), eye, eye, 1.0, 1.0, f(3, H, W),
                f(1, H, W), f(1, H, W), f(S, H, W), f(P, M, 3), 3, f(3), state, 0, state, state, True, False)
    brdf = (f(P, 3), f(P, 1), f(P, 1), f(P, 3), f(P, 3), f(P, M, 3), f(1, M, 3), f(P, M, 1))
    widths, roles, groups = [3, 3, 4, 1], [0, 1, 2, 3], [-1] * 10
    n = P * sum(widths)
    layout = (P, widths, roles)
    one, three = f(1, H, W), f(3, H, W)
    maps = [one, one, three, three, three, one, one, three, one, one, three]
    vis = (f(P, 1, 1), f(P, M - 1, 1), f(P, 3), f(P), None)
    nodes, aabbs = i32(2 * P - 1, 5), f(2 * P - 1, 6)
    gaussians = (f(P, 3), f(P, 6), f(P))
    return {
        "rasterize_gaussians": (f(3), 0.0, 0.0, f(P, 3), f(P, S), f(0), f(P, 1), f(P, 3), f(P, 4), 1.0, f(0), eye, eye,
                                eye, eye, 1.0, 1.0, 4.0, 4.0, H, W, f(P, M, 3), 3, f(3), False, False, None, None, None,
                                None, False),
        "rasterize_gaussians_backward": backward,
        "rasterize_gaussians_backward_ex": backward + (H, W),
        "rasterize_gaussians_backward_chunked": backward + (H, W, True, True, 1, None),
        "rasterize_gaussians_backward_chunked_packed": backward + (H, W, True, True, 1, None),
        "mark_visible": (f(P, 3), eye, eye),
        "PreprocessModel": (f(P, 3),),
        "rasterizer_state": (state, state, state, P, H, W, 0),
        "sh_color_grads": (state, P, f(P, 3), 0, P),
        "sh_grad_from_views": (f(P, 3), f(2, 3), f(2, P, 3), 3, 0, f(P, M, 3)),
        "render_equation_forward": brdf + (Ns, False, False),
        "render_equation_forward_with_rand": brdf + (Ns, False, f(P, Ns, 1)),
        "render_equation_forward_complex": brdf + (Ns,),
        "render_equation_backward": brdf + (Ns, f(P, Ns, 3), f(P, 3), f(P, 3), False),
        "render_equation_relight": brdf + (Ns, 1, None, None, None),
        "envmap_direct_light": (f(R, 3), f(4, 8, 3), None),
        "adam_step": layout + (f(n), f(n), f(n), f(n), 0, n, [1e-3] * 4, 0.9, 0.999, 1e-15, 1),
        "adam_step_groups": layout + (f(n), f(n), f(n), f(n), 0, n, [1e-3] * 4, 0.9, 0.999, 1e-15, [1] * 4),
        "densification_stats": (f(P, 3), f(0), i32(P), f(P, 1), f(P, 1), f(P, 1), f(P)),
        "densify_and_prune": layout + (f(n), f(n), f(n), f(P, 1), f(P, 1), f(P, 1), f(0), 0.1, 0.1, 0.01, 1.0, 0.005,
                                       0.0, 2, False, f(0)),
        "reset_opacity": layout + (f(n), f(n), f(n)),
        "activate_forward": layout + (groups, f(n), None, False),
        "activate_backward": layout + (groups, f(n), None, [None] * 12, f(n), False),
        "set_transform": layout + (-1, f(n), None, 0),
        "compose_object": layout + (groups, f(n), None, 0, [None] * 13, 0),
        "render_points": (f(P, 3), f(P, 3), eye, f(3, 3), H, W, None, [0.0, 0.0, 0.0], False),
        "image_loss_forward": (three, three, False, True),
        "image_loss_backward": (three, three, False, f(3, 3, H, W), f(3), f(3), None),
        "reg_loss_forward": (maps, H, W, 255, False),
        "reg_loss_backward": (maps, H, W, 255, False, i32(1), f(8), None, 63),
        "visibility_sh_loss_forward": vis + (None,),
        "visibility_sh_loss_backward": vis + (None, f(1)),
        "visibility_sh_fit_step": vis + (f(P, 1, 1), f(P, M - 1, 1), f(P, 1, 1), f(P, M - 1, 1), 1, 1e-3, 0.9, 0.999,
                                         1e-8, f(4), 0),
        "create_bvh": (f(P, 3), f(P, 3), f(P, 4), nodes, aabbs),
        "trace_bvh": (nodes, aabbs, f(R, 3), f(R, 3)) + gaussians,
        "trace_bvh_opacity": (nodes, aabbs, f(R, 3), f(R, 3)) + gaussians + (f(P, 3),),
        "trace_bvh_opacity_centres": (nodes, aabbs, None) + gaussians + (f(P, 3),),
        "bvh_leaf_aabbs": (f(P, 3), f(P, 3), f(P, 4)),
        "fibonacci_dirs": (f(P, 3), 4),
        "distCUDA2": (f(8, 3),),
    }


def test_host_call_table_covers_every_bound_function():
    import relightable3dgaussian_amd as r

    bound = {n for n in dir(r._C) if not n.startswith("_") and callable(getattr(r._C, n))}
    assert bound == set(_host_calls()) | NO_TENSOR_FUNCTIONS | HOST_DATA_FUNCTIONS


def test_host_tensors_refused_before_any_hip_call():
    """There is no CPU path: every bound function that takes a tensor refuses well-shaped host tensors with
    its own check ("... must be a GPU tensor ..."), not with whatever the HIP runtime says when a host
    pointer or a host device index reaches it."""
    import relightable3dgaussian_amd as r

    wrong = {}
    for name, args in sorted(_host_calls().items()):
        try:
            getattr(r._C, name)(*args)
            wrong[name] = "no error"
        except RuntimeError as e:
            if "GPU tensor" not in str(e):
                wrong[name] = str(e).splitlines()[0]
        except Exception as e:  # any other type is not the binding's own refusal
            wrong[name] = f"{type(e).__name__}: {e}"
    assert not wrong, wrong


def test_product_package_never_imports_oracle():
    """Only tests/, smoke() and bench.py's cpu_baseline may touch oracle/."""
    pkg = os.path.join(ROOT, "relightable3dgaussian_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                bad = re.findall(r"^\s*(?:import oracle|from oracle|#include [\"<].*oracle.*)|libr3dg_oracle", text,
                                 flags=re.M)
                assert not bad, (f, bad)


def test_integration_shim_package():
    """integration/r3dg_rasterization is importable under the reference's package name."""
    import subprocess
    import sys

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "integration")]))
    code = ("from r3dg_rasterization import _C, GaussianRasterizer, RenderEquation; "
            "import relightable3dgaussian_amd as r; assert _C is r._C; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_integration_shim_bvh_packages():
    """integration/bvh and integration/bvh_tracing import under the reference's package names."""
    import subprocess
    import sys

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "integration")]))
    code = ("from bvh import RayTracer; from bvh_tracing import _C; import relightable3dgaussian_amd as r; "
            "assert _C is r._C and RayTracer is r.bvh.RayTracer; "
            "assert all(hasattr(_C, n) for n in ('create_bvh', 'trace_bvh', 'trace_bvh_opacity')); print('ok')")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_options_roundtrip_and_validation(lib):
    """r3dg_get_options / r3dg_set_options (include/r3dg_hip.h): the library reads no environment
    variable on a launch; the test / experiment variants are switched through this struct, whose
    struct_size and ranges are checked."""
    from tests import _abi_ctypes as A

    A.bind(lib)
    cur = A.new(A.Options)
    assert lib.r3dg_get_options(ctypes.byref(cur)) == 0, lib.r3dg_last_error()
    want = "rows" if os.environ.get("R3DG_BWD_REDUCE", "").startswith("r") else "atomic"
    assert cur.bwd_reduce == (1 if want == "rows" else 0)  # the one option seeded from the environment
    assert all(getattr(cur, f) == 0 for f in A.OPTION_FIELDS if f != "bwd_reduce")
    try:
        new = A.new(A.Options, bwd_reduce=1, test_no_cull=1, test_bwd_wterms=3, test_bvh_lanes=8)
        assert lib.r3dg_set_options(ctypes.byref(new)) == 0, lib.r3dg_last_error()
        got = A.new(A.Options)
        assert lib.r3dg_get_options(ctypes.byref(got)) == 0
        assert [getattr(got, f) for f in A.OPTION_FIELDS] == [getattr(new, f) for f in A.OPTION_FIELDS]
        for bad in (dict(struct_size=0), dict(struct_size=ctypes.sizeof(A.Options) + 8), dict(bwd_reduce=2),
                    dict(test_bwd_wterms=2), dict(test_bvh_lanes=65), dict(test_bwd_srs=-1), dict(test_bvh_sort=3)):
            o = A.new(A.Options, **bad)
            assert lib.r3dg_set_options(ctypes.byref(o)) == -1, bad
            assert lib.r3dg_last_error()
        assert lib.r3dg_get_options(ctypes.byref(got)) == 0  # refused sets change nothing
        assert [getattr(got, f) for f in A.OPTION_FIELDS] == [getattr(new, f) for f in A.OPTION_FIELDS]
        stale = A.new(A.Options, struct_size=8)
        assert lib.r3dg_get_options(ctypes.byref(stale)) == -1
    finally:
        assert lib.r3dg_set_options(ctypes.byref(cur)) == 0


def test_raster_structs_checked_before_any_launch(lib):
    """ABI 2: r3dg_raster_settings and r3dg_backward_outputs start with struct_size, and a struct
    that is not this header's (struct_size 0 from a caller that zero-initialises an older layout, or
    garbage) is refused with R3DG_ERR_ARG before any device work -- which is why this runs on the
    CPU. dense_stride must be 0 or exactly 11 + S (round 5's appended field)."""
    from tests import _abi_ctypes as A

    A.bind(lib)
    nr = ctypes.c_int(-1)
    alloc = A.ALLOC(lambda ctx, n: None)
    for size in (0, ctypes.sizeof(A.RasterSettings) - 8, 12345):
        s = A.new(A.RasterSettings, P=10, S=3, W=16, H=16)
        s.struct_size = size
        rc = lib.r3dg_rasterize_gaussians_ex(ctypes.byref(s), ctypes.byref(A.Gaussians()),
                                             ctypes.byref(A.ForwardOutputs()), alloc, None, alloc, None, alloc, None,
                                             alloc, None, ctypes.byref(nr), None)
        assert rc == -1 and b"struct_size" in lib.r3dg_last_error(), size
    s = A.new(A.RasterSettings, P=10, S=3, W=16, H=16)
    gr = A.BackwardGrads()
    for kw in (dict(struct_size=0), dict(struct_size=ctypes.sizeof(A.BackwardOutputs) - 8), dict(dense_stride=1),
               dict(dense_stride=15), dict(dense_stride=1 << 20)):
        out = A.new(A.BackwardOutputs, **kw)
        rc = lib.r3dg_rasterize_gaussians_backward(ctypes.byref(s), ctypes.byref(A.Gaussians()), None,
                                                   ctypes.byref(gr), None, None, None, 0, 1, alloc, None,
                                                   ctypes.byref(out), None)
        assert rc == -1, kw
        msg = lib.r3dg_last_error()
        assert (b"struct_size" in msg) if "struct_size" in kw else (b"dense_stride" in msg), (kw, msg)


def _kernel_resources():
    """{demangled kernel name: metadata} of every gfx950 kernel in the built library (its
    .hip_fatbin section holds one offload bundle per source file)."""
    import subprocess
    import tempfile

    import yaml

    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(f"{llvm}/llvm-readelf"):
        pytest.skip("ROCm llvm tools not found")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([f"{llvm}/llvm-objcopy", f"--dump-section=.hip_fatbin={d}/fb.bin", LIB], check=True)
        data = open(f"{d}/fb.bin", "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts, i = [], data.find(magic)
        while i >= 0:
            starts.append(i)
            i = data.find(magic, i + 1)
        for n, s in enumerate(starts):
            e = starts[n + 1] if n + 1 < len(starts) else len(data)
            open(f"{d}/b{n}.bin", "wb").write(data[s:e])
            subprocess.run([f"{llvm}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={d}/b{n}.bin",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={d}/k{n}.co"], check=True)
            notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f"{d}/k{n}.co"], check=True,
                                   capture_output=True, text=True).stdout
            if "---" not in notes:
                continue
            meta = yaml.safe_load(notes[notes.index("---"):notes.rindex("...") + 3])
            for k in meta.get("amdhsa.kernels", []):
                name = subprocess.run(["c++filt", k[".name"]], capture_output=True, text=True).stdout.strip()
                out[name] = k
    return out


def test_blend_kernel_occupancy_budget():
    """The blend kernels' occupancy is set by registers and LDS together; a code or
    compiler change that tips one over a step would silently lose a wave per SIMD. Pinned here from
    the built code objects: render_bwd_glds_kernel<11, true, 2> (M1's backward) <= 128 VGPRs and
    <= 40 KiB of LDS (4 workgroups = 4 waves per SIMD), render_fwd_glds_kernel<11, false> <= 64
    VGPRs, <= 80 SGPRs (MI355X_MICROARCH.md: 82-96 SGPRs admit 7 workgroups of 256 per CU) and
    <= 20 KiB of LDS (8 waves per SIMD); neither spills."""
    res = _kernel_resources()
    budgets = {"void r3dg::render_bwd_glds_kernel<11, true, 2>(r3dg::RenderBwdArgs)": (128, 102, 40960),
               "void r3dg::render_fwd_glds_kernel<11, false>(r3dg::RenderFwdArgs)": (64, 80, 20480)}
    for name, (vg, sg, lds) in budgets.items():
        assert name in res, (name, sorted(k for k in res if "render_" in k))
        k = res[name]
        print(f"{name}: vgpr {k['.vgpr_count']} sgpr {k['.sgpr_count']} lds {k['.group_segment_fixed_size']}")
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= vg, name
        assert k[".sgpr_count"] <= sg, name
        assert k[".group_segment_fixed_size"] <= lds, name
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
        assert k[".private_segment_fixed_size"] == 0, name
