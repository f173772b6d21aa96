"""In-tree build of the HIP library and the torch binding.

Produces (git-ignored, but shipped to the GPU box with the tree):
  relightable3dgaussian_amd/lib/libr3dg_hip.so   -- HIP kernels + the C ABI of include/r3dg_hip.h
  relightable3dgaussian_amd/lib/_C.so             -- pybind module mirroring r3dg_rasterization._C

`python relightable3dgaussian_amd/build.py` rebuilds what is out of date. hipcc cross-compiles
for gfx950 without a GPU, so this runs in the CPU container too.
"""
from __future__ import annotations

import os
import subprocess
import sys
import sysconfig
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
# experiment builds put their objects / libraries elsewhere (tools/exp_build.sh)
LIB = os.environ.get("R3DG_LIB_DIR") or os.path.join(PKG, "lib")
INC = os.path.join(ROOT, "include")
OBJ = os.environ.get("R3DG_OBJ_DIR") or os.path.join(PKG, "build", "obj")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.path.join(ROCM, "bin", "hipcc")

HIP_SOURCES = ["preprocess.hip", "render_fwd.hip", "render_bwd.hip", "brdf.hip", "shaders.hip", "rasterizer.hip",
               "optim.hip", "bvh.hip", "knn.hip", "loss.hip", "reg_loss.hip", "relight.hip", "visibility.hip",
               "activation.hip", "compose.hip", "pbr_head.hip", "display.hip"]
# the torch binding: binding.h is shared, module.cpp holds PYBIND11_MODULE, the others one operator family each
BINDING = os.path.join(CSRC, "binding")
BINDING_SOURCES = ["module.cpp", "rasterizer.cpp", "render_equation.cpp", "training.cpp", "losses.cpp", "bvh.cpp", "pbr.cpp",
                   "display.cpp"]
HIP_FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-result",
             "-munsafe-fp-atomics", f"-I{INC}", f"-I{CSRC}"]
# the key path (projection, radius, rect) must not contract a*b+c into fma: see preprocess.hip
# render_bwd: the SLP vectorizer pairs the two unrolled blend steps into packed f32 ops plus
# register shuffles (more instructions, 30 more VGPRs); plain scalar code measures faster; in
# render_fwd it packs the blend's channel sums into v_pk_fma_f32 (4 cycles each, as two v_fma_f32):
# scalar FMAs measured 1.5 % faster; brdf.hip: the BRDF forwards 1.5-2 % faster unpacked
# brdf.hip: the render equation restates the oracle's operation sequence (no a*b+c contraction), so
# the BRDF outputs are bit-identical to it
# render_bwd.hip: the max-memory-clause scheduling strategy (same registers): render_bwd -0.3 %,
# gather -1.5 % at M1 (round 5; max-ilp: +17 %, iterative-ilp: +1 %)
# knn.hip: d2 = (dx*dx + dy*dy) + dz*dz uncontracted, so a numpy-f32 brute force is its bit-exact reference
# loss.hip: the per-pixel SSIM arithmetic rounds every operation, as the reference's tensor operations do, so
# that identical images give ssim_map == 1 and a gradient of exactly 0 (a contracted a*b+c breaks the
# cancellation: 1.2e-4 of a pixel's share measured); its filter loops call fmaf themselves
# reg_loss.hip: the two sides of a Sobel difference are added in one order and must stay equal for equal
# means (a contracted 2*b+c on one side only breaks the exact zero); the upstream scale multiplies last
# relight.hip: its float32 reference is the reference's torch tensor code, which rounds every operation; the
# BRDF, direction and texture-coordinate expressions stay uncontracted so that they round where it does (the
# sample angle delta * r above all: 6e-5 rad of rounding at r = 383 that the reference has too). Only the SH
# sums are FMAs, written as such. No other flag: nothing measured yet that would justify one
# visibility.hip: the hemisphere flip's dot product and eval_sh's products round one operation at a time, as
# the reference's tensor code, so a float32 numpy restatement decides the flip and forms the basis bit for bit
# (csrc/sh_dirs.h is shared with bvh.hip and relight.hip, both uncontracted as well)
# activation.hip: its float32 reference is the getters' torch tensor code, which rounds every operation (the
# squared norms, the rotation matrix, L L^T and the normalise gradient's projection stay uncontracted)
# compose.hip: the same reason and the same device functions (csrc/act_device.h): its reference is set_transform's
# and the getters' torch tensor code, and a composed activation must have activation.hip's bits
# pbr_head.hip: the composite x = pbr + (1 - opacity) * bg is three torch tensor operations in the reference, each
# rounded on its own; uncontracted, the "none" and "clamp" images are the reference's bits (a contracted
# fma(1 - opacity, bg, pbr) rounds once and differs in the last bit), and ACES rounds where hdr2ldr does
# display.hip: the same reason and the same tone functions (csrc/tone_device.h): every mode is two to four torch
# tensor operations in the reference (s * 0.5 + 0.5, (1 - opacity) * bg, y * 255 + 0.5), each rounded on its own;
# uncontracted, the float32 and the 8-bit images are the reference's bits (a contracted fma(y, 255, 0.5) moves a
# value that sits half a float32 step under a half-way point into the next byte)
PER_FILE_FLAGS = {"preprocess.hip": ["-ffp-contract=off"], "bvh.hip": ["-ffp-contract=off"],
                  "visibility.hip": ["-ffp-contract=off"], "activation.hip": ["-ffp-contract=off"],
                  "compose.hip": ["-ffp-contract=off"], "pbr_head.hip": ["-ffp-contract=off"],
                  "display.hip": ["-ffp-contract=off"],
                  "knn.hip": ["-ffp-contract=off"], "loss.hip": ["-ffp-contract=off"],
                  "reg_loss.hip": ["-ffp-contract=off"], "relight.hip": ["-ffp-contract=off"],
                  "brdf.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
                  "render_bwd.hip": ["-fno-slp-vectorize", "-mllvm", "-amdgpu-sched-strategy=max-memory-clause"],
                  "render_fwd.hip": ["-fno-slp-vectorize"]}


def _newer(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd: list[str]) -> None:
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("build failed: " + " ".join(cmd[:3]) + " ...")


def _headers() -> list[str]:
    hs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return hs + [os.path.join(INC, "r3dg_hip.h")]


def build_hip(jobs: int = 8) -> str:
    os.makedirs(OBJ, exist_ok=True)
    os.makedirs(LIB, exist_ok=True)
    hdrs = _headers()
    objs, cmds = [], []
    for src in HIP_SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.replace(".hip", ".o"))
        objs.append(o)
        if _newer(o, [s] + hdrs + [__file__]):
            extra = os.environ.get("R3DG_EXTRA_HIPFLAGS", "").split()  # experiment builds only
            cmds.append([HIPCC, "-c", s, "-o", o] + HIP_FLAGS + PER_FILE_FLAGS.get(src, []) + extra)
    with ThreadPoolExecutor(max(1, jobs)) as ex:
        list(ex.map(_run, cmds))
    so = os.path.join(LIB, "libr3dg_hip.so")
    if _newer(so, objs):
        _run([HIPCC, "-shared", "-o", so, *objs, "--offload-arch=gfx950", "-fPIC",
              "-Wl,-soname,libr3dg_hip.so"])
    return so


def build_torch_ext(jobs: int = 8) -> str:
    """pybind module `_C` (csrc/binding/: one source per operator family) linked against libr3dg_hip.so.

    A binding object depends on its source, the shared binding.h and the C ABI header only: the kernels'
    headers are not its business."""
    import torch
    from torch.utils import cpp_extension

    os.makedirs(OBJ, exist_ok=True)
    os.makedirs(LIB, exist_ok=True)
    inc = cpp_extension.include_paths() + [sysconfig.get_paths()["include"], INC, os.path.join(ROCM, "include")]
    abi = int(torch._C._GLIBCXX_USE_CXX11_ABI)
    flags = ["-O2", "-std=c++17", "-fPIC", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1", "-DTORCH_EXTENSION_NAME=_C",
             "-DTORCH_API_INCLUDE_EXTENSION_H", f"-D_GLIBCXX_USE_CXX11_ABI={abi}", "-Wno-deprecated-declarations"]
    flags += [f"-I{p}" for p in inc]
    deps = [os.path.join(BINDING, "binding.h"), os.path.join(INC, "r3dg_hip.h"), __file__]
    objs, cmds = [], []
    for src in BINDING_SOURCES:
        s = os.path.join(BINDING, src)
        o = os.path.join(OBJ, "binding_" + src.replace(".cpp", ".o"))
        objs.append(o)
        if _newer(o, [s] + deps):
            cmds.append(["g++", "-c", s, "-o", o] + flags)
    with ThreadPoolExecutor(max(1, jobs)) as ex:
        list(ex.map(_run, cmds))
    so = os.path.join(LIB, "_C.so")
    if _newer(so, objs + [os.path.join(LIB, "libr3dg_hip.so")]):
        tlib = os.path.join(os.path.dirname(torch.__file__), "lib")
        _run(["g++", "-shared", "-o", so, *objs, f"-L{LIB}", "-lr3dg_hip", f"-L{tlib}", "-ltorch", "-ltorch_cpu",
              "-ltorch_python", "-lc10", "-lc10_hip", "-ltorch_hip", "-Wl,-rpath,$ORIGIN", f"-Wl,-rpath,{tlib}"])
    return so


def build(jobs: int = 8, torch_ext: bool = True) -> None:
    build_hip(jobs)
    if torch_ext:
        build_torch_ext(jobs)


if __name__ == "__main__":
    build()
    print("built", os.listdir(LIB))
