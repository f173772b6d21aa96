"""sha256 of the gfx950 .text and .rodata of every HIP source, built with build.py's flags.

    python tools/device_code_digest.py [TREE_ROOT]

A refactor that must not change a kernel runs this on a checkout of the parent commit and on the
branch: equal hashes mean the device code is byte-identical. (Whole object files always differ:
paths and the host part.) Needs hipcc and the LLVM binutils of ROCm; no GPU.
"""
import hashlib
import importlib.util
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
os.environ.pop("R3DG_EXTRA_HIPFLAGS", None)
spec = importlib.util.spec_from_file_location("r3dg_build", os.path.join(root, "relightable3dgaussian_amd", "build.py"))
b = importlib.util.module_from_spec(spec)
spec.loader.exec_module(b)
LLVM = os.path.join(b.ROCM, "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def digest(src: str, tmp: str) -> str:
    p = os.path.join(tmp, src[:-4])
    run = lambda *cmd: subprocess.run(cmd, check=True)
    run(b.HIPCC, "-c", os.path.join(b.CSRC, src), "-o", p + ".o", *b.HIP_FLAGS, *b.PER_FILE_FLAGS.get(src, []))
    if subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={p}.fatbin", p + ".o"],
                      stderr=subprocess.DEVNULL).returncode:
        return f"{src:16s} (host code only: no device section)"
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
        f"--input={p}.fatbin", f"--output={p}.co")
    run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".text={p}.text",
        "--dump-section", f".rodata={p}.rodata", p + ".co")
    sha = lambda ext: hashlib.sha256(open(p + ext, "rb").read()).hexdigest()
    return f"{src:16s} {sha('.text')}  {sha('.rodata')}"


with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as ex:
    for line in ex.map(lambda s: digest(s, tmp), b.HIP_SOURCES):
        print(line)
