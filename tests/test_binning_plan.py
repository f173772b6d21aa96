"""CPU tests of the binning's plan: its LDS budget from the built code objects, the Python mirror of the
host's path choice (tests/_binning_cases.py) against the constants of r3dg_kernels.h and preprocess.hip, and
the coverage check of every scene the GPU tests (tests/test_gpu_binning_bands.py) run."""
from __future__ import annotations

import os
import re

import pytest

from tests import _binning_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "relightable3dgaussian_amd", "csrc")
BIN_KERNELS = ["r3dg::bin_count_kernel(r3dg::BinArgs)",
               "r3dg::bin_scatter_kernel(r3dg::BinArgs, HIP_vector_type<unsigned int, 2u> const*, unsigned int*)"]


def _text(name):
    return open(os.path.join(CSRC, name)).read()


def _constant(text, name, env):
    """The value of `constexpr int <name> = <integer expression of earlier constants>;`."""
    m = re.search(rf"constexpr\s+int\s+{name}\s*=\s*([^;]+);", text)
    assert m, name
    expr = m.group(1)
    assert re.fullmatch(r"[\w\s()+\-*/<]+", expr), expr
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(env)))  # noqa: S307 (checked above)


def test_mirror_matches_header():
    """The mirror's constants are the header's literals, kBinMaxTiles its expression, and the thresholds of
    launch_bin_prepare / allow_lds / bin_lds_bytes those of preprocess.hip."""
    h = _text("r3dg_kernels.h")
    env = {}
    for name, mine in [("kBinBucket", bc.BIN_BUCKET), ("kBinBucketShift", bc.BIN_BUCKET_SHIFT),
                       ("kBinSub", bc.BIN_SUB), ("kBinMaxTiles", bc.BIN_MAX_TILES),
                       ("kBinBlocksMax", bc.BIN_BLOCKS_MAX), ("kBinMatrix", bc.BIN_MATRIX)]:
        env[name] = _constant(h, name, env)
        print(name, env[name])
        assert env[name] == mine, (name, env[name], mine)
    m = re.search(r"constexpr\s+int\s+kBinMaxTiles\s*=\s*\((\d+)\s*-\s*16\s*\*\s*kBinSub\)\s*/\s*4;", h)
    assert m and int(m.group(1)) == bc.LDS_CU
    assert "T > kBinMaxTiles ? 0 : std::max(1, std::min(kBinBlocksMax, kBinMatrix / std::max(T, 1)))" in h
    p = _text("preprocess.hip")
    assert "return sizeof(uint32_t) * ((size_t)T + 4 * kBinSub);" in p
    assert f"if (bytes <= {bc.LDS_DEFAULT}) return hipSuccess;" in p
    assert re.search(r"if \(a\.T <= 8 \* 1024\)\s+hipLaunchKernelGGL\(tile_ranges_kernel<8>", p)
    assert re.search(r"else if \(a\.T <= 40 \* 1024\)\s+hipLaunchKernelGGL\(tile_ranges_kernel<40>", p)
    assert "bin_atomic_kernel<false>, dim3((a.P + 255) / 256), dim3(256)" in p and bc.ATOMIC_SUB == 256
    r = _text("rasterizer.hip")
    assert "const bool lds = bin_blocks_max(p.T) > 0 && !c.opt.test_bin_atomic;" in r
    assert "if (c.opt.test_bin_blocks > 0) nb = std::min(nb, c.opt.test_bin_blocks);" in r
    assert "b.nblk = lds ? std::min(nb, (p.P + kBinSub - 1) / kBinSub) : 0;" in r
    assert "binning.stage = (!c.opt.test_bin_one_pass && p.P < (1 << kBinBucketShift))" in r


def test_mirror_bands():
    """The band boundaries the GPU cases are named for, from the mirror."""
    assert bc.BIN_MAX_TILES == 36864
    assert bc.bin_lds_bytes(12288) == 65536 and not bc.raises_lds_limit(12288) and bc.raises_lds_limit(12289)
    assert bc.bin_lds_bytes(bc.BIN_MAX_TILES) == bc.LDS_CU
    assert bc.plan(36864, 60_000).lds and not bc.plan(36865, 60_000).lds
    assert [bc.plan(t, 60_000, test_bin_atomic=1).ranges_kernel for t in (8192, 8193, 40960, 40961)] == [8, 40, 40, 0]
    assert bc.plan(8192, 60_000).nblk == 59 and bc.plan(36864, 60_000).nblk == 56 == bc.bin_blocks_max(36864)
    assert bc.plan(510, 60_000, test_bin_blocks=17).nblk == 17 and bc.plan(510, 1).nblk == 1
    assert bc.plan(510, 60_000).two_pass and not bc.plan(510, 60_000, test_bin_one_pass=1).two_pass
    assert {t % 8 for t in bc.SMALL_T} == {0, 1, 7}  # the padded launch grid: full, one past, one short
    for T, w in bc.SMALL_T.items():
        assert (w + 15) // 16 == T


def test_binning_lds_budget():
    """Static + dynamic LDS of the LDS binning's kernels, the static part read from the built code objects:
    within one CU's 160 KiB at kBinMaxTiles tiles, and within the default 64 KiB at every tile count at which the
    host does not raise the kernel's dynamic-LDS limit (allow_lds looks at the dynamic bytes alone). A static
    array added to one of these kernels (an inlined device function's __shared__ array counts) fails here."""
    from tests.test_abi import _kernel_resources

    res = _kernel_resources()
    t64 = max(t for t in range(1, bc.BIN_MAX_TILES + 1) if not bc.raises_lds_limit(t))
    assert t64 == 12288
    bad = []
    for name in BIN_KERNELS:
        full = f"{name}"
        match = [k for k in res if k == full or k.endswith(" " + full) or full in k]
        assert len(match) == 1, (name, sorted(k for k in res if "bin_" in k))
        static = res[match[0]][".group_segment_fixed_size"]
        top, mid = static + bc.bin_lds_bytes(bc.BIN_MAX_TILES), static + bc.bin_lds_bytes(t64)
        print(f"{name}: static LDS {static} B; {top} B at {bc.BIN_MAX_TILES} tiles (limit {bc.LDS_CU}); "
              f"{mid} B at {t64} tiles, the last without the attribute (limit {bc.LDS_DEFAULT})")
        if top > bc.LDS_CU or mid > bc.LDS_DEFAULT:
            bad.append((name, static, top, mid))
    assert not bad, bad


def test_case_names_unique_and_complete():
    assert len(set(bc.NAMES)) == len(bc.NAMES)
    for name in bc.NAMES:
        assert set(bc.case(name).variants) <= set(bc.VARIANTS)


@pytest.mark.parametrize("name", bc.NAMES)
def test_case_covers_its_branch(name):
    bc.covers(name)
