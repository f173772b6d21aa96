// display.hip -- the display and capture head (gfx950): from the rasterizer's buffers to the bytes that are copied
// to the host. Semantics are stated in include/r3dg_hip.h `r3dg_display_frame`.
//
// It restates the last element-wise torch code before a frame leaves the GPU: the GUI's get_buffer
// (gui.py:138-172), the relighting script's captures with torchvision's save_image (relighting.py:222-230) and the
// evaluation report's tiles (train.py:243-272). There a capture is about seven launches that each read and
// write a whole image, and a frame has ten captures; here all K <= 16 images of a frame are one launch.
//
//   * display_kernel: one lane per FOUR consecutive pixels, as pbr_head.hip. The spec table (source pointer,
//     channel count, layout, mode, tone) arrives by value in the kernel arguments and is walked by a uniform
//     loop, so every mode and tone branch is uniform. Opacity and the background are loaded once per lane for
//     all specs; a source named by several specs is loaded per spec. A run is taken with 16-byte accesses when
//     its address allows (a block view of the feature buffer starts 4, 8 or 12 bytes off for odd H W) and as
//     dwords otherwise or in the tail lane (act_device.h load_run / store_run); the test is uniform over the
//     launch. Four pixels of 8-bit output are 12 contiguous bytes: three dwords when image k starts on a dword
//     (3 k H W a multiple of 4), bytes otherwise or in the tail lane.
//   * MODE_RANGE needs the minimum and maximum of a whole source first: range_partial_kernel (grid.y = the range
//     specs) leaves (min, max, saw-a-NaN) per workgroup, range_finish_kernel (one workgroup) reduces them to
//     (mn, mx) per spec in scratch, NaN for both when a NaN was seen, as torch.min / torch.max. Two extra
//     launches however many range specs there are. Min and max do not depend on the order: no atomics, the
//     same bits in every run.
// No host synchronisation.
// Built with -ffp-contract=off: every mode is a short sequence of torch tensor operations in the reference,
// each rounded on its own (s * 0.5 + 0.5, (1 - o) * b, y * 255 + 0.5); uncontracted, every output but the ACES
// tone's is the reference's bits, and the ACES tone rounds where hdr2ldr does (tone_device.h, pbr_head.hip's).
#include "act_device.h"
#include "tone_device.h"

namespace r3dg {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxSpecs = R3DG_DISPLAY_MAX_SPECS;

struct SpecK {
    const float* src;  // int32 bits with MODE_COUNT
    int ch, chw, mode, tone;
};

struct DisplayArgs {
    long long n;
    int K, enc, bg_kind;
    const float* opacity;
    const float* bg;
    float bgv[3];
    const float* range;  // [kMaxSpecs][2]: (mn, mx) of a range spec
    void* out;
    SpecK spec[kMaxSpecs];
};

// save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8); NaN -> 0
__device__ __forceinline__ unsigned quantise(float y) {
    float t = y * 255.0f;
    t = t + 0.5f;
    t = clampf(t, 0.0f, 255.0f);
    return t != t ? 0u : (unsigned)t;
}

__global__ void __launch_bounds__(kThreads) display_kernel(DisplayArgs a) {
    const long long n = a.n;
    const long long q0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kQuad;
    if (q0 >= n) return;
    const int rows = n - q0 < kQuad ? (int)(n - q0) : kQuad;
    float o[kQuad] = {0.f, 0.f, 0.f, 0.f}, b[kQuad * 3];
    if (a.opacity) load_run(a.opacity + q0, rows, o);
    if (a.bg_kind == R3DG_DISPLAY_BG_IMAGE) {
        load_run(a.bg + q0 * 3, rows * 3, b);
    } else {
        float b0 = a.bgv[0], b1 = a.bgv[1], b2 = a.bgv[2];
        if (a.bg_kind == R3DG_DISPLAY_BG_VECTOR) b0 = a.bg[0], b1 = a.bg[1], b2 = a.bg[2];
#pragma unroll
        for (int r = 0; r < kQuad; ++r) b[3 * r] = b0, b[3 * r + 1] = b1, b[3 * r + 2] = b2;
    }
    for (int k = 0; k < a.K; ++k) {
        const float* src = a.spec[k].src;
        const int ch = a.spec[k].ch, chw = a.spec[k].chw, mode = a.spec[k].mode, tone = a.spec[k].tone;
        float y[kQuad * 3];
        if (ch == 1) {
            float t[kQuad];
            load_run(src + q0, rows, t);
            if (mode == R3DG_DISPLAY_MODE_COUNT) {
#pragma unroll
                for (int r = 0; r < kQuad; ++r) t[r] = (float)min(__float_as_int(t[r]), 1000) / 1000.0f;
            }
#pragma unroll
            for (int i = 0; i < kQuad * 3; ++i) y[i] = t[i / 3];
        } else if (!chw) {
            load_run(src + q0 * 3, rows * 3, y);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float t[kQuad];
                load_run(src + c * n + q0, rows, t);
#pragma unroll
                for (int r = 0; r < kQuad; ++r) y[3 * r + c] = t[r];
            }
        }
        if (mode == R3DG_DISPLAY_MODE_OVER) {
#pragma unroll
            for (int i = 0; i < kQuad * 3; ++i) y[i] = y[i] + (1.0f - o[i / 3]) * b[i];
        } else if (mode == R3DG_DISPLAY_MODE_NORMAL_OVER) {
#pragma unroll
            for (int i = 0; i < kQuad * 3; ++i) y[i] = (y[i] * 0.5f + 0.5f) + (1.0f - o[i / 3]) * b[i];
        } else if (mode == R3DG_DISPLAY_MODE_NORMAL_MASK) {
#pragma unroll
            for (int i = 0; i < kQuad * 3; ++i) y[i] = y[i] * 0.5f + 0.5f * o[i / 3];
        } else if (mode == R3DG_DISPLAY_MODE_RANGE) {
            const float mn = a.range[2 * k], mx = a.range[2 * k + 1];
            const float span = mx - mn;
#pragma unroll
            for (int i = 0; i < kQuad * 3; ++i) y[i] = (y[i] - mn) / span;
        }
        if (tone == R3DG_DISPLAY_TONE_CLAMP) {
#pragma unroll
            for (int i = 0; i < kQuad * 3; ++i) y[i] = clampf(y[i], 0.0f, 1.0f);
        } else if (tone == R3DG_DISPLAY_TONE_ACES) {
#pragma unroll
            for (int i = 0; i < kQuad * 3; ++i) y[i] = aces(y[i]);
        }
        const long long e0 = ((long long)k * n + q0) * 3;  // the lane's first output element
        if (a.enc == R3DG_DISPLAY_ENC_F32) {
            store_run((float*)a.out + e0, rows * 3, y);
        } else {
            unsigned char* p = (unsigned char*)a.out + e0;
            unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < kQuad * 3; ++i) w[i / 4] |= quantise(y[i]) << (8 * (i % 4));
            if (rows == kQuad && ((uintptr_t)p & 3) == 0) {
                struct alignas(4) U3 { unsigned x, y, z; };
                *reinterpret_cast<U3*>(p) = U3{w[0], w[1], w[2]};
            } else {
#pragma unroll
                for (int i = 0; i < kQuad * 3; ++i)
                    if (i < rows * 3) p[i] = (unsigned char)(w[i / 4] >> (8 * (i % 4)));
            }
        }
    }
}

struct RangeArgs {
    int R, blocks;             // range specs; workgroups per spec (grid.x)
    long long count[kMaxSpecs];  // elements of range spec r's source (dense: the layout does not matter)
    const float* src[kMaxSpecs];
    int slot[kMaxSpecs];       // the spec index k of range spec r
    float* partial;            // [R][blocks][3]: min, max, 1 when a NaN was seen
    float* range;              // [kMaxSpecs][2]
};

__device__ __forceinline__ void wave_minmax(float& mn, float& mx, float& nan) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, s));
        mx = fmaxf(mx, __shfl_xor(mx, s));
        nan = fmaxf(nan, __shfl_xor(nan, s));
    }
}

// the workgroup's (min, max, nan) in thread 0
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float& nan) {
    __shared__ float s_red[3][kThreads / 64];
    wave_minmax(mn, mx, nan);
    if ((threadIdx.x & 63) == 0) {
        s_red[0][threadIdx.x >> 6] = mn;
        s_red[1][threadIdx.x >> 6] = mx;
        s_red[2][threadIdx.x >> 6] = nan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) {
            mn = fminf(mn, s_red[0][w]);
            mx = fmaxf(mx, s_red[1][w]);
            nan = fmaxf(nan, s_red[2][w]);
        }
    }
}

__global__ void __launch_bounds__(kThreads) range_partial_kernel(RangeArgs a) {
    const int r = blockIdx.y;
    const long long cnt = a.count[r];
    const long long e0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kQuad;
    float mn = INFINITY, mx = -INFINITY, nan = 0.0f;
    if (e0 < cnt) {
        const int m = cnt - e0 < kQuad ? (int)(cnt - e0) : kQuad;
        float v[kQuad];
        load_run(a.src[r] + e0, m, v);
#pragma unroll
        for (int i = 0; i < kQuad; ++i) {
            if (i < m) {
                mn = fminf(mn, v[i]);  // a NaN is dropped here and counted below
                mx = fmaxf(mx, v[i]);
                nan = v[i] != v[i] ? 1.0f : nan;
            }
        }
    }
    block_minmax(mn, mx, nan);
    if (threadIdx.x == 0) {
        float* p = a.partial + ((size_t)r * a.blocks + blockIdx.x) * 3;
        p[0] = mn; p[1] = mx; p[2] = nan;
    }
}

__global__ void __launch_bounds__(kThreads) range_finish_kernel(RangeArgs a) {
    for (int r = 0; r < a.R; ++r) {
        float mn = INFINITY, mx = -INFINITY, nan = 0.0f;
        for (int i = threadIdx.x; i < a.blocks; i += kThreads) {
            const float* p = a.partial + ((size_t)r * a.blocks + i) * 3;
            mn = fminf(mn, p[0]);
            mx = fmaxf(mx, p[1]);
            nan = fmaxf(nan, p[2]);
        }
        block_minmax(mn, mx, nan);
        if (threadIdx.x == 0) {
            const float q = __int_as_float(0x7fc00000);
            a.range[2 * a.slot[r]] = nan != 0.0f ? q : mn;
            a.range[2 * a.slot[r] + 1] = nan != 0.0f ? q : mx;
        }
        __syncthreads();  // s_red is reused by the next spec
    }
}

unsigned blocks_for(long long n) { return (unsigned)((n + (long long)kThreads * kQuad - 1) / ((long long)kThreads * kQuad)); }

}  // namespace
}  // namespace r3dg

using namespace r3dg;

extern "C" int r3dg_display_frame(int H, int W, int n_specs, const r3dg_display_spec* specs, const float* opacity,
                                  const float* bg, int bg_kind, int encoding, void* out, r3dg_alloc_fn scratch_alloc,
                                  void* scratch_ctx, r3dg_stream_t stream) {
    R3DG_REQUIRE(H >= 1 && W >= 1, "display_frame: H, W >= 1 expected");
    R3DG_REQUIRE((long long)H * W <= 0x7fffffffll, "display_frame: H * W exceeds int32");
    R3DG_REQUIRE(n_specs >= 1 && n_specs <= kMaxSpecs, "display_frame: 1 to 16 specs expected");
    R3DG_REQUIRE(specs && out, "display_frame: null specs / out");
    R3DG_REQUIRE(encoding == R3DG_DISPLAY_ENC_F32 || encoding == R3DG_DISPLAY_ENC_U8, "display_frame: unknown encoding");
    R3DG_REQUIRE(bg_kind >= R3DG_DISPLAY_BG_NONE && bg_kind <= R3DG_DISPLAY_BG_HOST, "display_frame: unknown bg_kind");
    R3DG_REQUIRE((bg_kind == R3DG_DISPLAY_BG_NONE) == (bg == nullptr),
                 "display_frame: bg is given with a bg_kind other than BG_NONE and with no other");
    const long long n = (long long)H * W;
    DisplayArgs a{};
    RangeArgs ra{};
    for (int k = 0; k < n_specs; ++k) {
        const r3dg_display_spec& s = specs[k];
        const std::string w = "display_frame: spec " + std::to_string(k);
        R3DG_REQUIRE(s.source, w + ": null source");
        R3DG_REQUIRE(s.channels == 1 || s.channels == 3, w + ": channels 1 or 3 expected");
        R3DG_REQUIRE(s.layout == R3DG_PBR_LAYOUT_CHW || s.layout == R3DG_PBR_LAYOUT_HWC, w + ": unknown layout");
        R3DG_REQUIRE(s.mode >= R3DG_DISPLAY_MODE_PLAIN && s.mode <= R3DG_DISPLAY_MODE_COUNT, w + ": unknown mode");
        R3DG_REQUIRE(s.tone >= R3DG_DISPLAY_TONE_NONE && s.tone <= R3DG_DISPLAY_TONE_ACES, w + ": unknown tone");
        R3DG_REQUIRE(s.mode != R3DG_DISPLAY_MODE_COUNT || s.channels == 1, w + ": mode count takes a one-channel int32 source");
        const bool over = s.mode == R3DG_DISPLAY_MODE_OVER || s.mode == R3DG_DISPLAY_MODE_NORMAL_OVER;
        R3DG_REQUIRE(!(over || s.mode == R3DG_DISPLAY_MODE_NORMAL_MASK) || opacity, w + ": the mode needs opacity");
        R3DG_REQUIRE(!over || bg, w + ": the mode needs bg");
        R3DG_REQUIRE(s.mode != R3DG_DISPLAY_MODE_RANGE || scratch_alloc, w + ": mode range with a null scratch_alloc");
        a.spec[k] = SpecK{(const float*)s.source, s.channels, s.layout == R3DG_PBR_LAYOUT_CHW, s.mode, s.tone};
        if (s.mode == R3DG_DISPLAY_MODE_RANGE) {
            ra.count[ra.R] = n * s.channels;
            ra.src[ra.R] = (const float*)s.source;
            ra.slot[ra.R] = k;
            ++ra.R;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    if (ra.R) {
        long long most = 0;
        for (int r = 0; r < ra.R; ++r) most = ra.count[r] > most ? ra.count[r] : most;
        ra.blocks = (int)blocks_for(most);
        const size_t floats = (size_t)ra.R * ra.blocks * 3 + 2 * kMaxSpecs;
        float* scratch = (float*)scratch_alloc(scratch_ctx, sizeof(float) * floats);
        if (!scratch) {
            set_error("display_frame: scratch allocation failed");
            return R3DG_ERR_ALLOC;
        }
        ra.range = scratch;
        ra.partial = scratch + 2 * kMaxSpecs;
        hipLaunchKernelGGL(range_partial_kernel, dim3(ra.blocks, ra.R), dim3(kThreads), 0, st, ra);
        R3DG_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(range_finish_kernel, dim3(1), dim3(kThreads), 0, st, ra);
        R3DG_CHECK_HIP(hipGetLastError());
    }
    a.n = n;
    a.K = n_specs;
    a.enc = encoding;
    a.bg_kind = bg_kind;
    a.opacity = opacity;
    a.bg = bg_kind == R3DG_DISPLAY_BG_HOST ? nullptr : bg;
    if (bg_kind == R3DG_DISPLAY_BG_HOST) a.bgv[0] = bg[0], a.bgv[1] = bg[1], a.bgv[2] = bg[2];
    a.range = ra.range;
    a.out = out;
    hipLaunchKernelGGL(display_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, a);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}
