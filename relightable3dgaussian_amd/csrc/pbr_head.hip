// pbr_head.hip -- the PBR image head and the light regulariser of a training iteration (gfx950). Semantics are
// stated in include/r3dg_hip.h `r3dg_pbr_head_forward` and `r3dg_light_loss_forward`.
//
// The head restates the torch code between the rasterizer's feature output and the image loss
// (gaussian_renderer/neilf.py:169-175 and scene/gamma_trans.py:45-51; the captures' composite of
// relighting.py:225-229 and the evaluation grid's clamp / ACES hdr2ldr of utils/graphics_utils.py:197-201):
//   x = pbr + (1 - opacity) * bg, then y = x | clamp(x, 1e-9, 1) ** gamma | ACES(x) | clamp(x, 0, 1).
// There that is about a dozen element-wise launches forward and backward and a full-image reduction for the
// gamma gradient; here it is one launch forward and one (two with gamma) backward.
//
//   * head_fwd_kernel / head_bwd_kernel: one lane per FOUR consecutive pixels. In the pixel-major layout four
//     pixels are three float4 of pbr and one of opacity; in the planar layout one float4 per plane. A run is
//     taken with 16-byte accesses when its address allows (the rasterizer's pbr block starts at float 2 H W of
//     the feature buffer: 8 bytes off for odd H W) and as dwords otherwise or in the tail lane (act_device.h
//     load_run / store_run, as activation.hip takes its groups). The test is uniform over the launch.
//   * The backward saves nothing and recomputes x. With gamma every element needs y = xc ** gamma, the slope
//     gamma xc ** (gamma - 1) and the term G y ln(xc) of dL/dgamma. powf is evaluated once: the slope is
//     gamma * (y / xc), an exactly rounded division instead of a second powf, and ln(xc) is one logf. y cannot
//     be formed from that float logarithm: exp(gamma ln xc) multiplies the logarithm's rounding by |gamma ln xc|,
//     up to 45 at xc = 1e-9 and gamma = 2.2, where powf carries its logarithm in extended precision and stays
//     within an ulp, which is what the accuracy bars (4 float32 roundings of the largest value) need.
//   * dL/dgamma: each lane adds its twelve terms in double, a wave adds by butterfly, the four waves in order,
//     one double per workgroup; sum_partials_kernel (one workgroup) adds the partials in a fixed order. No float
//     atomics: two runs give the same bits.
//   * light_loss_{fwd,bwd}_kernel: one lane per four rows of diffuse_light [P,3] (three float4). The row mean,
//     the distances and the signs are evaluated in double from the float32 inputs: three float32 values add
//     exactly in double, so a row of equal channels has distance and gradient exactly 0, and a channel equal to
//     an exactly representable mean has sign 0, neither of which float32's fl(fl(3 a) / 3) guarantees. The value
//     is reduced like dL/dgamma and rounded once.
// No LDS beyond the four wave sums, no host synchronisation, nothing launched for an empty input.
// Built with -ffp-contract=off: the composite's three operations round one at a time, as torch's do, so the
// "none" and "clamp" forwards are the reference's bits.
#include "act_device.h"
#include "tone_device.h"  // clampf, aces (shared with display.hip)

namespace r3dg {
namespace {

constexpr int kThreads = 256;
constexpr float kGammaLo = 1e-9f;  // gamma_trans.py:47: a Python double, rounded when it meets the f32 tensor

// four pixels of a three-channel map as v[3 r + c]
template <bool HWC>
__device__ __forceinline__ void load3(const float* p, long long n, long long q0, int rows, float (&v)[kQuad * 3]) {
    if (HWC) {
        load_run(p + q0 * 3, rows * 3, v);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t[kQuad];
            load_run(p + c * n + q0, rows, t);
#pragma unroll
            for (int r = 0; r < kQuad; ++r) v[3 * r + c] = t[r];
        }
    }
}
template <bool HWC>
__device__ __forceinline__ void store3(float* p, long long n, long long q0, int rows, const float (&v)[kQuad * 3]) {
    if (HWC) {
        store_run(p + q0 * 3, rows * 3, v);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t[kQuad];
#pragma unroll
            for (int r = 0; r < kQuad; ++r) t[r] = v[3 * r + c];
            store_run(p + c * n + q0, rows, t);
        }
    }
}

template <bool HWC, bool BGIMG>
__device__ __forceinline__ void load_bg(const float* bg, long long n, long long q0, int rows, float (&b)[kQuad * 3]) {
    if (BGIMG) {
        load3<HWC>(bg, n, q0, rows, b);
    } else {
        const float b0 = bg[0], b1 = bg[1], b2 = bg[2];
#pragma unroll
        for (int r = 0; r < kQuad; ++r) b[3 * r] = b0, b[3 * r + 1] = b1, b[3 * r + 2] = b2;
    }
}

template <bool HWC, bool BGIMG>
__global__ void __launch_bounds__(kThreads) head_fwd_kernel(long long n, int tone, const float* __restrict__ pbr,
                                                           const float* __restrict__ opacity,
                                                           const float* __restrict__ bg,
                                                           const float* __restrict__ gamma, float* __restrict__ out) {
    const long long q0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kQuad;
    if (q0 >= n) return;
    const int rows = n - q0 < kQuad ? (int)(n - q0) : kQuad;
    float x[kQuad * 3], b[kQuad * 3], o[kQuad];
    load3<HWC>(pbr, n, q0, rows, x);
    load_run(opacity + q0, rows, o);
    load_bg<HWC, BGIMG>(bg, n, q0, rows, b);
#pragma unroll
    for (int i = 0; i < kQuad * 3; ++i) x[i] = x[i] + (1.0f - o[i / 3]) * b[i];
    if (tone == R3DG_PBR_TONE_GAMMA) {
        const float g = gamma[0];
#pragma unroll
        for (int i = 0; i < kQuad * 3; ++i) x[i] = powf(clampf(x[i], kGammaLo, 1.0f), g);
    } else if (tone == R3DG_PBR_TONE_ACES) {
#pragma unroll
        for (int i = 0; i < kQuad * 3; ++i) x[i] = aces(x[i]);
    } else if (tone == R3DG_PBR_TONE_CLAMP) {
#pragma unroll
        for (int i = 0; i < kQuad * 3; ++i) x[i] = clampf(x[i], 0.0f, 1.0f);
    }
    store3<HWC>(out, n, q0, rows, x);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the workgroup's sum of v to partial[blockIdx.x]: butterfly in the wave, the four waves in order
__device__ __forceinline__ void block_sum_to(double v, double* __restrict__ partial) {
    __shared__ double s_red[kThreads / 64];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_red[0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) s += s_red[w];
        partial[blockIdx.x] = s;
    }
}

// GAMMA: tone "gamma" (else "none"). d_pbr, d_opacity: NULL = not wanted; partial: GAMMA's per-workgroup sums of
// G y ln(xc), NULL = dL/dgamma not wanted
template <bool HWC, bool BGIMG, bool GAMMA>
__global__ void __launch_bounds__(kThreads) head_bwd_kernel(long long n, const float* __restrict__ pbr,
                                                           const float* __restrict__ opacity,
                                                           const float* __restrict__ bg,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ up, float* __restrict__ d_pbr,
                                                           float* __restrict__ d_opacity,
                                                           double* __restrict__ partial) {
    const long long q0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kQuad;
    double acc = 0.0;
    if (q0 < n) {
        const int rows = n - q0 < kQuad ? (int)(n - q0) : kQuad;
        float x[kQuad * 3], b[kQuad * 3], g[kQuad * 3], o[kQuad];
        load3<HWC>(up, n, q0, rows, g);
        if (GAMMA || d_opacity) load_bg<HWC, BGIMG>(bg, n, q0, rows, b);
        if (GAMMA) {
            load3<HWC>(pbr, n, q0, rows, x);
            load_run(opacity + q0, rows, o);
            const float gm = gamma[0];
#pragma unroll
            for (int i = 0; i < kQuad * 3; ++i) {
                const float xi = x[i] + (1.0f - o[i / 3]) * b[i];
                const bool open = xi >= kGammaLo && xi <= 1.0f;  // torch's clamp backward: bounds included
                const float xc = clampf(xi, kGammaLo, 1.0f);
                const float y = powf(xc, gm);
                if (partial && i / 3 < rows) acc += ((double)g[i] * (double)y) * (double)logf(xc);
                g[i] = open ? g[i] * (gm * (y / xc)) : 0.0f;
            }
        }
        if (d_pbr) store3<HWC>(d_pbr, n, q0, rows, g);
        if (d_opacity) {
#pragma unroll
            for (int r = 0; r < kQuad; ++r)
                o[r] = -((g[3 * r] * b[3 * r] + g[3 * r + 1] * b[3 * r + 1]) + g[3 * r + 2] * b[3 * r + 2]);
            store_run(d_opacity + q0, rows, o);
        }
    }
    if (GAMMA && partial) block_sum_to(acc, partial);
}

// out[0] = (float)(scale * the n partials added in a fixed order: thread k takes k, k + 256, ..., then a tree)
__global__ void __launch_bounds__(kThreads) sum_partials_kernel(int n, const double* __restrict__ partial,
                                                               double scale, float* __restrict__ out) {
    __shared__ double s_acc[kThreads];
    const int tid = threadIdx.x;
    double a = 0.0;
    for (int i = tid; i < n; i += kThreads) a += partial[i];
    s_acc[tid] = a;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) s_acc[tid] += s_acc[tid + s];
        __syncthreads();
    }
    if (tid == 0) out[0] = (float)(s_acc[0] * scale);
}

__global__ void __launch_bounds__(kThreads) light_loss_fwd_kernel(long long P, const float* __restrict__ d,
                                                                 double* __restrict__ partial) {
    const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kQuad;
    double acc = 0.0;
    if (p0 < P) {
        const int rows = P - p0 < kQuad ? (int)(P - p0) : kQuad;
        float v[kQuad * 3];
        load_run(d + p0 * 3, rows * 3, v);
#pragma unroll
        for (int r = 0; r < kQuad; ++r) {
            const double a = v[3 * r], b = v[3 * r + 1], c = v[3 * r + 2];
            const double m = ((a + b) + c) / 3.0;
            if (r < rows) acc += (fabs(a - m) + fabs(b - m)) + fabs(c - m);
        }
    }
    block_sum_to(acc, partial);
}

__device__ __forceinline__ double sgn(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0); }

__global__ void __launch_bounds__(kThreads) light_loss_bwd_kernel(long long P, double inv_n,
                                                                 const float* __restrict__ d,
                                                                 const float* __restrict__ up,
                                                                 float* __restrict__ grad) {
    const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kQuad;
    if (p0 >= P) return;
    const int rows = P - p0 < kQuad ? (int)(P - p0) : kQuad;
    const double k = (double)up[0] * inv_n;
    float v[kQuad * 3];
    load_run(d + p0 * 3, rows * 3, v);
#pragma unroll
    for (int r = 0; r < kQuad; ++r) {
        const double a = v[3 * r], b = v[3 * r + 1], c = v[3 * r + 2];
        const double m = ((a + b) + c) / 3.0;
        const double sa = sgn(a - m), sb = sgn(b - m), sc = sgn(c - m);
        const double mean = ((sa + sb) + sc) / 3.0;
        v[3 * r] = (float)((sa - mean) * k);
        v[3 * r + 1] = (float)((sb - mean) * k);
        v[3 * r + 2] = (float)((sc - mean) * k);
    }
    store_run(grad + p0 * 3, rows * 3, v);
}

unsigned blocks_for(long long n) { return (unsigned)((n + (long long)kThreads * kQuad - 1) / ((long long)kThreads * kQuad)); }

int check_head(const char* who, int H, int W, int layout, int tone, bool backward) {
    const std::string w(who);
    R3DG_REQUIRE(layout == R3DG_PBR_LAYOUT_CHW || layout == R3DG_PBR_LAYOUT_HWC, w + ": unknown layout");
    R3DG_REQUIRE(tone == R3DG_PBR_TONE_NONE || tone == R3DG_PBR_TONE_GAMMA ||
                     (!backward && (tone == R3DG_PBR_TONE_ACES || tone == R3DG_PBR_TONE_CLAMP)),
                 w + (backward ? ": tone must be none or gamma (aces and clamp are forward only)" : ": unknown tone"));
    R3DG_REQUIRE(H >= 1 && W >= 1, w + ": H, W >= 1 expected");
    R3DG_REQUIRE((long long)H * W <= 0x7fffffffll, w + ": H * W exceeds int32");
    return R3DG_OK;
}

}  // namespace
}  // namespace r3dg

using namespace r3dg;

extern "C" int r3dg_pbr_head_forward(int H, int W, int layout, int tone, const float* pbr, const float* opacity,
                                     const float* bg, int bg_per_pixel, const float* gamma, float* image,
                                     r3dg_stream_t stream) {
    if (int rc = check_head("pbr_head_forward", H, W, layout, tone, false)) return rc;
    R3DG_REQUIRE(pbr && opacity && bg && image, "pbr_head_forward: null pbr / opacity / bg / image");
    R3DG_REQUIRE(tone != R3DG_PBR_TONE_GAMMA || gamma, "pbr_head_forward: tone gamma needs gamma");
    const long long n = (long long)H * W;
    const dim3 grid(blocks_for(n)), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    const bool hwc = layout == R3DG_PBR_LAYOUT_HWC;
#define R3DG_HEAD_FWD(L, B) \
    hipLaunchKernelGGL((head_fwd_kernel<L, B>), grid, block, 0, st, n, tone, pbr, opacity, bg, gamma, image)
    if (hwc && bg_per_pixel) R3DG_HEAD_FWD(true, true);
    else if (hwc) R3DG_HEAD_FWD(true, false);
    else if (bg_per_pixel) R3DG_HEAD_FWD(false, true);
    else R3DG_HEAD_FWD(false, false);
#undef R3DG_HEAD_FWD
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}

extern "C" int r3dg_pbr_head_backward(int H, int W, int layout, int tone, const float* pbr, const float* opacity,
                                      const float* bg, int bg_per_pixel, const float* gamma, const float* dL_dimage,
                                      float* dL_dpbr, float* dL_dopacity, float* dL_dgamma,
                                      r3dg_alloc_fn scratch_alloc, void* scratch_ctx, r3dg_stream_t stream) {
    if (int rc = check_head("pbr_head_backward", H, W, layout, tone, true)) return rc;
    const bool gam = tone == R3DG_PBR_TONE_GAMMA;
    R3DG_REQUIRE(bg && dL_dimage, "pbr_head_backward: null bg / dL_dimage");
    R3DG_REQUIRE(!gam || (pbr && opacity && gamma), "pbr_head_backward: tone gamma needs pbr, opacity and gamma");
    R3DG_REQUIRE(gam || !dL_dgamma, "pbr_head_backward: dL_dgamma without tone gamma");
    R3DG_REQUIRE(!dL_dgamma || scratch_alloc, "pbr_head_backward: null scratch_alloc");
    if (!dL_dpbr && !dL_dopacity && !dL_dgamma) return R3DG_OK;
    const long long n = (long long)H * W;
    const dim3 grid(blocks_for(n)), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    double* partial = nullptr;
    if (dL_dgamma) {
        partial = (double*)scratch_alloc(scratch_ctx, sizeof(double) * grid.x);
        if (!partial) {
            set_error("pbr_head_backward: scratch allocation failed");
            return R3DG_ERR_ALLOC;
        }
    }
    const bool hwc = layout == R3DG_PBR_LAYOUT_HWC;
#define R3DG_HEAD_BWD(L, B, G)                                                                                   \
    hipLaunchKernelGGL((head_bwd_kernel<L, B, G>), grid, block, 0, st, n, pbr, opacity, bg, gamma, dL_dimage, \
                       dL_dpbr, dL_dopacity, partial)
#define R3DG_HEAD_BWD_LB(G)                                   \
    do {                                                      \
        if (hwc && bg_per_pixel) R3DG_HEAD_BWD(true, true, G); \
        else if (hwc) R3DG_HEAD_BWD(true, false, G);          \
        else if (bg_per_pixel) R3DG_HEAD_BWD(false, true, G); \
        else R3DG_HEAD_BWD(false, false, G);                  \
    } while (0)
    if (gam) R3DG_HEAD_BWD_LB(true);
    else R3DG_HEAD_BWD_LB(false);
#undef R3DG_HEAD_BWD_LB
#undef R3DG_HEAD_BWD
    R3DG_CHECK_HIP(hipGetLastError());
    if (dL_dgamma) {
        hipLaunchKernelGGL(sum_partials_kernel, dim3(1), block, 0, st, (int)grid.x, partial, 1.0, dL_dgamma);
        R3DG_CHECK_HIP(hipGetLastError());
    }
    return R3DG_OK;
}

extern "C" int r3dg_light_loss_forward(int P, const float* diffuse_light, float* loss, r3dg_alloc_fn scratch_alloc,
                                       void* scratch_ctx, r3dg_stream_t stream) {
    R3DG_REQUIRE(P >= 0, "light_loss_forward: negative P");
    if (P == 0) return R3DG_OK;
    R3DG_REQUIRE(diffuse_light && loss, "light_loss_forward: null diffuse_light / loss");
    R3DG_REQUIRE(scratch_alloc, "light_loss_forward: null scratch_alloc");
    const dim3 grid(blocks_for(P)), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)scratch_alloc(scratch_ctx, sizeof(double) * grid.x);
    if (!partial) {
        set_error("light_loss_forward: scratch allocation failed");
        return R3DG_ERR_ALLOC;
    }
    hipLaunchKernelGGL(light_loss_fwd_kernel, grid, block, 0, st, (long long)P, diffuse_light, partial);
    R3DG_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), block, 0, st, (int)grid.x, partial, 1.0 / (3.0 * (double)P), loss);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}

extern "C" int r3dg_light_loss_backward(int P, const float* diffuse_light, const float* upstream, float* grad,
                                        r3dg_stream_t stream) {
    R3DG_REQUIRE(P >= 0, "light_loss_backward: negative P");
    if (P == 0) return R3DG_OK;
    R3DG_REQUIRE(diffuse_light && upstream && grad, "light_loss_backward: null diffuse_light / upstream / grad");
    hipLaunchKernelGGL(light_loss_bwd_kernel, dim3(blocks_for(P)), dim3(kThreads), 0, (hipStream_t)stream,
                       (long long)P, 1.0 / (3.0 * (double)P), diffuse_light, upstream, grad);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}
