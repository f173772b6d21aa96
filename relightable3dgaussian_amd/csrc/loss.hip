// loss.hip -- the fused L1 + SSIM image loss of a training iteration (the reference's calculate_loss,
// gaussian_renderer/neilf.py:216-222: F.l1_loss, utils/loss_utils.py:31-62 ssim, utils/image_utils.py:24-29
// psnr), forward and backward.
//
// An image is `planes` = B*C independent [H, W] planes, addressed through three element strides (plane,
// row, pixel), so CHW and the rasterizer's HWC are the same code. Per plane:
//   mu1 = g*x, mu2 = g*y, s1 = g*x^2 - mu1^2, s2 = g*y^2 - mu2^2, s12 = g*xy - mu1 mu2
//   map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2))
// with g the zero-padded 11x11 Gaussian window (sigma 1.5) = kWin kWin^T, all in f32 as the reference.
//
// Forward: one workgroup per 16x16 tile. The 26x26 patches of x and y go to LDS, a horizontal pass writes
// the five row-filtered statistics (26 rows x 16 columns) to LDS, the vertical pass leaves the five window
// means in registers. Each pixel gives map, |x-y| and (x-y)^2; the workgroup adds them (butterfly inside
// each wave, the four waves in order) and writes one partial triple. A second kernel, one workgroup per
// plane, adds the partials in a fixed order in f64. No float atomics: the sums are bitwise reproducible.
// When a gradient is wanted the forward also stores, per pixel, the derivatives of map by mu1, by g*x^2
// and by g*xy (s1, s2, s12 substituted, so the first is the total derivative by mu1).
//
// Backward: per tile the same separable filter over those three planes (the window is symmetric, so the
// adjoint of the zero-padded convolution is the convolution), then
//   dL/dx = scale * (w_ssim * (g*d_mu1 + 2 x g*d_xx + y g*d_xy) + w_abs * sign(x - y)),  sign(0) = 0,
// with the per-plane weights read from device memory. The weights multiply after the filter (it is
// linear) and `scale` multiplies last, so scaling the loss by k scales the gradient to fl(k * gradient).
//
// LDS: addresses follow the flat thread index in every pass (patch fill, row-filtered stores, vertical
// reads at tid + 16 k), so ds_read/write_b32 see distinct banks; only the horizontal reads, where a wave
// spans four patch rows of stride 26, overlap by four banks.
#include <cstdint>

#include "r3dg_common.h"

namespace r3dg {
namespace {

constexpr int kTile = 16;                    // output tile edge; 256 threads, one per pixel
constexpr int kHalo = 5;                     // window_size // 2
constexpr int kTaps = 2 * kHalo + 1;         // 11
constexpr int kPatch = kTile + 2 * kHalo;    // 26
constexpr int kPatchN = kPatch * kPatch;     // 676 input pixels per tile
constexpr int kRowsN = kPatch * kTile;       // 416 row-filtered values per statistic
constexpr int kThreads = kTile * kTile;

// loss_utils.py:19-21 gaussian(11, 1.5): exp(-(k-5)^2 / 4.5) as f32, divided by their f32 sum
#define R3DG_LOSS_WINDOW                                                                                   \
    {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,      \
     0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}
__constant__ float kWin[kTaps] = R3DG_LOSS_WINDOW;
const float kWinHost[kTaps] = R3DG_LOSS_WINDOW;

constexpr float kC1 = (float)(0.01 * 0.01);  // loss_utils.py:54-55: Python doubles, rounded when they meet the f32 tensor
constexpr float kC2 = (float)(0.03 * 0.03);

struct Strides {
    int64_t plane, row, px;
};

// One pixel's ssim_map value from the five window means, and its derivatives by mu1 (total: s1 and s12
// depend on it), by g*x^2 and by g*xy. Every operation is rounded on its own, as the reference's
// tensor operations are (this file is compiled with -ffp-contract=off, build.py; the filter loops ask
// for their FMAs by name), and the derivatives are arranged so that identical
// images give map == 1 and derivatives that cancel to an exactly zero gradient: then a1 == b1 and
// a2 == b2 bit for bit, d_mu is 0, and d_xy is exactly -2 d_xx.
struct SsimPixel {
    float map, d_mu, d_xx, d_xy;
};
__device__ __forceinline__ SsimPixel ssim_pixel(float mu1, float mu2, float e11, float e22, float e12) {
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const float a1 = 2.0f * mu12 + kC1, a2 = 2.0f * (e12 - mu12) + kC2;
    const float b1 = mu1_sq + mu2_sq + kC1, b2 = (e11 - mu1_sq) + (e22 - mu2_sq) + kC2;
    SsimPixel p;
    p.map = (a1 * a2) / (b1 * b2);
    p.d_mu = 2.0f * (mu2 * (a2 - a1) + mu1 * p.map * (b1 - b2)) / (b1 * b2);
    p.d_xx = -(p.map / b2);
    p.d_xy = 2.0f * ((a1 / b1) / b2);
    return p;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// blockIdx.x -> (plane, tile origin)
__device__ __forceinline__ void tile_of(int tiles_x, int tiles, int& plane, int& x0, int& y0) {
    plane = (int)(blockIdx.x / (unsigned)tiles);
    const int t = (int)(blockIdx.x % (unsigned)tiles);
    x0 = (t % tiles_x) * kTile;
    y0 = (t / tiles_x) * kTile;
}

template <bool GRAD>
__global__ void __launch_bounds__(kThreads) image_loss_forward_kernel(int H, int W, int tiles_x, int tiles,
                                                                     const float* __restrict__ img, Strides si,
                                                                     const float* __restrict__ gt, Strides sg,
                                                                     float* __restrict__ partial,
                                                                     float* __restrict__ dmaps, int64_t dmap_stride) {
    __shared__ float s_x[kPatchN], s_y[kPatchN];
    __shared__ float s_h[5][kRowsN];
    __shared__ float s_red[kThreads / 64][3];
    int plane, x0, y0;
    tile_of(tiles_x, tiles, plane, x0, y0);
    const int tid = threadIdx.x;
    const float* ip = img + (int64_t)plane * si.plane;
    const float* gp = gt + (int64_t)plane * sg.plane;

    for (int i = tid; i < kPatchN; i += kThreads) {
        const int y = y0 - kHalo + i / kPatch, x = x0 - kHalo + i % kPatch;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;  // zero padding
        s_x[i] = in ? ip[(int64_t)y * si.row + (int64_t)x * si.px] : 0.0f;
        s_y[i] = in ? gp[(int64_t)y * sg.row + (int64_t)x * sg.px] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < kRowsN; i += kThreads) {
        const int base = (i / kTile) * kPatch + i % kTile;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const float w = kWin[k], x = s_x[base + k], y = s_y[base + k];
            a = fmaf(w, x, a);
            b = fmaf(w, y, b);
            aa = fmaf(w, x * x, aa);
            bb = fmaf(w, y * y, bb);
            ab = fmaf(w, x * y, ab);
        }
        s_h[0][i] = a;
        s_h[1][i] = b;
        s_h[2][i] = aa;
        s_h[3][i] = bb;
        s_h[4][i] = ab;
    }
    __syncthreads();
    float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
        const float w = kWin[k];
        const int j = tid + k * kTile;
        mu1 = fmaf(w, s_h[0][j], mu1);
        mu2 = fmaf(w, s_h[1][j], mu2);
        e11 = fmaf(w, s_h[2][j], e11);
        e22 = fmaf(w, s_h[3][j], e22);
        e12 = fmaf(w, s_h[4][j], e12);
    }
    const int lx = tid % kTile, ly = tid / kTile, x = x0 + lx, y = y0 + ly;
    const bool valid = x < W && y < H;
    float v_map = 0.f, v_abs = 0.f, v_sq = 0.f;
    if (valid) {
        const SsimPixel p = ssim_pixel(mu1, mu2, e11, e22, e12);
        v_map = p.map;
        const int c = (ly + kHalo) * kPatch + lx + kHalo;
        const float d = s_x[c] - s_y[c];
        v_abs = fabsf(d);
        v_sq = d * d;
        if (GRAD) {
            float* o = dmaps + ((int64_t)plane * H + y) * W + x;
            o[0] = p.d_mu;
            o[dmap_stride] = p.d_xx;
            o[2 * dmap_stride] = p.d_xy;
        }
    }
    v_map = wave_sum(v_map);
    v_abs = wave_sum(v_abs);
    v_sq = wave_sum(v_sq);
    if ((tid & 63) == 0) {
        s_red[tid >> 6][0] = v_map;
        s_red[tid >> 6][1] = v_abs;
        s_red[tid >> 6][2] = v_sq;
    }
    __syncthreads();
    if (tid < 3) {
        float s = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) s += s_red[w][tid];
        partial[(int64_t)blockIdx.x * 3 + tid] = s;
    }
}

// sums[plane][k] = the plane's partials added in a fixed order: thread t takes partials t, t + 256, ...
// in f64, then a tree over the 256 threads.
__global__ void __launch_bounds__(kThreads) image_loss_finish_kernel(int tiles, const float* __restrict__ partial,
                                                                    float* __restrict__ sums) {
    __shared__ double s_acc[3][kThreads];
    const int plane = blockIdx.x, tid = threadIdx.x;
    const float* p = partial + (int64_t)plane * tiles * 3;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int t = tid; t < tiles; t += kThreads) {
        a0 += (double)p[3 * (int64_t)t];
        a1 += (double)p[3 * (int64_t)t + 1];
        a2 += (double)p[3 * (int64_t)t + 2];
    }
    s_acc[0][tid] = a0;
    s_acc[1][tid] = a1;
    s_acc[2][tid] = a2;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            s_acc[0][tid] += s_acc[0][tid + s];
            s_acc[1][tid] += s_acc[1][tid + s];
            s_acc[2][tid] += s_acc[2][tid + s];
        }
        __syncthreads();
    }
    if (tid < 3) sums[(int64_t)plane * 3 + tid] = (float)s_acc[tid][0];
}

__global__ void __launch_bounds__(kThreads) image_loss_backward_kernel(
    int H, int W, int tiles_x, int tiles, const float* __restrict__ img, Strides si, const float* __restrict__ gt,
    Strides sg, const float* __restrict__ dmaps, int64_t dmap_stride, const float* __restrict__ w_ssim,
    const float* __restrict__ w_abs, const float* __restrict__ scale, float* __restrict__ dL_dimg) {
    __shared__ float s_d[3][kPatchN];
    __shared__ float s_h[3][kRowsN];
    int plane, x0, y0;
    tile_of(tiles_x, tiles, plane, x0, y0);
    const int tid = threadIdx.x;
    const float* dp = dmaps + (int64_t)plane * H * W;

    for (int i = tid; i < kPatchN; i += kThreads) {
        const int y = y0 - kHalo + i / kPatch, x = x0 - kHalo + i % kPatch;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const int64_t o = (int64_t)y * W + x;
        s_d[0][i] = in ? dp[o] : 0.0f;
        s_d[1][i] = in ? dp[o + dmap_stride] : 0.0f;
        s_d[2][i] = in ? dp[o + 2 * dmap_stride] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < kRowsN; i += kThreads) {
        const int base = (i / kTile) * kPatch + i % kTile;
        float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const float w = kWin[k];
            a = fmaf(w, s_d[0][base + k], a);
            b = fmaf(w, s_d[1][base + k], b);
            c = fmaf(w, s_d[2][base + k], c);
        }
        s_h[0][i] = a;
        s_h[1][i] = b;
        s_h[2][i] = c;
    }
    __syncthreads();
    const int x = x0 + tid % kTile, y = y0 + tid / kTile;
    if (x >= W || y >= H) return;
    float c_mu = 0.f, c_xx = 0.f, c_xy = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
        const float w = kWin[k];
        const int j = tid + k * kTile;
        c_mu = fmaf(w, s_h[0][j], c_mu);
        c_xx = fmaf(w, s_h[1][j], c_xx);
        c_xy = fmaf(w, s_h[2][j], c_xy);
    }
    const int64_t oi = (int64_t)plane * si.plane + (int64_t)y * si.row + (int64_t)x * si.px;
    const float xv = img[oi];
    const float yv = gt[(int64_t)plane * sg.plane + (int64_t)y * sg.row + (int64_t)x * sg.px];
    const float d = xv - yv;
    const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    // identical images: (2 x) c_xx + y c_xy cancels exactly (ssim_pixel)
    float g = w_ssim[plane] * ((c_mu + (2.0f * xv) * c_xx) + yv * c_xy) + w_abs[plane] * sgn;
    if (scale) g *= scale[plane];
    dL_dimg[oi] = g;
}

struct Geometry {
    int tiles_x, tiles;
    long long blocks;
};

// the checks both entry points share; geometry only when there is work
int check_image(const char* who, int planes, int H, int W, const void* img, const void* gt, Geometry& geo) {
    const std::string w(who);
    R3DG_REQUIRE(planes >= 0 && H >= 0 && W >= 0, w + ": negative planes / H / W");
    geo = Geometry{0, 0, 0};
    if (planes == 0 || H == 0 || W == 0) return R3DG_OK;
    R3DG_REQUIRE((long long)planes * H * W <= 0x7fffffffll, w + ": planes * H * W exceeds int32");
    R3DG_REQUIRE(img && gt, w + ": null img / gt");
    geo.tiles_x = (W + kTile - 1) / kTile;
    geo.tiles = geo.tiles_x * ((H + kTile - 1) / kTile);
    geo.blocks = (long long)planes * geo.tiles;  // <= planes * H * W
    return R3DG_OK;
}

}  // namespace
}  // namespace r3dg

using namespace r3dg;

extern "C" const float* r3dg_image_loss_window(void) { return kWinHost; }

extern "C" int r3dg_image_loss_forward(int planes, int H, int W, const float* img, int64_t img_plane_stride,
                                       int64_t img_row_stride, int64_t img_px_stride, const float* gt,
                                       int64_t gt_plane_stride, int64_t gt_row_stride, int64_t gt_px_stride,
                                       float* sums, float* dmaps, r3dg_alloc_fn scratch_alloc, void* scratch_ctx,
                                       r3dg_stream_t stream) {
    Geometry geo;
    if (int rc = check_image("image_loss_forward", planes, H, W, img, gt, geo)) return rc;
    if (geo.blocks == 0) return R3DG_OK;
    R3DG_REQUIRE(sums, "image_loss_forward: null sums");
    R3DG_REQUIRE(scratch_alloc, "image_loss_forward: null scratch_alloc");
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)scratch_alloc(scratch_ctx, sizeof(float) * 3 * (size_t)geo.blocks);
    if (!partial) {
        set_error("image_loss_forward: scratch allocation failed");
        return R3DG_ERR_ALLOC;
    }
    const Strides si{img_plane_stride, img_row_stride, img_px_stride}, sg{gt_plane_stride, gt_row_stride, gt_px_stride};
    const int64_t dmap_stride = (int64_t)planes * H * W;
    if (dmaps)
        hipLaunchKernelGGL(image_loss_forward_kernel<true>, dim3((unsigned)geo.blocks), dim3(kThreads), 0, st, H, W,
                           geo.tiles_x, geo.tiles, img, si, gt, sg, partial, dmaps, dmap_stride);
    else
        hipLaunchKernelGGL(image_loss_forward_kernel<false>, dim3((unsigned)geo.blocks), dim3(kThreads), 0, st, H, W,
                           geo.tiles_x, geo.tiles, img, si, gt, sg, partial, (float*)nullptr, dmap_stride);
    R3DG_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(image_loss_finish_kernel, dim3(planes), dim3(kThreads), 0, st, geo.tiles, partial, sums);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}

extern "C" int r3dg_image_loss_backward(int planes, int H, int W, const float* img, int64_t img_plane_stride,
                                        int64_t img_row_stride, int64_t img_px_stride, const float* gt,
                                        int64_t gt_plane_stride, int64_t gt_row_stride, int64_t gt_px_stride,
                                        const float* dmaps, const float* w_ssim, const float* w_abs,
                                        const float* scale, float* dL_dimg, r3dg_stream_t stream) {
    Geometry geo;
    if (int rc = check_image("image_loss_backward", planes, H, W, img, gt, geo)) return rc;
    if (geo.blocks == 0) return R3DG_OK;
    R3DG_REQUIRE(dmaps && w_ssim && w_abs && dL_dimg, "image_loss_backward: null dmaps / w_ssim / w_abs / dL_dimg");
    const Strides si{img_plane_stride, img_row_stride, img_px_stride}, sg{gt_plane_stride, gt_row_stride, gt_px_stride};
    hipLaunchKernelGGL(image_loss_backward_kernel, dim3((unsigned)geo.blocks), dim3(kThreads), 0, (hipStream_t)stream, H,
                       W, geo.tiles_x, geo.tiles, img, si, gt, sg, dmaps, (int64_t)planes * H * W, w_ssim, w_abs, scale,
                       dL_dimg);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}
