// reg_loss.hip -- the eight image-space regularisers of a training iteration (the reference's calculate_loss,
// gaussian_renderer/neilf.py:233-321, and utils/loss_utils.py:65-96 bilateral_smooth_loss), forward and
// backward: depth L1, mask entropy, the two normal MSE terms, the base-colour guide and the three bilateral
// smoothness terms. Semantics per pixel are stated in include/r3dg_hip.h `r3dg_reg_loss_forward`.
//
// Every map is n planes addressed through three element strides (plane, row, pixel), so CHW tensors and the
// rasterizer's [H*W, n] feature blocks are the same code and give the same bits. Which terms run is a bit set
// read at run time: a disabled term loads nothing, and the arithmetic of an enabled one does not depend on
// the others, so a subset reproduces the full run's bits.
//
// Forward: one workgroup per 16x16 tile. The pointwise terms read global memory. For the smoothness terms the
// channel means of gt_image and of the enabled data maps go to 18x18 LDS patches (halo 1, zero outside the
// image); |Sobel_x| + |Sobel_y| is taken from LDS, each difference as (right side) - (left side) with both
// sides added in one order, so equal means give exactly 0. The guide exp(-G(gt_image)) * mask is computed
// once per pixel for the three terms. Per term the workgroup adds its pixels (butterfly in the wave, the four
// waves in order) into one partial; the depth term's selected-pixel count is an integer. A finishing kernel,
// one workgroup per term, adds the partials in a fixed order in f64 and divides: no float atomics.
//
// Backward: one launch, nothing saved. Means on halo 2 (20x20), the guide and the signs of the two Sobel
// responses on halo 1 (18x18, zero outside the image), then the adjoint of both filters on the tile, the
// division by the channel count, and the pointwise derivatives; each gradient map is written once.
//
// Compiled with -ffp-contract=off (build.py): every operation rounds on its own, so the exact zeros above and
// "upstream scale multiplies last" (a loss scaled by k gives fl(k * gradient)) hold.
#include <cstdint>

#include "r3dg_common.h"

namespace r3dg {
namespace {

constexpr int kTile = 16;
constexpr int kThreads = kTile * kTile;
constexpr int kP1 = kTile + 2, kP1N = kP1 * kP1;  // halo 1: 18 x 18
constexpr int kP2 = kTile + 4, kP2N = kP2 * kP2;  // halo 2: 20 x 20
constexpr int kTerms = R3DG_REG_TERMS;
constexpr float kClampLo = (float)1e-6;           // neilf.py:244: Python doubles, rounded when they meet the f32 tensor
constexpr float kClampHi = (float)(1 - 1e-6);

constexpr unsigned kDepth = 1u << R3DG_REG_DEPTH, kEntropy = 1u << R3DG_REG_MASK_ENTROPY,
                   kNormalRD = 1u << R3DG_REG_NORMAL_RENDER_DEPTH, kNormalMVS = 1u << R3DG_REG_NORMAL_MVS_DEPTH,
                   kBase = 1u << R3DG_REG_BASE_COLOR, kBaseS = 1u << R3DG_REG_BASE_COLOR_SMOOTH,
                   kMetalS = 1u << R3DG_REG_METALLIC_SMOOTH, kRoughS = 1u << R3DG_REG_ROUGHNESS_SMOOTH;
constexpr unsigned kSmooth = kBaseS | kMetalS | kRoughS, kAll = (1u << kTerms) - 1;

struct Maps {
    r3dg_map opacity, depth, normal, pseudo, base, rough, metal, gt, gdepth, mask, mvs;
};

__device__ __forceinline__ float ld(const r3dg_map& m, int c, int y, int x) {
    return m.ptr[(int64_t)c * m.plane_stride + (int64_t)y * m.row_stride + (int64_t)x * m.px_stride];
}
__device__ __forceinline__ float* at(float* p, const r3dg_map& m, int c, int y, int x) {
    return p + ((int64_t)c * m.plane_stride + (int64_t)y * m.row_stride + (int64_t)x * m.px_stride);
}
__device__ __forceinline__ float mean3(const r3dg_map& m, int y, int x) {
    return ((ld(m, 0, y, x) + ld(m, 1, y, x)) + ld(m, 2, y, x)) / 3.0f;
}
__device__ __forceinline__ float sgn(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }

// The two Sobel responses at centre c of a patch with row stride `stride` (loss_utils.py:69-79, a
// cross-correlation): gx = right column - left column, gy = bottom row - top row, weights 1 2 1.
__device__ __forceinline__ void sobel(const float* s, int c, int stride, float& gx, float& gy) {
    const float t0 = s[c - stride - 1], t1 = s[c - stride], t2 = s[c - stride + 1];
    const float m0 = s[c - 1], m2 = s[c + 1];
    const float b0 = s[c + stride - 1], b1 = s[c + stride], b2 = s[c + stride + 1];
    gx = ((t2 + 2.0f * m2) + b2) - ((t0 + 2.0f * m0) + b0);
    gy = ((b0 + 2.0f * b1) + b2) - ((t0 + 2.0f * t1) + t2);
}

// neilf.py:287-296: the guide's target for channel value g = gt * mask, with v the largest of the three
__device__ __forceinline__ float base_target(float g, float w) {
    return w * (g * g) + (1.0f - w) * (1.0f - (1.0f - g) * (1.0f - g));
}
__device__ __forceinline__ float specular_weight(float v) { return 1.0f / (1.0f + expf(-5.0f * (v - 0.5f))); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// fills dst (edge `edge`, origin (y0 - halo, x0 - halo)) with the channel mean of m, zero outside the image
template <int CH>
__device__ __forceinline__ void fill_mean(float* dst, const r3dg_map& m, int edge, int halo, int y0, int x0, int H,
                                          int W) {
    for (int i = threadIdx.x; i < edge * edge; i += kThreads) {
        const int y = y0 - halo + i / edge, x = x0 - halo + i % edge;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        dst[i] = in ? (CH == 3 ? mean3(m, y, x) : ld(m, 0, y, x)) : 0.0f;
    }
}

// partial: [kTerms][tiles] f32 sums, then [tiles] int32 counts of the depth term's selected pixels
__global__ void __launch_bounds__(kThreads) reg_loss_forward_kernel(int H, int W, int tiles_x, int tiles,
                                                                   unsigned terms, Maps m,
                                                                   float* __restrict__ partial) {
    __shared__ float s_gt[kP1N], s_base[kP1N], s_rough[kP1N], s_metal[kP1N];
    __shared__ float s_red[kThreads / 64][kTerms];
    __shared__ int s_cnt[kThreads / 64];
    const int tid = threadIdx.x;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * kTile, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kTile;
    if (terms & kSmooth) {
        fill_mean<3>(s_gt, m.gt, kP1, 1, y0, x0, H, W);
        if (terms & kBaseS) fill_mean<3>(s_base, m.base, kP1, 1, y0, x0, H, W);
        if (terms & kRoughS) fill_mean<1>(s_rough, m.rough, kP1, 1, y0, x0, H, W);
        if (terms & kMetalS) fill_mean<1>(s_metal, m.metal, kP1, 1, y0, x0, H, W);
        __syncthreads();
    }
    const int lx = tid % kTile, ly = tid / kTile, x = x0 + lx, y = y0 + ly;
    float v[kTerms];
#pragma unroll
    for (int t = 0; t < kTerms; ++t) v[t] = 0.0f;
    int cnt = 0;
    if (x < W && y < H) {
        const float mk = m.mask.ptr ? ld(m.mask, 0, y, x) : 1.0f;
        const float gd = (terms & (kDepth | kNormalMVS)) ? ld(m.gdepth, 0, y, x) : 0.0f;
        if (terms & kDepth) {
            if ((mk != 0.0f) == (gd > 0.0f)) {  // ~xor(image_mask.bool(), gt_depth > 0)
                v[R3DG_REG_DEPTH] = fabsf(ld(m.depth, 0, y, x) - gd);
                cnt = 1;
            }
        }
        if (terms & kEntropy) {
            float o = ld(m.opacity, 0, y, x);
            o = o < kClampLo ? kClampLo : (o > kClampHi ? kClampHi : o);  // a NaN stays NaN, as torch's clamp
            v[R3DG_REG_MASK_ENTROPY] = -(mk * logf(o) + (1.0f - mk) * logf(1.0f - o));
        }
        if (terms & (kNormalRD | kNormalMVS)) {
            const float dm = gd > 0.0f ? 1.0f : 0.0f;
            float a = 0.0f, b = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float n = ld(m.normal, c, y, x);
                if (terms & kNormalRD) {
                    const float d = n * mk - ld(m.pseudo, c, y, x) * mk;
                    a += d * d;
                }
                if (terms & kNormalMVS) {
                    const float d = n * dm - ld(m.mvs, c, y, x) * dm;
                    b += d * d;
                }
            }
            v[R3DG_REG_NORMAL_RENDER_DEPTH] = a;
            v[R3DG_REG_NORMAL_MVS_DEPTH] = b;
        }
        if (terms & kBase) {
            const float g0 = ld(m.gt, 0, y, x) * mk, g1 = ld(m.gt, 1, y, x) * mk, g2 = ld(m.gt, 2, y, x) * mk;
            const float w = specular_weight(fmaxf(fmaxf(g0, g1), g2));
            v[R3DG_REG_BASE_COLOR] = (fabsf(base_target(g0, w) - ld(m.base, 0, y, x)) +
                                      fabsf(base_target(g1, w) - ld(m.base, 1, y, x))) +
                                     fabsf(base_target(g2, w) - ld(m.base, 2, y, x));
        }
        if (terms & kSmooth) {
            const int c = (ly + 1) * kP1 + lx + 1;
            float gx, gy;
            sobel(s_gt, c, kP1, gx, gy);
            const float e = expf(-(fabsf(gx) + fabsf(gy))) * mk;  // shared by the three terms
            if (terms & kBaseS) {
                sobel(s_base, c, kP1, gx, gy);
                v[R3DG_REG_BASE_COLOR_SMOOTH] = (fabsf(gx) + fabsf(gy)) * e;
            }
            if (terms & kMetalS) {
                sobel(s_metal, c, kP1, gx, gy);
                v[R3DG_REG_METALLIC_SMOOTH] = (fabsf(gx) + fabsf(gy)) * e;
            }
            if (terms & kRoughS) {
                sobel(s_rough, c, kP1, gx, gy);
                v[R3DG_REG_ROUGHNESS_SMOOTH] = (fabsf(gx) + fabsf(gy)) * e;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kTerms; ++t) {
        v[t] = wave_sum(v[t]);
        if ((tid & 63) == 0) s_red[tid >> 6][t] = v[t];
    }
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid < kTerms) {
        float s = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) s += s_red[w][tid];
        partial[(int64_t)tid * tiles + blockIdx.x] = s;
    } else if (tid == kTerms) {
        int c = s_cnt[0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) c += s_cnt[w];
        ((int*)(partial + (int64_t)kTerms * tiles))[blockIdx.x] = c;
    }
}

// One workgroup per term: values[t] = (the term's partials added in a fixed order in f64: thread k takes
// partials k, k + 256, ..., then a tree) / (its denominator); 0 for a disabled term. The depth term's
// denominator is its exact integer count, written to depth_count; 0 / 0 is the NaN of the reference's
// F.l1_loss over an empty selection.
__global__ void __launch_bounds__(kThreads) reg_loss_finish_kernel(int tiles, unsigned terms, double n_px,
                                                                  const float* __restrict__ partial,
                                                                  float* __restrict__ values,
                                                                  int* __restrict__ depth_count) {
    __shared__ double s_acc[kThreads];
    __shared__ long long s_cnt[kThreads];
    const int t = blockIdx.x, tid = threadIdx.x;
    if (!(terms >> t & 1u)) {
        if (tid == 0) {
            values[t] = 0.0f;
            if (t == R3DG_REG_DEPTH) *depth_count = 0;
        }
        return;
    }
    const float* p = partial + (int64_t)t * tiles;
    const int* pc = (const int*)(partial + (int64_t)kTerms * tiles);
    double a = 0.0;
    long long c = 0;
    for (int i = tid; i < tiles; i += kThreads) {
        a += (double)p[i];
        if (t == R3DG_REG_DEPTH) c += pc[i];
    }
    s_acc[tid] = a;
    s_cnt[tid] = c;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            s_acc[tid] += s_acc[tid + s];
            s_cnt[tid] += s_cnt[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double den = n_px;
        if (t == R3DG_REG_DEPTH) {
            den = (double)s_cnt[0];
            *depth_count = (int)s_cnt[0];  // <= H * W <= INT32_MAX
        } else if (t == R3DG_REG_NORMAL_RENDER_DEPTH || t == R3DG_REG_NORMAL_MVS_DEPTH || t == R3DG_REG_BASE_COLOR) {
            den = 3.0 * n_px;
        }
        values[t] = (float)(s_acc[0] / den);
    }
}

struct Grads {
    float *opacity, *depth, *normal, *base, *rough, *metal;
};

// 18x18: per data map the guide times the sign of each Sobel response times the term's weight / N
__device__ __forceinline__ void signed_guide(const float* s_mean, int c2, float coef, float* s_a, float* s_b, int j) {
    float gx, gy;
    sobel(s_mean, c2, kP2, gx, gy);
    s_a[j] = coef * sgn(gx);
    s_b[j] = coef * sgn(gy);
}
// the adjoint of both filters at centre c of the 18x18 planes: d(sum) / d(mean at this pixel)
__device__ __forceinline__ float sobel_adjoint(const float* a, const float* b, int c) {
    const float dx = ((a[c - kP1 - 1] + 2.0f * a[c - 1]) + a[c + kP1 - 1]) -
                     ((a[c - kP1 + 1] + 2.0f * a[c + 1]) + a[c + kP1 + 1]);
    const float dy = ((b[c - kP1 - 1] + 2.0f * b[c - kP1]) + b[c - kP1 + 1]) -
                     ((b[c + kP1 - 1] + 2.0f * b[c + kP1]) + b[c + kP1 + 1]);
    return dx + dy;
}

__global__ void __launch_bounds__(kThreads) reg_loss_backward_kernel(int H, int W, int tiles_x, unsigned terms,
                                                                    float inv_n, Maps m,
                                                                    const int* __restrict__ depth_count,
                                                                    const float* __restrict__ weights,
                                                                    const float* __restrict__ scale, Grads g) {
    __shared__ float s_gt[kP2N], s_base[kP2N], s_rough[kP2N], s_metal[kP2N];
    __shared__ float s_a[3][kP1N], s_b[3][kP1N];  // base colour, metallic, roughness
    const int tid = threadIdx.x;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * kTile, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kTile;
    const unsigned smooth = terms & kSmooth;
    if (smooth) {
        fill_mean<3>(s_gt, m.gt, kP2, 2, y0, x0, H, W);
        if (smooth & kBaseS) fill_mean<3>(s_base, m.base, kP2, 2, y0, x0, H, W);
        if (smooth & kRoughS) fill_mean<1>(s_rough, m.rough, kP2, 2, y0, x0, H, W);
        if (smooth & kMetalS) fill_mean<1>(s_metal, m.metal, kP2, 2, y0, x0, H, W);
        __syncthreads();
        const float w_base = (smooth & kBaseS) ? weights[R3DG_REG_BASE_COLOR_SMOOTH] * inv_n : 0.0f;
        const float w_metal = (smooth & kMetalS) ? weights[R3DG_REG_METALLIC_SMOOTH] * inv_n : 0.0f;
        const float w_rough = (smooth & kRoughS) ? weights[R3DG_REG_ROUGHNESS_SMOOTH] * inv_n : 0.0f;
        for (int j = tid; j < kP1N; j += kThreads) {
            const int y = y0 - 1 + j / kP1, x = x0 - 1 + j % kP1;
            const bool in = y >= 0 && y < H && x >= 0 && x < W;
            const int c2 = (j / kP1 + 1) * kP2 + j % kP1 + 1;
            float e = 0.0f;
            if (in) {
                float gx, gy;
                sobel(s_gt, c2, kP2, gx, gy);
                e = expf(-(fabsf(gx) + fabsf(gy))) * (m.mask.ptr ? ld(m.mask, 0, y, x) : 1.0f);
            }
            if (smooth & kBaseS) {
                if (in) signed_guide(s_base, c2, w_base * e, s_a[0], s_b[0], j);
                else s_a[0][j] = s_b[0][j] = 0.0f;
            }
            if (smooth & kMetalS) {
                if (in) signed_guide(s_metal, c2, w_metal * e, s_a[1], s_b[1], j);
                else s_a[1][j] = s_b[1][j] = 0.0f;
            }
            if (smooth & kRoughS) {
                if (in) signed_guide(s_rough, c2, w_rough * e, s_a[2], s_b[2], j);
                else s_a[2][j] = s_b[2][j] = 0.0f;
            }
        }
        __syncthreads();
    }
    const int lx = tid % kTile, ly = tid / kTile, x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    const float k = scale ? scale[0] : 1.0f;  // multiplies last
    const int c = (ly + 1) * kP1 + lx + 1;
    const float mk = m.mask.ptr ? ld(m.mask, 0, y, x) : 1.0f;
    const float gd = (terms & (kDepth | kNormalMVS)) ? ld(m.gdepth, 0, y, x) : 0.0f;

    if (g.depth) {  // the depth term alone reaches it
        const int n = *depth_count;
        float d = 0.0f;
        if (n > 0 && (mk != 0.0f) == (gd > 0.0f))
            d = (weights[R3DG_REG_DEPTH] / (float)n) * sgn(ld(m.depth, 0, y, x) - gd);
        *at(g.depth, m.depth, 0, y, x) = d * k;
    }
    if (g.opacity) {  // the mask entropy alone
        const float o = ld(m.opacity, 0, y, x);
        float d = 0.0f;
        if (o >= kClampLo && o <= kClampHi)  // torch's clamp backward: inside the bounds, inclusive
            d = -(weights[R3DG_REG_MASK_ENTROPY] * inv_n) * (mk / o - (1.0f - mk) / (1.0f - o));
        *at(g.opacity, m.opacity, 0, y, x) = d * k;
    }
    if (g.normal) {  // the two normal terms into one gradient
        const float dm = gd > 0.0f ? 1.0f : 0.0f;
        const float w_rd = (terms & kNormalRD) ? weights[R3DG_REG_NORMAL_RENDER_DEPTH] * (inv_n / 3.0f) : 0.0f;
        const float w_mvs = (terms & kNormalMVS) ? weights[R3DG_REG_NORMAL_MVS_DEPTH] * (inv_n / 3.0f) : 0.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float n = ld(m.normal, ch, y, x);
            float d = 0.0f;
            if (terms & kNormalRD) d = w_rd * ((2.0f * (n * mk - ld(m.pseudo, ch, y, x) * mk)) * mk);
            if (terms & kNormalMVS) d += w_mvs * ((2.0f * (n * dm - ld(m.mvs, ch, y, x) * dm)) * dm);
            *at(g.normal, m.normal, ch, y, x) = d * k;
        }
    }
    if (g.base) {  // the guide and the smoothness term into one gradient
        const float ds = (terms & kBaseS) ? sobel_adjoint(s_a[0], s_b[0], c) / 3.0f : 0.0f;
        float gm[3] = {0.0f, 0.0f, 0.0f}, w = 0.0f, w_guide = 0.0f;
        if (terms & kBase) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) gm[ch] = ld(m.gt, ch, y, x) * mk;
            w = specular_weight(fmaxf(fmaxf(gm[0], gm[1]), gm[2]));
            w_guide = weights[R3DG_REG_BASE_COLOR] * (inv_n / 3.0f);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float d = ds;
            if (terms & kBase) d += w_guide * -sgn(base_target(gm[ch], w) - ld(m.base, ch, y, x));
            *at(g.base, m.base, ch, y, x) = d * k;
        }
    }
    if (g.metal) *at(g.metal, m.metal, 0, y, x) = sobel_adjoint(s_a[1], s_b[1], c) * k;
    if (g.rough) *at(g.rough, m.rough, 0, y, x) = sobel_adjoint(s_a[2], s_b[2], c) * k;
}

struct Geometry {
    int tiles_x, tiles;
};

// the checks both entry points share; tiles == 0 when there is no work. Order: the struct and the signs of H
// and W first, then "nothing to do" (an empty image or no term), and only then the int32 bound and the maps
int check_inputs(const char* who, const r3dg_reg_loss_inputs* in, Maps& m, Geometry& geo) {
    const std::string w(who);
    R3DG_REQUIRE(in, w + ": null inputs");
    R3DG_REQUIRE(in->struct_size == sizeof(r3dg_reg_loss_inputs), w + ": unknown r3dg_reg_loss_inputs.struct_size");
    R3DG_REQUIRE(in->H >= 0 && in->W >= 0, w + ": negative H / W");
    R3DG_REQUIRE((in->terms & ~kAll) == 0, w + ": unknown bits in terms");
    geo = Geometry{0, 0};
    const unsigned t = in->terms;
    if (in->H == 0 || in->W == 0 || t == 0) return R3DG_OK;
    R3DG_REQUIRE((long long)in->H * in->W <= 0x7fffffffll, w + ": H * W exceeds int32");
    R3DG_REQUIRE(!(t & kDepth) || (in->depth.ptr && in->gt_depth.ptr), w + ": the depth term needs depth and gt_depth");
    R3DG_REQUIRE(!(t & kEntropy) || in->opacity.ptr, w + ": the mask entropy term needs opacity");
    R3DG_REQUIRE(!(t & kNormalRD) || (in->normal.ptr && in->pseudo_normal.ptr),
                 w + ": the normal_render_depth term needs normal and pseudo_normal");
    R3DG_REQUIRE(!(t & kNormalMVS) || (in->normal.ptr && in->mvs_normal.ptr && in->gt_depth.ptr),
                 w + ": the normal_mvs_depth term needs normal, mvs_normal and gt_depth");
    R3DG_REQUIRE(!(t & (kBase | kSmooth)) || in->gt_image.ptr, w + ": the base colour and smoothness terms need gt_image");
    R3DG_REQUIRE(!(t & (kBase | kBaseS)) || in->base_color.ptr, w + ": the base colour terms need base_color");
    R3DG_REQUIRE(!(t & kMetalS) || in->metallic.ptr, w + ": the metallic smoothness term needs metallic");
    R3DG_REQUIRE(!(t & kRoughS) || in->roughness.ptr, w + ": the roughness smoothness term needs roughness");
    m = Maps{in->opacity, in->depth, in->normal, in->pseudo_normal, in->base_color, in->roughness,
             in->metallic, in->gt_image, in->gt_depth, in->image_mask, in->mvs_normal};
    geo.tiles_x = (in->W + kTile - 1) / kTile;
    geo.tiles = (int)((long long)geo.tiles_x * ((in->H + kTile - 1) / kTile));  // <= H * W
    return R3DG_OK;
}

}  // namespace
}  // namespace r3dg

using namespace r3dg;

extern "C" int r3dg_reg_loss_forward(const r3dg_reg_loss_inputs* in, float* values, int32_t* depth_count,
                                     r3dg_alloc_fn scratch_alloc, void* scratch_ctx, r3dg_stream_t stream) {
    Maps m;
    Geometry geo;
    if (int rc = check_inputs("reg_loss_forward", in, m, geo)) return rc;
    if (geo.tiles == 0) return R3DG_OK;
    R3DG_REQUIRE(values && depth_count, "reg_loss_forward: null values / depth_count");
    R3DG_REQUIRE(scratch_alloc, "reg_loss_forward: null scratch_alloc");
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)scratch_alloc(scratch_ctx, sizeof(float) * (kTerms + 1) * (size_t)geo.tiles);
    if (!partial) {
        set_error("reg_loss_forward: scratch allocation failed");
        return R3DG_ERR_ALLOC;
    }
    hipLaunchKernelGGL(reg_loss_forward_kernel, dim3((unsigned)geo.tiles), dim3(kThreads), 0, st, in->H, in->W,
                       geo.tiles_x, geo.tiles, in->terms, m, partial);
    R3DG_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(reg_loss_finish_kernel, dim3(kTerms), dim3(kThreads), 0, st, geo.tiles, in->terms,
                       (double)in->H * (double)in->W, partial, values, (int*)depth_count);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}

extern "C" int r3dg_reg_loss_backward(const r3dg_reg_loss_inputs* in, const int32_t* depth_count,
                                      const float* weights, const float* scale, const r3dg_reg_loss_grads* out,
                                      r3dg_stream_t stream) {
    Maps m;
    Geometry geo;
    if (int rc = check_inputs("reg_loss_backward", in, m, geo)) return rc;
    R3DG_REQUIRE(out, "reg_loss_backward: null grads");
    R3DG_REQUIRE(out->struct_size == sizeof(r3dg_reg_loss_grads),
                 "reg_loss_backward: unknown r3dg_reg_loss_grads.struct_size");
    if (geo.tiles == 0) return R3DG_OK;
    R3DG_REQUIRE(weights, "reg_loss_backward: null weights");
    const unsigned t = in->terms;
    // a map that no enabled term reaches gets no gradient, whatever the caller passed
    Grads g{(t & kEntropy) ? out->opacity : nullptr,
            (t & kDepth) ? out->depth : nullptr,
            (t & (kNormalRD | kNormalMVS)) ? out->normal : nullptr,
            (t & (kBase | kBaseS)) ? out->base_color : nullptr,
            (t & kRoughS) ? out->roughness : nullptr,
            (t & kMetalS) ? out->metallic : nullptr};
    R3DG_REQUIRE(!g.depth || depth_count, "reg_loss_backward: the depth gradient needs depth_count");
    if (!(g.opacity || g.depth || g.normal || g.base || g.rough || g.metal)) return R3DG_OK;
    // smoothness work only for the maps whose gradient is wanted
    unsigned run = t;
    if (!g.base) run &= ~(kBase | kBaseS);
    if (!g.rough) run &= ~kRoughS;
    if (!g.metal) run &= ~kMetalS;
    const float inv_n = (float)(1.0 / ((double)in->H * (double)in->W));
    hipLaunchKernelGGL(reg_loss_backward_kernel, dim3((unsigned)geo.tiles), dim3(kThreads), 0, (hipStream_t)stream,
                       in->H, in->W, geo.tiles_x, run, inv_n, m, (const int*)depth_count, weights, scale, g);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}
