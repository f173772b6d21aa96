// visibility.hip -- the visibility-SH fit around the tracer (gfx950): the L1 loss between traced
// visibility and the baked visibility SH, its gradient, and a fit step with Adam fused in.
//
// Restates the reference's torch code around RayTracer.trace_visibility at two call sites:
// gaussian_renderer/neilf.py:331-346 (the lambda_visibility training term: eval_sh, clamp, F.l1_loss
// and their autograd) and scene/gaussian_model.py:446-462 (finetune_visibility: the same per
// iteration plus torch.optim.Adam over visibility_dc / visibility_rest). There these are ~50
// elementwise launches forward over [R, K] temporaries, as many backward, and a foreach Adam.
//
// One lane per ray does everything that belongs to the ray (ray_eval): the direction after the call
// sites' hemisphere flip (sh_dirs.h flip_to_normal, the tracer's own), the K basis factors, the SH
// sum in the reference's order, clamp and |traced - s|. The coefficients are read from the two
// parameter arrays as they are stored ([P,1,1] and [P,K-1,1]); no concatenated copy exists.
//   * loss forward: per-block partial sums (lanes in order within a wave, waves in order), then a
//     finishing workgroup adds the partials in a fixed order in f64 and divides by R: no float
//     atomics, so the loss is bit-reproducible (the pattern of loss.hip / reg_loss.hip);
//   * loss backward: the same evaluation, then upstream * sign * [clamp open] * basis_k / R stored to
//     the dense gradient row (without index: every row is written once, nothing is cleared; with
//     index: the rows are cleared first and added with atomics, so a row named twice accumulates);
//   * fit step: R = P, the gradient stays in registers and goes straight into Adam for the K
//     coefficients of the lane's Gaussian, with the arithmetic of optim.hip's adam_elem; a zero
//     gradient still decays the moments and moves the parameter, as torch.optim.Adam does for a
//     present gradient. The loss partials come from the same launch.
// Built with -ffp-contract=off: a float32 numpy restatement reproduces the flip decision and the
// basis factors bit for bit.
#include <cmath>

#include "r3dg_common.h"
#include "sh_dirs.h"

namespace r3dg {
namespace {

constexpr int kThreads = 256;

struct VisArgs {
    int P, K, R;
    float* sh_dc;          // [P]
    float* sh_rest;        // [P, K - 1]
    const float* dirs;     // [R, 3]
    const float* traced;   // [R]
    const float* normals;  // [P, 3] or null: no flip
    const int32_t* index;  // [R] or null: ray r belongs to Gaussian r
    float* partial;        // [blocks] (forward, fit)
    const float* upstream; // device scalar (backward)
    float* grad_dc;        // [P]
    float* grad_rest;      // [P, K - 1]
    // fit
    float *m_dc, *m_rest, *v_dc, *v_rest;
    float neg_step, bc2_sqrt, omb1, beta2, omb2, eps;
};

struct RayEval {
    float term;   // |traced - s|
    float sgn;    // d term / d raw: sign(s - traced) where the clamp is open, else 0
};

// Everything of one ray. basis[K] is filled for the caller's gradient. g must be a valid row.
__device__ __forceinline__ RayEval ray_eval(const VisArgs& a, int r, int g, float* basis) {
    float3 d = make_float3(a.dirs[3 * (size_t)r], a.dirs[3 * (size_t)r + 1], a.dirs[3 * (size_t)r + 2]);
    if (a.normals)
        d = flip_to_normal(d, make_float3(a.normals[3 * (size_t)g], a.normals[3 * (size_t)g + 1],
                                          a.normals[3 * (size_t)g + 2]));
    eval_sh_basis(a.K, d.x, d.y, d.z, basis);
    float raw = basis[0] * a.sh_dc[g];
    const float* rest = a.sh_rest + (size_t)g * (a.K - 1);
#pragma unroll
    for (int k = 1; k < kMaxSH; ++k)
        if (k < a.K) raw = raw + basis[k] * rest[k - 1];
    const float u = raw + 0.5f;
    const float s = fminf(fmaxf(u, 0.0f), 1.0f);
    const float t = a.traced[r];
    const float diff = s - t;
    RayEval e;
    e.term = fabsf(diff);
    // torch's clamp backward passes the gradient at the bounds (inclusive); sign(0) = 0
    const bool open = u >= 0.0f && u <= 1.0f;
    e.sgn = open ? (diff > 0.0f ? 1.0f : diff < 0.0f ? -1.0f : 0.0f) : 0.0f;
    return e;
}

// sum over the block in a fixed order: lanes of a wave by butterfly, the four waves in order
__device__ __forceinline__ void block_partial(float v, float* partial) {
    __shared__ float s_w[kThreads / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// the Gaussian of ray r; -1 for an index outside [0, P) (the caller's error: the loss becomes NaN, no
// memory outside the arrays is touched)
__device__ __forceinline__ int ray_row(const VisArgs& a, int r) {
    if (!a.index) return r;
    const int g = a.index[r];
    return (unsigned)g < (unsigned)a.P ? g : -1;
}

__global__ void __launch_bounds__(kThreads) vis_loss_fwd_kernel(VisArgs a) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    float term = 0.0f;
    if (r < a.R) {
        const int g = ray_row(a, r);
        float basis[kMaxSH];
        term = g >= 0 ? ray_eval(a, r, g, basis).term : NAN;
    }
    block_partial(term, a.partial);
}

// loss = (partials added in a fixed order in f64: thread k takes k, k + 256, ..., then a tree) / R
__global__ void __launch_bounds__(kThreads) vis_loss_finish_kernel(int n, const float* __restrict__ partial, double R,
                                                                   float* __restrict__ loss) {
    __shared__ double s_acc[kThreads];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) acc += (double)partial[i];
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_acc[threadIdx.x] += s_acc[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(s_acc[0] / R);
}

__global__ void __launch_bounds__(kThreads) vis_loss_bwd_kernel(VisArgs a) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= a.R) return;
    const int g = ray_row(a, r);
    if (g < 0) return;
    float basis[kMaxSH];
    const RayEval e = ray_eval(a, r, g, basis);
    const float c = *a.upstream * e.sgn;
    const float fR = (float)a.R;
    float* rest = a.grad_rest + (size_t)g * (a.K - 1);
    if (a.index) {
        if (c == 0.0f) return;  // the rows were cleared
        atomicAdd(a.grad_dc + g, c * basis[0] / fR);
#pragma unroll
        for (int k = 1; k < kMaxSH; ++k)
            if (k < a.K) atomicAdd(rest + k - 1, c * basis[k] / fR);
    } else {
        a.grad_dc[g] = c * basis[0] / fR;
#pragma unroll
        for (int k = 1; k < kMaxSH; ++k)
            if (k < a.K) rest[k - 1] = c * basis[k] / fR;
    }
}

// optim.hip adam_elem: torch.optim.Adam's m = lerp(m, g, 1 - b1); v = b2 v + (1 - b2) g^2;
// p += -(lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
__device__ __forceinline__ void fit_adam(const VisArgs& a, float g, float* p, float* m, float* v) {
    float mm = *m, vv = *v;
    mm = __builtin_fmaf(a.omb1, g - mm, mm);
    vv = vv * a.beta2;
    vv = __builtin_fmaf(a.omb2, g * g, vv);
    const float denom = sqrtf(vv) / a.bc2_sqrt + a.eps;
    *p = __builtin_fmaf(a.neg_step, mm / denom, *p);
    *m = mm;
    *v = vv;
}

// R = P, no index: gradient (upstream 1) and Adam for the K coefficients of Gaussian r in one pass
__global__ void __launch_bounds__(kThreads) vis_fit_kernel(VisArgs a) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    float term = 0.0f;
    if (r < a.R) {
        float basis[kMaxSH];
        const RayEval e = ray_eval(a, r, r, basis);
        term = e.term;
        const float fR = (float)a.R;
        fit_adam(a, e.sgn * basis[0] / fR, a.sh_dc + r, a.m_dc + r, a.v_dc + r);
        const size_t row = (size_t)r * (a.K - 1);
#pragma unroll
        for (int k = 1; k < kMaxSH; ++k)
            if (k < a.K)
                fit_adam(a, e.sgn * basis[k] / fR, a.sh_rest + row + k - 1, a.m_rest + row + k - 1,
                         a.v_rest + row + k - 1);
    }
    block_partial(term, a.partial);
}

inline unsigned vis_blocks(int n) { return (unsigned)(((long long)n + kThreads - 1) / kThreads); }

}  // namespace
}  // namespace r3dg

using namespace r3dg;

static int check_vis_inputs(const r3dg_visibility_sh_inputs* in, const char* who, bool fit) {
    const std::string w(who);
    R3DG_REQUIRE(in && in->struct_size == sizeof(r3dg_visibility_sh_inputs),
                 w + ": r3dg_visibility_sh_inputs.struct_size does not match this library");
    R3DG_REQUIRE(in->K == 1 || in->K == 4 || in->K == 9 || in->K == 16 || in->K == 25,
                 w + ": K must be 1, 4, 9, 16 or 25 coefficients (eval_sh degrees 0..4)");
    R3DG_REQUIRE(in->P >= 1 && in->R >= 1, w + ": P and R must be at least 1 (the mean over no ray is undefined)");
    R3DG_REQUIRE(in->sh_dc && (in->K == 1 || in->sh_rest) && in->dirs && in->traced, w + ": null buffer");
    R3DG_REQUIRE(in->index || in->R == in->P, w + ": without index, R must equal P (one ray per Gaussian)");
    R3DG_REQUIRE(!fit || !in->index, w + ": the fit step takes no index");
    return R3DG_OK;
}

static VisArgs vis_args(const r3dg_visibility_sh_inputs* in) {
    VisArgs a{};
    a.P = in->P; a.K = in->K; a.R = in->R;
    a.sh_dc = in->sh_dc; a.sh_rest = in->sh_rest; a.dirs = in->dirs; a.traced = in->traced;
    a.normals = in->normals; a.index = in->index;
    return a;
}

static int finish_loss(const VisArgs& a, float* loss, hipStream_t st) {
    hipLaunchKernelGGL(vis_loss_finish_kernel, dim3(1), dim3(kThreads), 0, st, (int)vis_blocks(a.R), a.partial,
                       (double)a.R, loss);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}

extern "C" int r3dg_visibility_sh_loss_forward(const r3dg_visibility_sh_inputs* in, float* loss,
                                               r3dg_alloc_fn scratch_alloc, void* scratch_ctx, r3dg_stream_t stream) {
    if (int e = check_vis_inputs(in, "visibility_sh_loss_forward", false)) return e;
    R3DG_REQUIRE(loss && scratch_alloc, "visibility_sh_loss_forward: null argument");
    VisArgs a = vis_args(in);
    a.partial = (float*)scratch_alloc(scratch_ctx, sizeof(float) * (size_t)vis_blocks(a.R));
    R3DG_REQUIRE(a.partial, "visibility_sh_loss_forward: scratch allocation failed");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(vis_loss_fwd_kernel, dim3(vis_blocks(a.R)), dim3(kThreads), 0, st, a);
    R3DG_CHECK_HIP(hipGetLastError());
    return finish_loss(a, loss, st);
}

extern "C" int r3dg_visibility_sh_loss_backward(const r3dg_visibility_sh_inputs* in, const float* upstream,
                                                float* grad_dc, float* grad_rest, r3dg_stream_t stream) {
    if (int e = check_vis_inputs(in, "visibility_sh_loss_backward", false)) return e;
    R3DG_REQUIRE(upstream && grad_dc && (in->K == 1 || grad_rest), "visibility_sh_loss_backward: null argument");
    VisArgs a = vis_args(in);
    a.upstream = upstream; a.grad_dc = grad_dc; a.grad_rest = grad_rest;
    hipStream_t st = (hipStream_t)stream;
    if (a.index) {
        R3DG_CHECK_HIP(hipMemsetAsync(grad_dc, 0, sizeof(float) * (size_t)a.P, st));
        if (a.K > 1) R3DG_CHECK_HIP(hipMemsetAsync(grad_rest, 0, sizeof(float) * (size_t)a.P * (a.K - 1), st));
    }
    hipLaunchKernelGGL(vis_loss_bwd_kernel, dim3(vis_blocks(a.R)), dim3(kThreads), 0, st, a);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}

extern "C" int r3dg_visibility_sh_fit_step(const r3dg_visibility_sh_inputs* in, const r3dg_visibility_fit* fit,
                                           float* loss, r3dg_alloc_fn scratch_alloc, void* scratch_ctx,
                                           r3dg_stream_t stream) {
    if (int e = check_vis_inputs(in, "visibility_sh_fit_step", true)) return e;
    R3DG_REQUIRE(fit && fit->struct_size == sizeof(r3dg_visibility_fit),
                 "visibility_sh_fit_step: r3dg_visibility_fit.struct_size does not match this library");
    R3DG_REQUIRE(fit->step >= 1, "visibility_sh_fit_step: step must be >= 1");
    R3DG_REQUIRE(loss && scratch_alloc && fit->exp_avg_dc && fit->exp_avg_sq_dc &&
                     (in->K == 1 || (fit->exp_avg_rest && fit->exp_avg_sq_rest)),
                 "visibility_sh_fit_step: null argument");
    VisArgs a = vis_args(in);
    a.m_dc = fit->exp_avg_dc; a.m_rest = fit->exp_avg_rest; a.v_dc = fit->exp_avg_sq_dc; a.v_rest = fit->exp_avg_sq_rest;
    // the bias corrections in double on the host, as r3dg_adam_step
    const double bc1 = 1.0 - std::pow(fit->beta1, (double)fit->step), bc2 = 1.0 - std::pow(fit->beta2, (double)fit->step);
    a.neg_step = (float)(-((double)fit->lr / bc1));
    a.bc2_sqrt = (float)std::sqrt(bc2);
    a.omb1 = (float)(1.0 - fit->beta1); a.beta2 = (float)fit->beta2; a.omb2 = (float)(1.0 - fit->beta2);
    a.eps = (float)fit->eps;
    a.partial = (float*)scratch_alloc(scratch_ctx, sizeof(float) * (size_t)vis_blocks(a.R));
    R3DG_REQUIRE(a.partial, "visibility_sh_fit_step: scratch allocation failed");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(vis_fit_kernel, dim3(vis_blocks(a.R)), dim3(kThreads), 0, st, a);
    R3DG_CHECK_HIP(hipGetLastError());
    return finish_loss(a, loss, st);
}
