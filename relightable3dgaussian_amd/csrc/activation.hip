// activation.hip -- the parameter activations of a training iteration (gfx950): from the flat parameter
// buffer to every per-Gaussian input of the rasterizer, the render equation and the tracer, and from the
// upstream gradients of those inputs straight into the flat gradient buffer.
//
// Restates the reference's torch code between its nn.Parameters and its kernels: the getters of
// scene/gaussian_model.py:23-44, 331-413 (exp, two F.normalize, four sigmoid, three torch.cat of SH blocks,
// get_inverse_covariance = build_rotation + bmm + strip_symmetric) and gaussian_renderer/neilf.py:102
// (F.normalize(camera_center - means3D)). There these are ~20 launches forward, their autograd replays
// backward, a clone per non-contiguous cat slice, and one more pass to copy each .grad into the flat buffer.
//
// Two launches per direction, both streaming:
//   * act_{fwd,bwd}_kernel: one lane per FOUR consecutive Gaussians for the groups up to 4 floats wide (xyz,
//     normal, rotation, scaling, opacity, base_color, roughness, metallic). Four rows of a [P, w] block are w
//     float4s, so every block is read and written with 16-byte accesses whatever w is. Group g starts at
//     float P * sum(width[<g]) of the flat buffer, which for P no multiple of 4 is not 16-byte aligned: every
//     run tests its own address (uniform over the launch) and takes dword accesses when the test fails or
//     the lane holds the tail (P % 4 rows).
//   * sh_{fwd,bwd}_kernel: one lane per 16 B of a concatenated SH row (shs and incidents [P,16,3],
//     visibility [P,16,1]); a workgroup of 192 lanes holds 16 (48) whole rows, so the row and the quad come
//     from the lane index by a constant division. The concatenated side is one float4 per lane; the split
//     side (row p of dc, row p of rest at 45 p or 15 p) has no alignment to use and goes as dwords, which
//     are contiguous across the lanes.
// Backward recomputes the activations from the raw parameters (9 expf per Gaussian beside ~350 B) and saves
// nothing. No atomics, no LDS, no allocation, no host synchronisation; P = 0 launches nothing.
// Built with -ffp-contract=off: the float32 reference is torch tensor code that rounds every operation.
#include "act_device.h"

namespace r3dg {
namespace {

constexpr int kThreads = 256;
constexpr int kShThreads = 192; // 16 rows of 12 float4 (48 floats), or 48 rows of 4 float4 (16 floats)

// four rows of an upstream gradient whose rows are `stride` floats apart (r3dg_grad_rows)
template <int W>
__device__ __forceinline__ void load_rows(const float* ptr, long long stride, long long p0, int rows,
                                          float (&v)[kQuad * W]) {
    if (stride == W) {
        load_run(ptr + p0 * W, rows * W, v);
        return;
    }
#pragma unroll
    for (int r = 0; r < kQuad; ++r)
#pragma unroll
        for (int c = 0; c < W; ++c) v[r * W + c] = r < rows ? ptr[(p0 + r) * stride + c] : 0.0f;
}

// grad[...] = v, or += v
template <int N>
__device__ __forceinline__ void emit(float* p, int n, float (&v)[N], bool accumulate) {
    if (accumulate) {
        float old[N];
        load_run(p, n, old);
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = old[i] + v[i];
    }
    store_run(p, n, v);
}

// its gradient: the projection (g - y (y.g)) / r where the clamp is open (r >= eps, torch's mask, decided
// on the float32 norm as the forward's clamp is), else g / eps. The projection cancels when g is nearly
// parallel to x: in float32 its error is an ulp of |g| / r however small the result is, so how far it lands
// from the exact gradient depends on the worst-aligned row of the data. It is evaluated in double from the
// float32 inputs (x: the same vector in double) and rounded once by the caller; ~40 f64 operations per row
// beside the row's memory traffic.
template <int W>
__device__ __forceinline__ void normalize_bwd(const float* xf, const double* x, const float* g, float eps,
                                              double* out) {
    if (norm_of<W>(xf) >= eps) {
        double ss = x[0] * x[0];
#pragma unroll
        for (int c = 1; c < W; ++c) ss = ss + x[c] * x[c];
        const double inv = 1.0 / sqrt(ss);
        double y[W], dot = 0.0;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            y[c] = x[c] * inv;
            dot = dot + y[c] * (double)g[c];
        }
#pragma unroll
        for (int c = 0; c < W; ++c) out[c] = ((double)g[c] - y[c] * dot) * inv;
    } else {
#pragma unroll
        for (int c = 0; c < W; ++c) out[c] = (double)(g[c] / eps);
    }
}

// d sigmoid / dx = s (1 - s) without forming 1 - s, which loses |x| / ln 2 bits in float32 (at x = 20,
// s rounds to 1 and the product to 0): with t = e^-|x|, s (1 - s) = t / (1 + t)^2, no cancellation and no
// overflow (t <= 1)
__device__ __forceinline__ float sigmoid_slope(float x) {
    const float t = expf(-fabsf(x));
    const float d = 1.0f + t;
    return t / (d * d);
}

struct GradRows {
    const float* ptr;
    long long stride;
};

// group starts inside param (raw) and grad (d_*); a null raw pointer is an absent role
struct ActArgs {
    int P;
    const float *xyz, *scaling, *rotation, *normal, *opacity, *base_color, *roughness, *metallic;
    const float* campos;
    // forward
    float *o_scaling, *o_rotation, *o_normal, *o_opacity, *o_base_color, *o_roughness, *o_metallic, *o_viewdirs,
        *o_symm_inv;
    // backward
    GradRows g_xyz, g_scaling, g_rotation, g_normal, g_opacity, g_base_color, g_roughness, g_metallic, g_viewdirs;
    float *d_xyz, *d_scaling, *d_rotation, *d_normal, *d_opacity, *d_base_color, *d_roughness, *d_metallic;
    int accumulate;
};

// one sigmoid group of width W: forward
template <int W>
__device__ __forceinline__ void sigmoid_fwd(const float* raw, float* out, long long p0, int rows) {
    if (!raw || !out) return;
    float v[kQuad * W];
    load_run(raw + p0 * W, rows * W, v);
#pragma unroll
    for (int i = 0; i < kQuad * W; ++i) v[i] = sigmoid(v[i]);
    store_run(out + p0 * W, rows * W, v);
}

__global__ void __launch_bounds__(kThreads) act_fwd_kernel(ActArgs a) {
    const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kQuad;
    if (p0 >= a.P) return;
    const int rows = a.P - p0 < kQuad ? (int)(a.P - p0) : kQuad;

    if (a.o_viewdirs) {
        float x[kQuad * 3], y[kQuad * 3];
        load_run(a.xyz + p0 * 3, rows * 3, x);
        const float cx = a.campos[0], cy = a.campos[1], cz = a.campos[2];
#pragma unroll
        for (int r = 0; r < kQuad; ++r) {
            const float v[3] = {cx - x[3 * r], cy - x[3 * r + 1], cz - x[3 * r + 2]};
            normalize<3>(v, kEpsUnit, y + 3 * r);
        }
        store_run(a.o_viewdirs + p0 * 3, rows * 3, y);
    }
    if (a.o_normal) {
        float x[kQuad * 3], y[kQuad * 3];
        load_run(a.normal + p0 * 3, rows * 3, x);
#pragma unroll
        for (int r = 0; r < kQuad; ++r) normalize<3>(x + 3 * r, kEpsNormal, y + 3 * r);
        store_run(a.o_normal + p0 * 3, rows * 3, y);
    }
    if (a.o_rotation || a.o_scaling || a.o_symm_inv) {
        float q[kQuad * 4], s[kQuad * 3];
        load_run(a.rotation + p0 * 4, rows * 4, q);
        load_run(a.scaling + p0 * 3, rows * 3, s);
#pragma unroll
        for (int r = 0; r < kQuad; ++r) {
            float qh[4];
            normalize<4>(q + 4 * r, kEpsUnit, qh);
#pragma unroll
            for (int c = 0; c < 4; ++c) q[4 * r + c] = qh[c];
        }
#pragma unroll
        for (int i = 0; i < kQuad * 3; ++i) s[i] = expf(s[i]);
        if (a.o_rotation) store_run(a.o_rotation + p0 * 4, rows * 4, q);
        if (a.o_scaling) store_run(a.o_scaling + p0 * 3, rows * 3, s);
        if (a.o_symm_inv) {
            float o[kQuad * 6];
#pragma unroll
            for (int r = 0; r < kQuad; ++r) symm_inverse(q + 4 * r, s + 3 * r, o + 6 * r);
            store_run(a.o_symm_inv + p0 * 6, rows * 6, o);
        }
    }
    sigmoid_fwd<1>(a.opacity, a.o_opacity, p0, rows);
    sigmoid_fwd<3>(a.base_color, a.o_base_color, p0, rows);
    sigmoid_fwd<1>(a.roughness, a.o_roughness, p0, rows);
    sigmoid_fwd<1>(a.metallic, a.o_metallic, p0, rows);
}

// a group with no upstream: zeros in overwrite mode, untouched in accumulate mode
template <int W>
__device__ __forceinline__ bool no_upstream(const GradRows& g, float* dst, long long p0, int rows, bool accumulate) {
    if (g.ptr) return false;
    if (!accumulate) {
        float z[kQuad * W];
#pragma unroll
        for (int i = 0; i < kQuad * W; ++i) z[i] = 0.0f;
        store_run(dst + p0 * W, rows * W, z);
    }
    return true;
}

template <int W>
__device__ __forceinline__ void sigmoid_bwd(const float* raw, const GradRows& g, float* dst, long long p0, int rows,
                                            bool accumulate) {
    if (!raw || no_upstream<W>(g, dst, p0, rows, accumulate)) return;
    float x[kQuad * W], u[kQuad * W];
    load_run(raw + p0 * W, rows * W, x);
    load_rows<W>(g.ptr, g.stride, p0, rows, u);
#pragma unroll
    for (int i = 0; i < kQuad * W; ++i) u[i] = u[i] * sigmoid_slope(x[i]);
    emit(dst + p0 * W, rows * W, u, accumulate);
}

template <int W>
__device__ __forceinline__ void normalize_group_bwd(const float* raw, const GradRows& g, float eps, float* dst,
                                                    long long p0, int rows, bool accumulate) {
    if (no_upstream<W>(g, dst, p0, rows, accumulate)) return;
    float x[kQuad * W], u[kQuad * W], d[kQuad * W];
    load_run(raw + p0 * W, rows * W, x);
    load_rows<W>(g.ptr, g.stride, p0, rows, u);
#pragma unroll
    for (int r = 0; r < kQuad; ++r) {
        double xd[W], dd[W];
#pragma unroll
        for (int c = 0; c < W; ++c) xd[c] = (double)x[W * r + c];
        normalize_bwd<W>(x + W * r, xd, u + W * r, eps, dd);
#pragma unroll
        for (int c = 0; c < W; ++c) d[W * r + c] = (float)dd[c];
    }
    emit(dst + p0 * W, rows * W, d, accumulate);
}

__global__ void __launch_bounds__(kThreads) act_bwd_kernel(ActArgs a) {
    const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kQuad;
    if (p0 >= a.P) return;
    const int rows = a.P - p0 < kQuad ? (int)(a.P - p0) : kQuad;
    const bool acc = a.accumulate != 0;

    // xyz: the rasterizer's and the tracer's gradient passes through, the view direction's goes through
    // v = campos - xyz (hence the minus)
    if (a.g_xyz.ptr || a.g_viewdirs.ptr || !acc) {
        float d[kQuad * 3];
        if (a.g_xyz.ptr) {
            load_rows<3>(a.g_xyz.ptr, a.g_xyz.stride, p0, rows, d);
        } else {
#pragma unroll
            for (int i = 0; i < kQuad * 3; ++i) d[i] = 0.0f;
        }
        if (a.g_viewdirs.ptr) {
            float x[kQuad * 3], u[kQuad * 3];
            load_run(a.xyz + p0 * 3, rows * 3, x);
            load_rows<3>(a.g_viewdirs.ptr, a.g_viewdirs.stride, p0, rows, u);
            const float cx = a.campos[0], cy = a.campos[1], cz = a.campos[2];
#pragma unroll
            for (int r = 0; r < kQuad; ++r) {
                const float v[3] = {cx - x[3 * r], cy - x[3 * r + 1], cz - x[3 * r + 2]};
                const double vd[3] = {(double)cx - (double)x[3 * r], (double)cy - (double)x[3 * r + 1],
                                      (double)cz - (double)x[3 * r + 2]};
                double dv[3];
                normalize_bwd<3>(v, vd, u + 3 * r, kEpsUnit, dv);
#pragma unroll
                for (int c = 0; c < 3; ++c) d[3 * r + c] = (float)((double)d[3 * r + c] - dv[c]);
            }
        }
        emit(a.d_xyz + p0 * 3, rows * 3, d, acc);
    }
    normalize_group_bwd<3>(a.normal, a.g_normal, kEpsNormal, a.d_normal, p0, rows, acc);
    normalize_group_bwd<4>(a.rotation, a.g_rotation, kEpsUnit, a.d_rotation, p0, rows, acc);
    if (!no_upstream<3>(a.g_scaling, a.d_scaling, p0, rows, acc)) {
        float x[kQuad * 3], u[kQuad * 3];
        load_run(a.scaling + p0 * 3, rows * 3, x);
        load_rows<3>(a.g_scaling.ptr, a.g_scaling.stride, p0, rows, u);
#pragma unroll
        for (int i = 0; i < kQuad * 3; ++i) u[i] = u[i] * expf(x[i]);
        emit(a.d_scaling + p0 * 3, rows * 3, u, acc);
    }
    sigmoid_bwd<1>(a.opacity, a.g_opacity, a.d_opacity, p0, rows, acc);
    sigmoid_bwd<3>(a.base_color, a.g_base_color, a.d_base_color, p0, rows, acc);
    sigmoid_bwd<1>(a.roughness, a.g_roughness, a.d_roughness, p0, rows, acc);
    sigmoid_bwd<1>(a.metallic, a.g_metallic, a.d_metallic, p0, rows, acc);
}

// ---- the three SH concatenations -----------------------------------------------------------------

// array i: split side dc [P, wdc] / rest [P, wrest] (param forward, grad backward), concatenated side cat
// with rows `stride` floats apart (the output forward, the upstream backward; null upstream = zeros).
// blocks[i] workgroups belong to array i (0 = not launched for it).
struct ShArgs {
    int P;
    const float* dc[3];
    const float* rest[3];
    float* d_dc[3];
    float* d_rest[3];
    float* out[3];
    GradRows up[3];
    unsigned blocks[3];
    int accumulate;
};

template <int WDC, int WREST>
__device__ __forceinline__ void sh_fwd_quad(const float* dc, const float* rest, float* out, int P, unsigned block) {
    constexpr int ROW = WDC + WREST, Q = ROW / 4, ROWS = kShThreads / Q;
    static_assert(ROW % 4 == 0 && kShThreads % Q == 0, "whole rows of float4 per workgroup");
    const int r = (int)threadIdx.x / Q, k = (int)threadIdx.x - r * Q;
    const long long p = (long long)block * ROWS + r;
    if (p >= P) return;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = 4 * k + e;
        v[e] = c < WDC ? dc[p * WDC + c] : rest[p * WREST + (c - WDC)];
    }
    float* o = out + p * ROW + 4 * k;
    if (aligned16(o)) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[e];
    }
}

template <int WDC, int WREST>
__device__ __forceinline__ void sh_bwd_quad(const GradRows& up, float* d_dc, float* d_rest, int P, unsigned block,
                                            bool accumulate) {
    constexpr int ROW = WDC + WREST, Q = ROW / 4, ROWS = kShThreads / Q;
    const int r = (int)threadIdx.x / Q, k = (int)threadIdx.x - r * Q;
    const long long p = (long long)block * ROWS + r;
    if (p >= P) return;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (up.ptr) {
        const float* u = up.ptr + p * up.stride + 4 * k;
        if (aligned16(u)) {
            const float4 t = *reinterpret_cast<const float4*>(u);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = u[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = 4 * k + e;
        float* d = c < WDC ? d_dc + p * WDC + c : d_rest + p * WREST + (c - WDC);
        *d = accumulate ? *d + v[e] : v[e];
    }
}

__global__ void __launch_bounds__(kShThreads) sh_fwd_kernel(ShArgs a) {
    unsigned b = blockIdx.x;
    if (b < a.blocks[0]) return sh_fwd_quad<3, 45>(a.dc[0], a.rest[0], a.out[0], a.P, b);
    b -= a.blocks[0];
    if (b < a.blocks[1]) return sh_fwd_quad<3, 45>(a.dc[1], a.rest[1], a.out[1], a.P, b);
    b -= a.blocks[1];
    sh_fwd_quad<1, 15>(a.dc[2], a.rest[2], a.out[2], a.P, b);
}

__global__ void __launch_bounds__(kShThreads) sh_bwd_kernel(ShArgs a) {
    unsigned b = blockIdx.x;
    const bool acc = a.accumulate != 0;
    if (b < a.blocks[0]) return sh_bwd_quad<3, 45>(a.up[0], a.d_dc[0], a.d_rest[0], a.P, b, acc);
    b -= a.blocks[0];
    if (b < a.blocks[1]) return sh_bwd_quad<3, 45>(a.up[1], a.d_dc[1], a.d_rest[1], a.P, b, acc);
    b -= a.blocks[1];
    sh_bwd_quad<1, 15>(a.up[2], a.d_dc[2], a.d_rest[2], a.P, b, acc);
}

}  // namespace
}  // namespace r3dg

using namespace r3dg;

static const float* at(const float* base, long long off) { return off < 0 ? nullptr : base + off; }
static float* at(float* base, long long off) { return off < 0 ? nullptr : base + off; }

static void raw_pointers(ActArgs& a, const Resolved& r, const float* param) {
    a.xyz = at(param, r.xyz); a.scaling = at(param, r.scaling); a.rotation = at(param, r.rotation);
    a.normal = at(param, r.normal); a.opacity = at(param, r.opacity); a.base_color = at(param, r.base_color);
    a.roughness = at(param, r.roughness); a.metallic = at(param, r.metallic);
}

extern "C" int r3dg_activate_forward(const r3dg_activation_io* io, const float* param, r3dg_stream_t stream) {
    Resolved r;
    if (int e = resolve_roles(io, "activate_forward", &r)) return e;
    const int P = io->layout->P;
    R3DG_REQUIRE(!io->out_viewdirs || io->campos, "activate_forward: out_viewdirs needs campos");
    R3DG_REQUIRE(r.pbr || !(io->out_base_color || io->out_roughness || io->out_metallic || io->out_incidents ||
                            io->out_visibility),
                 "activate_forward: an output of an absent role");
    if (P == 0) return R3DG_OK;
    R3DG_REQUIRE(param, "activate_forward: null param");
    hipStream_t st = (hipStream_t)stream;

    ActArgs a{};
    a.P = P;
    raw_pointers(a, r, param);
    a.campos = io->campos;
    a.o_scaling = io->out_scaling; a.o_rotation = io->out_rotation; a.o_normal = io->out_normal;
    a.o_opacity = io->out_opacity; a.o_base_color = io->out_base_color; a.o_roughness = io->out_roughness;
    a.o_metallic = io->out_metallic; a.o_viewdirs = io->out_viewdirs; a.o_symm_inv = io->out_symm_inv;
    if (a.o_scaling || a.o_rotation || a.o_normal || a.o_opacity || a.o_base_color || a.o_roughness || a.o_metallic ||
        a.o_viewdirs || a.o_symm_inv) {
        hipLaunchKernelGGL(act_fwd_kernel, dim3(ceil_div(ceil_div(P, kQuad), kThreads)), dim3(kThreads), 0, st, a);
        R3DG_CHECK_HIP(hipGetLastError());
    }

    ShArgs s{};
    s.P = P;
    const long long dc[3] = {r.f_dc, r.incidents_dc, r.visibility_dc};
    const long long rest[3] = {r.f_rest, r.incidents_rest, r.visibility_rest};
    float* outs[3] = {io->out_shs, io->out_incidents, io->out_visibility};
    unsigned total = 0;
    for (int i = 0; i < 3; ++i) {
        s.dc[i] = at(param, dc[i]); s.rest[i] = at(param, rest[i]); s.out[i] = outs[i];
        s.blocks[i] = outs[i] && s.dc[i] ? ceil_div(P, kShThreads / (i == 2 ? 4 : 12)) : 0;
        total += s.blocks[i];
    }
    if (total) {
        hipLaunchKernelGGL(sh_fwd_kernel, dim3(total), dim3(kShThreads), 0, st, s);
        R3DG_CHECK_HIP(hipGetLastError());
    }
    return R3DG_OK;
}

extern "C" int r3dg_activate_backward(const r3dg_activation_io* io, const float* param,
                                      const r3dg_activation_grads* grads, float* grad, int accumulate,
                                      r3dg_stream_t stream) {
    Resolved r;
    if (int e = resolve_roles(io, "activate_backward", &r)) return e;
    R3DG_REQUIRE(grads && grads->struct_size == sizeof(r3dg_activation_grads),
                 "activate_backward: r3dg_activation_grads.struct_size does not match this library");
    const int P = io->layout->P;
    const r3dg_grad_rows* ups[12] = {&grads->xyz, &grads->scaling, &grads->rotation, &grads->normal, &grads->opacity,
                                     &grads->shs, &grads->viewdirs, &grads->base_color, &grads->roughness,
                                     &grads->metallic, &grads->incidents, &grads->visibility};
    const int width[12] = {3, 3, 4, 3, 1, 48, 3, 3, 1, 1, 48, 16};
    for (int i = 0; i < 12; ++i) {
        R3DG_REQUIRE(!ups[i]->ptr || ups[i]->stride >= width[i],
                     "activate_backward: an upstream's row stride is below its row width");
        R3DG_REQUIRE(i < 7 || r.pbr || !ups[i]->ptr, "activate_backward: an upstream of an absent role");
    }
    R3DG_REQUIRE(!grads->viewdirs.ptr || io->campos, "activate_backward: the viewdirs upstream needs campos");
    if (P == 0) return R3DG_OK;
    R3DG_REQUIRE(param && grad, "activate_backward: null param or grad");
    hipStream_t st = (hipStream_t)stream;
    auto rows = [](const r3dg_grad_rows& g) { return GradRows{g.ptr, (long long)g.stride}; };

    ActArgs a{};
    a.P = P;
    a.accumulate = accumulate;
    raw_pointers(a, r, param);
    a.campos = io->campos;
    a.g_xyz = rows(grads->xyz); a.g_scaling = rows(grads->scaling); a.g_rotation = rows(grads->rotation);
    a.g_normal = rows(grads->normal); a.g_opacity = rows(grads->opacity); a.g_base_color = rows(grads->base_color);
    a.g_roughness = rows(grads->roughness); a.g_metallic = rows(grads->metallic); a.g_viewdirs = rows(grads->viewdirs);
    a.d_xyz = at(grad, r.xyz); a.d_scaling = at(grad, r.scaling); a.d_rotation = at(grad, r.rotation);
    a.d_normal = at(grad, r.normal); a.d_opacity = at(grad, r.opacity); a.d_base_color = at(grad, r.base_color);
    a.d_roughness = at(grad, r.roughness); a.d_metallic = at(grad, r.metallic);
    const bool any_small = a.g_xyz.ptr || a.g_scaling.ptr || a.g_rotation.ptr || a.g_normal.ptr || a.g_opacity.ptr ||
                           a.g_base_color.ptr || a.g_roughness.ptr || a.g_metallic.ptr || a.g_viewdirs.ptr;
    if (!accumulate || any_small) {
        hipLaunchKernelGGL(act_bwd_kernel, dim3(ceil_div(ceil_div(P, kQuad), kThreads)), dim3(kThreads), 0, st, a);
        R3DG_CHECK_HIP(hipGetLastError());
    }

    ShArgs s{};
    s.P = P;
    s.accumulate = accumulate;
    const long long dc[3] = {r.f_dc, r.incidents_dc, r.visibility_dc};
    const long long rest[3] = {r.f_rest, r.incidents_rest, r.visibility_rest};
    const r3dg_grad_rows* up[3] = {&grads->shs, &grads->incidents, &grads->visibility};
    unsigned total = 0;
    for (int i = 0; i < 3; ++i) {
        s.d_dc[i] = at(grad, dc[i]); s.d_rest[i] = at(grad, rest[i]); s.up[i] = rows(*up[i]);
        // accumulate mode adds nothing for a missing upstream; overwrite mode writes its zeros
        const bool run = s.d_dc[i] && (up[i]->ptr || !accumulate);
        s.blocks[i] = run ? ceil_div(P, kShThreads / (i == 2 ? 4 : 12)) : 0;
        total += s.blocks[i];
    }
    if (total) {
        hipLaunchKernelGGL(sh_bwd_kernel, dim3(total), dim3(kShThreads), 0, st, s);
        R3DG_CHECK_HIP(hipGetLastError());
    }
    return R3DG_OK;
}
