// compose.hip -- scene composition and the point-cloud capture of the relighting script (gfx950).
//
// Restates the reference's torch code around its relighting kernels:
//   * set_transform (scene/gaussian_model.py:237-262): an object's raw xyz, scaling, rotation and normal moved
//     by a 4x4 transform or by centre / rotation / scale / offset, with rotation_to_quaternion and
//     quaternion_multiply of utils/general_utils.py:105-149. There ~12 launches and as many temporaries;
//     here one launch in place on the flat parameter buffer (set_transform_kernel).
//   * scene_composition (relighting.py:31-55, create_from_gaussians gaussian_model.py:464-476) followed by the
//     getters: 14 torch.cat, the visibility_rest padding 15 -> 24, the zeroed incident SH, then ~20 activation
//     launches. Here two launches per object that read its flat buffer and write the ACTIVATED rows straight
//     into the composite at the object's row offset (compose_kernel, compose_sh_kernel); nothing of size P
//     exists in between and the object's buffer is read-only.
//   * render_points (relighting.py:89-123): a z-buffer written as `while True:` around two index_put and a
//     host synchronisation per pass. Here a 64-bit key per pixel (order-preserving depth bits : point index),
//     one global atomic min per candidate point and a resolve pass.
//
// The transform reaches the kernels as 19 floats on the device (r3dg_hip.h "scene composition"); the row
// norms, the rotation part and its quaternion are uniform over the launch and recomputed by every lane from
// scalar loads. The per-Gaussian kernels are laid out as activation.hip's (one lane per FOUR Gaussians, every
// [P, w] block in 16-byte runs where its address allows, dwords elsewhere: an output row block of the composite
// starts at any 4-byte-aligned address) and call its device functions (act_device.h), so an activation has
// the same bits from either file. Built with -ffp-contract=off: the float32 reference is torch tensor code
// that rounds every operation. No LDS, no host synchronisation; P = 0 launches nothing.
#include "act_device.h"

namespace r3dg {
namespace {

constexpr int kThreads = 256;
constexpr int kShThreads = 192;  // 16 rows of 12 float4 (48 floats), or 32 rows of 6 float4 (24 floats)

// what of the 19 floats applies (R3DG_XF_*)
struct Xform {
    int flags;
    float A[3][3];  // TRANSFORM: the linear part; ROTATION: the rotation
    float t[3];     // TRANSFORM: the translation; OFFSET: the offset
    float s[3];     // TRANSFORM: the row norms of A; SCALE: the scale
    float c[3];     // CENTER
    float R[3][3];  // what turns normals and (as q) rotations
    float q[4];
    bool turns;     // TRANSFORM or ROTATION
    bool scales;    // TRANSFORM or SCALE
};

// rotation_to_quaternion (general_utils.py:105-117)
__device__ __forceinline__ void rotation_to_quaternion(const float (&R)[3][3], float* q) {
    const float qw = sqrtf(fmaxf(((1.0f + R[0][0]) + R[1][1]) + R[2][2], 1e-7f)) / 2.0f;
    const float d = 4.0f * qw;
    const float v[4] = {qw, (R[2][1] - R[1][2]) / d, (R[0][2] - R[2][0]) / d, (R[1][0] - R[0][1]) / d};
    normalize<4>(v, kEpsUnit, q);
}

__device__ __forceinline__ Xform load_xform(const float* xf, int flags) {
    Xform x;
    x.flags = flags;
    x.turns = (flags & (R3DG_XF_TRANSFORM | R3DG_XF_ROTATION)) != 0;
    x.scales = (flags & (R3DG_XF_TRANSFORM | R3DG_XF_SCALE)) != 0;
    if (!flags) return x;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) x.A[i][j] = xf[4 * i + j];
        x.t[i] = xf[4 * i + 3];
        // a full transform reads M's first three rows only (its 16 floats may come without c)
        x.s[i] = (flags & R3DG_XF_SCALE) ? xf[12 + i] : 1.0f;
        x.c[i] = (flags & R3DG_XF_CENTER) ? xf[16 + i] : 0.0f;
    }
    if (flags & R3DG_XF_TRANSFORM) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            x.s[i] = norm_of<3>(x.A[i]);
#pragma unroll
            for (int j = 0; j < 3; ++j) x.R[i][j] = x.A[i][j] / x.s[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) x.R[i][j] = x.A[i][j];
    }
    if (x.turns) rotation_to_quaternion(x.R, x.q);
    return x;
}

// v @ M.T of one row (three products summed left to right)
__device__ __forceinline__ void mat_row(const float (&M)[3][3], const float* v, float* o) {
    const float a = v[0], b = v[1], c = v[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = (M[i][0] * a + M[i][1] * b) + M[i][2] * c;
}

__device__ __forceinline__ void move_xyz(const Xform& x, float* p) {
    if (x.flags & R3DG_XF_TRANSFORM) {
        float o[3];
        mat_row(x.A, p, o);
#pragma unroll
        for (int i = 0; i < 3; ++i) p[i] = o[i] + x.t[i];
        return;
    }
    if (x.flags & R3DG_XF_CENTER) {
#pragma unroll
        for (int i = 0; i < 3; ++i) p[i] = p[i] - x.c[i];
    }
    if (x.flags & R3DG_XF_ROTATION) {
        float o[3];
        mat_row(x.A, p, o);
#pragma unroll
        for (int i = 0; i < 3; ++i) p[i] = o[i];
    }
    if (x.flags & R3DG_XF_SCALE) {
#pragma unroll
        for (int i = 0; i < 3; ++i) p[i] = p[i] * x.s[i];
    }
    if (x.flags & R3DG_XF_OFFSET) {
#pragma unroll
        for (int i = 0; i < 3; ++i) p[i] = p[i] + x.t[i];
    }
}

__device__ __forceinline__ void turn_normal(const Xform& x, float* n) {
    if (!x.turns) return;
    float o[3];
    mat_row(x.R, n, o);
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = o[i];
}

// quaternion_multiply(q_T, q) (general_utils.py:139-149), left to right
__device__ __forceinline__ void turn_rotation(const Xform& x, float* q) {
    if (!x.turns) return;
    const float w1 = x.q[0], x1 = x.q[1], y1 = x.q[2], z1 = x.q[3];
    const float w2 = q[0], x2 = q[1], y2 = q[2], z2 = q[3];
    q[0] = ((w1 * w2 - x1 * x2) - y1 * y2) - z1 * z2;
    q[1] = ((w1 * x2 + x1 * w2) + y1 * z2) - z1 * y2;
    q[2] = ((w1 * y2 - x1 * z2) + y1 * w2) + z1 * x2;
    q[3] = ((w1 * z2 + x1 * y2) - y1 * x2) + z1 * w2;
}

// get_scaling * scale of one row
__device__ __forceinline__ void scaled_exp(const Xform& x, float* s) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float e = expf(s[i]);
        s[i] = x.scales ? e * x.s[i] : e;
    }
}

struct SetArgs {
    int P, flags;
    const float* xf;
    float *xyz, *scaling, *rotation, *normal;
};

__global__ void __launch_bounds__(kThreads) set_transform_kernel(SetArgs a) {
    const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kQuad;
    if (p0 >= a.P) return;
    const int rows = a.P - p0 < kQuad ? (int)(a.P - p0) : kQuad;
    const Xform x = load_xform(a.xf, a.flags);
    {
        float v[kQuad * 3];
        load_run(a.xyz + p0 * 3, rows * 3, v);
#pragma unroll
        for (int r = 0; r < kQuad; ++r) move_xyz(x, v + 3 * r);
        store_run(a.xyz + p0 * 3, rows * 3, v);
    }
    if (x.turns) {
        float n[kQuad * 3], q[kQuad * 4];
        load_run(a.normal + p0 * 3, rows * 3, n);
        load_run(a.rotation + p0 * 4, rows * 4, q);
#pragma unroll
        for (int r = 0; r < kQuad; ++r) {
            turn_normal(x, n + 3 * r);
            turn_rotation(x, q + 4 * r);
        }
        store_run(a.normal + p0 * 3, rows * 3, n);
        store_run(a.rotation + p0 * 4, rows * 4, q);
    }
    if (x.scales) {
        // scaling_inverse_activation(get_scaling * scale)
        float s[kQuad * 3];
        load_run(a.scaling + p0 * 3, rows * 3, s);
#pragma unroll
        for (int r = 0; r < kQuad; ++r) scaled_exp(x, s + 3 * r);
#pragma unroll
        for (int i = 0; i < kQuad * 3; ++i) s[i] = logf(s[i]);
        store_run(a.scaling + p0 * 3, rows * 3, s);
    }
}

// raw: group starts of the object's flat buffer; o_*: the composite's arrays at the object's first row
struct ComposeArgs {
    int P, flags;
    const float* xf;
    const float *xyz, *scaling, *rotation, *normal, *opacity, *base_color, *roughness, *metallic, *visibility_dc;
    float *o_xyz, *o_scaling, *o_rotation, *o_normal, *o_opacity, *o_base_color, *o_roughness, *o_metallic,
        *o_visibility_dc, *o_symm_inv;
};

template <int W>
__device__ __forceinline__ void sigmoid_rows(const float* raw, float* out, long long p0, int rows) {
    float v[kQuad * W];
    load_run(raw + p0 * W, rows * W, v);
#pragma unroll
    for (int i = 0; i < kQuad * W; ++i) v[i] = sigmoid(v[i]);
    store_run(out + p0 * W, rows * W, v);
}

__global__ void __launch_bounds__(kThreads) compose_kernel(ComposeArgs a) {
    const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kQuad;
    if (p0 >= a.P) return;
    const int rows = a.P - p0 < kQuad ? (int)(a.P - p0) : kQuad;
    const Xform x = load_xform(a.xf, a.flags);
    {
        float v[kQuad * 3];
        load_run(a.xyz + p0 * 3, rows * 3, v);
#pragma unroll
        for (int r = 0; r < kQuad; ++r) move_xyz(x, v + 3 * r);
        store_run(a.o_xyz + p0 * 3, rows * 3, v);
    }
    {
        float n[kQuad * 3], y[kQuad * 3];
        load_run(a.normal + p0 * 3, rows * 3, n);
#pragma unroll
        for (int r = 0; r < kQuad; ++r) {
            turn_normal(x, n + 3 * r);
            normalize<3>(n + 3 * r, kEpsNormal, y + 3 * r);
        }
        store_run(a.o_normal + p0 * 3, rows * 3, y);
    }
    {
        float q[kQuad * 4], s[kQuad * 3];
        load_run(a.rotation + p0 * 4, rows * 4, q);
        load_run(a.scaling + p0 * 3, rows * 3, s);
#pragma unroll
        for (int r = 0; r < kQuad; ++r) {
            float qh[4];
            turn_rotation(x, q + 4 * r);
            normalize<4>(q + 4 * r, kEpsUnit, qh);
#pragma unroll
            for (int c = 0; c < 4; ++c) q[4 * r + c] = qh[c];
            scaled_exp(x, s + 3 * r);
        }
        store_run(a.o_rotation + p0 * 4, rows * 4, q);
        store_run(a.o_scaling + p0 * 3, rows * 3, s);
        if (a.o_symm_inv) {
            float o[kQuad * 6];
#pragma unroll
            for (int r = 0; r < kQuad; ++r) symm_inverse(q + 4 * r, s + 3 * r, o + 6 * r);
            store_run(a.o_symm_inv + p0 * 6, rows * 6, o);
        }
    }
    sigmoid_rows<1>(a.opacity, a.o_opacity, p0, rows);
    sigmoid_rows<3>(a.base_color, a.o_base_color, p0, rows);
    sigmoid_rows<1>(a.roughness, a.o_roughness, p0, rows);
    sigmoid_rows<1>(a.metallic, a.o_metallic, p0, rows);
    {
        float v[kQuad];
        load_run(a.visibility_dc + p0, rows, v);
        store_run(a.o_visibility_dc + p0, rows, v);
    }
}

// ---- the wide rows: shs = cat(f_dc, f_rest), incidents = 0, visibility_rest padded 15 -> 24 --------------

struct ComposeShArgs {
    int P;
    const float *f_dc, *f_rest, *visibility_rest;
    float *o_shs, *o_incidents, *o_visibility_rest;
    unsigned blocks[2];  // workgroups of shs and of incidents; the others are visibility_rest's
};

// one lane per 16 B of an output row of ROW floats: WA floats of a's row, WB of b's, zeros behind
template <int WA, int WB, int ROW>
__device__ __forceinline__ void cat_rows(const float* a, const float* b, float* out, int P, unsigned block) {
    constexpr int Q = ROW / 4, ROWS = kShThreads / Q;
    static_assert(ROW % 4 == 0 && kShThreads % Q == 0, "whole rows of float4 per workgroup");
    const int r = (int)threadIdx.x / Q, k = (int)threadIdx.x - r * Q;
    const long long p = (long long)block * ROWS + r;
    if (p >= P) return;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = 4 * k + e;
        v[e] = c < WA ? a[p * WA + c] : c < WA + WB ? b[p * WB + (c - WA)] : 0.0f;
    }
    float* o = out + p * ROW + 4 * k;
    if (aligned16(o)) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[e];
    }
}

__global__ void __launch_bounds__(kShThreads) compose_sh_kernel(ComposeShArgs a) {
    unsigned b = blockIdx.x;
    if (b < a.blocks[0]) return cat_rows<3, 45, 48>(a.f_dc, a.f_rest, a.o_shs, a.P, b);
    b -= a.blocks[0];
    if (b < a.blocks[1]) return cat_rows<0, 0, 48>(nullptr, nullptr, a.o_incidents, a.P, b);
    b -= a.blocks[1];
    cat_rows<0, 15, 24>(nullptr, a.visibility_rest, a.o_visibility_rest, a.P, b);
}

// ---- the points capture -----------------------------------------------------------------------------

constexpr float kFarDepth = 10000.0f;          // relighting.py:113
constexpr unsigned long long kEmpty = ~0ull;   // what the clear writes: above every candidate's key

// unsigned order == float order (finite values; -0 sorts below +0)
__device__ __forceinline__ unsigned depth_bits(float z) {
    const unsigned u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bits_depth(unsigned b) {
    return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
}

struct PointsArgs {
    int P, H, W;
    const float *xyz, *color, *view, *K, *bg;  // bg NULL: bgv
    float bgv[3];
    unsigned long long* keys;
    float *rgb, *depth;
};

__global__ void __launch_bounds__(kThreads) points_scatter_kernel(PointsArgs a) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.P) return;
    const float x = a.xyz[3 * i], y = a.xyz[3 * i + 1], z = a.xyz[3 * i + 2];
    const float* V = a.view;  // [x, y, z, 1] @ V
    const float xc = ((x * V[0] + y * V[4]) + z * V[8]) + V[12];
    const float yc = ((x * V[1] + y * V[5]) + z * V[9]) + V[13];
    const float zc = ((x * V[2] + y * V[6]) + z * V[10]) + V[14];
    const float* K = a.K;     // xyz_cam @ K.T
    const float uh = (xc * K[0] + yc * K[1]) + zc * K[2];
    const float vh = (xc * K[3] + yc * K[4]) + zc * K[5];
    const float wh = (xc * K[6] + yc * K[7]) + zc * K[8];
    const float u = uh / wh, v = vh / wh;
    if (!isfinite(u) || !isfinite(v)) return;
    const float tu = truncf(u), tv = truncf(v);  // .long(): toward zero, so (-1, 0) lands in 0
    if (!(tu >= 0.0f && tu < (float)a.W && tv >= 0.0f && tv < (float)a.H && zc < kFarDepth)) return;
    const long long pix = (long long)(int)tv * a.W + (int)tu;
    const unsigned long long key = ((unsigned long long)depth_bits(zc) << 32) | (unsigned)i;
    // a plain load first: most points of a deep pixel already lose and skip the atomic
    if (key < a.keys[pix]) atomicMin(a.keys + pix, key);
}

__global__ void __launch_bounds__(kThreads) points_resolve_kernel(PointsArgs a) {
    const long long pix = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long HW = (long long)a.H * a.W;
    if (pix >= HW) return;
    const unsigned long long key = a.keys[pix];
    float c[3] = {a.bgv[0], a.bgv[1], a.bgv[2]}, d = kFarDepth;
    if (a.bg) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = a.bg[k];
    }
    if (key != kEmpty) {
        const long long i = (long long)(unsigned)key;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = a.color[3 * i + k];
        d = bits_depth((unsigned)(key >> 32));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) a.rgb[k * HW + pix] = c[k];
    if (a.depth) a.depth[pix] = d;
}

int check_flags(int flags, const float* xf, const std::string& w) {
    R3DG_REQUIRE((flags & ~(R3DG_XF_TRANSFORM | R3DG_XF_CENTER | R3DG_XF_ROTATION | R3DG_XF_SCALE | R3DG_XF_OFFSET)) == 0,
                 w + ": unknown transform flags");
    R3DG_REQUIRE(!(flags & R3DG_XF_TRANSFORM) || flags == R3DG_XF_TRANSFORM,
                 w + ": R3DG_XF_TRANSFORM excludes the other flags");
    R3DG_REQUIRE(!flags || xf, w + ": transform flags without the 19 floats");
    return R3DG_OK;
}

}  // namespace
}  // namespace r3dg

using namespace r3dg;

extern "C" int r3dg_set_transform(const r3dg_param_layout* L, int normal, float* param, const float* xform,
                                  int flags, r3dg_stream_t stream) {
    const std::string w("set_transform");
    R3DG_REQUIRE(L && L->P >= 0 && L->n_groups > 0 && L->n_groups <= R3DG_MAX_GROUPS, w + ": bad param layout");
    if (int e = check_flags(flags, xform, w)) return e;
    const int role[4] = {L->xyz, L->scaling, L->rotation, normal}, width[4] = {3, 3, 4, 3};
    long long start[R3DG_MAX_GROUPS], o = 0;
    for (int g = 0; g < L->n_groups; ++g) {
        start[g] = o;
        o += (long long)L->P * L->width[g];
    }
    for (int i = 0; i < 4; ++i) {
        R3DG_REQUIRE(role[i] >= 0 && role[i] < L->n_groups && L->width[role[i]] == width[i],
                     w + ": xyz, scaling, rotation and normal must name groups of width 3, 3, 4, 3");
        for (int j = 0; j < i; ++j) R3DG_REQUIRE(role[i] != role[j], w + ": a group is named twice");
    }
    if (L->P == 0 || !flags) return R3DG_OK;
    R3DG_REQUIRE(param, w + ": null param");
    SetArgs a{};
    a.P = L->P; a.flags = flags; a.xf = xform;
    a.xyz = param + start[role[0]]; a.scaling = param + start[role[1]]; a.rotation = param + start[role[2]];
    a.normal = param + start[role[3]];
    hipLaunchKernelGGL(set_transform_kernel, dim3(ceil_div(ceil_div(L->P, kQuad), kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, a);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}

extern "C" int r3dg_compose_object(const r3dg_activation_io* io, const float* param, const float* xform, int flags,
                                   const r3dg_compose_out* out, int64_t row, r3dg_stream_t stream) {
    const std::string w("compose_object");
    Resolved r;
    if (int e = resolve_roles(io, "compose_object", &r)) return e;
    R3DG_REQUIRE(r.pbr, w + ": the object needs all 14 groups");
    if (int e = check_flags(flags, xform, w)) return e;
    R3DG_REQUIRE(out && out->struct_size == sizeof(r3dg_compose_out),
                 w + ": r3dg_compose_out.struct_size does not match this library");
    R3DG_REQUIRE(row >= 0, w + ": negative row offset");
    R3DG_REQUIRE(out->xyz && out->scaling && out->rotation && out->normal && out->opacity && out->base_color &&
                     out->roughness && out->metallic && out->shs && out->incidents && out->visibility_dc &&
                     out->visibility_rest,
                 w + ": only symm_inv may be NULL");
    const int P = io->layout->P;
    R3DG_REQUIRE(P == 0 || param, w + ": null param");
    if (P == 0) return R3DG_OK;
    hipStream_t st = (hipStream_t)stream;

    ComposeArgs a{};
    a.P = P; a.flags = flags; a.xf = xform;
    a.xyz = param + r.xyz; a.scaling = param + r.scaling; a.rotation = param + r.rotation;
    a.normal = param + r.normal; a.opacity = param + r.opacity; a.base_color = param + r.base_color;
    a.roughness = param + r.roughness; a.metallic = param + r.metallic; a.visibility_dc = param + r.visibility_dc;
    a.o_xyz = out->xyz + row * 3; a.o_scaling = out->scaling + row * 3; a.o_rotation = out->rotation + row * 4;
    a.o_normal = out->normal + row * 3; a.o_opacity = out->opacity + row; a.o_base_color = out->base_color + row * 3;
    a.o_roughness = out->roughness + row; a.o_metallic = out->metallic + row;
    a.o_visibility_dc = out->visibility_dc + row;
    a.o_symm_inv = out->symm_inv ? out->symm_inv + row * 6 : nullptr;
    hipLaunchKernelGGL(compose_kernel, dim3(ceil_div(ceil_div(P, kQuad), kThreads)), dim3(kThreads), 0, st, a);
    R3DG_CHECK_HIP(hipGetLastError());

    ComposeShArgs s{};
    s.P = P;
    s.f_dc = param + r.f_dc; s.f_rest = param + r.f_rest; s.visibility_rest = param + r.visibility_rest;
    s.o_shs = out->shs + row * 48; s.o_incidents = out->incidents + row * 48;
    s.o_visibility_rest = out->visibility_rest + row * 24;
    s.blocks[0] = s.blocks[1] = ceil_div(P, kShThreads / 12);
    hipLaunchKernelGGL(compose_sh_kernel, dim3(2 * s.blocks[0] + ceil_div(P, kShThreads / 6)), dim3(kShThreads), 0, st,
                       s);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}

extern "C" int r3dg_render_points(int P, const float* xyz, const float* color, const float* world_view,
                                  const float* intrinsics, int H, int W, const float* bg, const float* bg_value,
                                  float* out_rgb, float* out_depth, r3dg_alloc_fn scratch_alloc,
                                  void* scratch_ctx, r3dg_stream_t stream) {
    const std::string w("render_points");
    R3DG_REQUIRE(P >= 0 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL, w + ": bad P, H or W");
    R3DG_REQUIRE(world_view && intrinsics && (bg || bg_value) && out_rgb && scratch_alloc, w + ": null argument");
    R3DG_REQUIRE(P == 0 || (xyz && color), w + ": null xyz or color");
    hipStream_t st = (hipStream_t)stream;
    const long long HW = (long long)H * W;
    PointsArgs a{};
    a.P = P; a.H = H; a.W = W;
    a.xyz = xyz; a.color = color; a.view = world_view; a.K = intrinsics; a.bg = bg;
    for (int k = 0; k < 3; ++k) a.bgv[k] = bg ? 0.0f : bg_value[k];
    a.rgb = out_rgb; a.depth = out_depth;
    a.keys = static_cast<unsigned long long*>(scratch_alloc(scratch_ctx, (size_t)HW * sizeof(unsigned long long)));
    R3DG_REQUIRE(a.keys, w + ": the scratch allocation failed");
    R3DG_CHECK_HIP(hipMemsetAsync(a.keys, 0xff, (size_t)HW * sizeof(unsigned long long), st));
    if (P > 0) {
        hipLaunchKernelGGL(points_scatter_kernel, dim3(ceil_div(P, kThreads)), dim3(kThreads), 0, st, a);
        R3DG_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(points_resolve_kernel, dim3(ceil_div(HW, kThreads)), dim3(kThreads), 0, st, a);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}
