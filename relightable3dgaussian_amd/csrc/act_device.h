// act_device.h -- what activation.hip and compose.hip share: the 16-byte run accessors of the one-lane-per-
// four-Gaussians kernels, the activations' device functions (F.normalize, sigmoid, get_inverse_covariance)
// and the resolution of a flat parameter layout's roles. Both files are built with -ffp-contract=off and
// include these definitions as they stand, so an activation computed by either has the same bits.
#pragma once

#include <cmath>

#include "r3dg_common.h"

namespace r3dg {

constexpr int kQuad = 4;             // Gaussians per lane of the per-Gaussian kernels
constexpr float kEpsNormal = 1e-3f;  // gaussian_model.py:30
constexpr float kEpsUnit = 1e-12f;   // F.normalize's default (rotation :39, viewdirs neilf.py:102)

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// N = 4 w floats (four rows of width w) from p; only the first n exist (n < N in the tail lane)
template <int N>
__device__ __forceinline__ void load_run(const float* p, int n, float (&v)[N]) {
    if (n == N && aligned16(p)) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) {
            const float4 t = reinterpret_cast<const float4*>(p)[i];
            v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = i < n ? p[i] : 0.0f;
    }
}

template <int N>
__device__ __forceinline__ void store_run(float* p, int n, const float (&v)[N]) {
    if (n == N && aligned16(p)) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i)
            reinterpret_cast<float4*>(p)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (i < n) p[i] = v[i];
    }
}

__device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int W>
__device__ __forceinline__ float norm_of(const float* x) {
    float ss = x[0] * x[0];
#pragma unroll
    for (int c = 1; c < W; ++c) ss = ss + x[c] * x[c];
    return sqrtf(ss);
}

// F.normalize: x / max(|x|, eps)
template <int W>
__device__ __forceinline__ void normalize(const float* x, float eps, float* y) {
    const float d = fmaxf(norm_of<W>(x), eps);
#pragma unroll
    for (int c = 0; c < W; ++c) y[c] = x[c] / d;
}

// get_inverse_covariance (gaussian_model.py:410-413) of the activated rotation qh and scaling s:
// build_rotation normalises qh again (general_utils.py:82-103), L = R diag(1 / s), strip_symmetric(L L^T)
__device__ __forceinline__ void symm_inverse(const float* qh, const float* s, float* o) {
    const float n = norm_of<4>(qh);
    const float r = qh[0] / n, x = qh[1] / n, y = qh[2] / n, z = qh[3] / n;
    const float R[3][3] = {{1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - r * z), 2.0f * (x * z + r * y)},
                           {2.0f * (x * y + r * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - r * x)},
                           {2.0f * (x * z - r * y), 2.0f * (y * z + r * x), 1.0f - 2.0f * (x * x + y * y)}};
    float L[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float inv = 1.0f / s[k];
#pragma unroll
        for (int i = 0; i < 3; ++i) L[i][k] = R[i][k] * inv;
    }
    int e = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) o[e++] = (L[i][0] * L[j][0] + L[i][1] * L[j][1]) + L[i][2] * L[j][2];
}

// Host helpers; static, so every file that includes this header has its own copy.
// the float offset of every role's group in the flat buffer, -1 for an absent role
struct Resolved {
    long long xyz, scaling, rotation, opacity, normal, f_dc, f_rest, base_color, roughness, metallic, incidents_dc,
        incidents_rest, visibility_dc, visibility_rest;
    bool pbr;
};

static inline int resolve_roles(const r3dg_activation_io* io, const char* who, Resolved* out) {
    const std::string w(who);
    R3DG_REQUIRE(io && io->struct_size == sizeof(r3dg_activation_io),
                 w + ": r3dg_activation_io.struct_size does not match this library");
    const r3dg_param_layout* L = io->layout;
    R3DG_REQUIRE(L && L->P >= 0 && L->n_groups > 0 && L->n_groups <= R3DG_MAX_GROUPS, w + ": bad param layout");
    const int pbr[7] = {io->base_color, io->roughness, io->metallic, io->incidents_dc, io->incidents_rest,
                        io->visibility_dc, io->visibility_rest};
    int present = 0;
    for (int i = 0; i < 7; ++i) present += pbr[i] != -1;
    R3DG_REQUIRE(present == 0 || present == 7,
                 w + ": base_color, roughness, metallic and the incidents / visibility SH groups come together or not "
                     "at all");
    struct Role { int group, width; long long* off; };
    const Role roles[14] = {{L->xyz, 3, &out->xyz}, {L->scaling, 3, &out->scaling}, {L->rotation, 4, &out->rotation},
                            {L->opacity, 1, &out->opacity}, {io->normal, 3, &out->normal}, {io->f_dc, 3, &out->f_dc},
                            {io->f_rest, 45, &out->f_rest}, {pbr[0], 3, &out->base_color}, {pbr[1], 1, &out->roughness},
                            {pbr[2], 1, &out->metallic}, {pbr[3], 3, &out->incidents_dc},
                            {pbr[4], 45, &out->incidents_rest}, {pbr[5], 1, &out->visibility_dc},
                            {pbr[6], 15, &out->visibility_rest}};
    const int n_roles = present ? 14 : 7;
    R3DG_REQUIRE(L->n_groups == n_roles, w + ": every group of the layout must be named by exactly one role");
    long long start[R3DG_MAX_GROUPS], o = 0;
    for (int g = 0; g < L->n_groups; ++g) {
        start[g] = o;
        o += (long long)L->P * L->width[g];
    }
    unsigned seen = 0;
    for (int i = 0; i < 14; ++i) {
        if (i >= n_roles) { *roles[i].off = -1; continue; }
        const int g = roles[i].group;
        R3DG_REQUIRE(g >= 0 && g < L->n_groups && !((seen >> g) & 1u),
                     w + ": a role's group index is outside the layout or named twice");
        R3DG_REQUIRE(L->width[g] == roles[i].width, w + ": a role's group has the wrong width");
        seen |= 1u << g;
        *roles[i].off = start[g];
    }
    out->pbr = present != 0;
    return R3DG_OK;
}

static inline unsigned ceil_div(long long n, int d) { return (unsigned)((n + d - 1) / d); }

}  // namespace r3dg
