// relight.hip -- the relighting render equation (gfx950), forward only.
//
// Restates the reference's Python path, gaussian_renderer/neilf_composite.py:241-334
// (rendering_equation_python, is_training=False) with the pieces it calls: the unrotated Fibonacci
// hemisphere turned to the normal (utils/graphics_utils.py:9-37, utils/sh_utils.py:36-68), the SH
// basis up to degree 4 (utils/sh_utils.py:131-182) and the lat-long environment lookup
// (scene/envmap.py:31-48, nvdiffrast's dr.texture(filter_mode='linear'), boundary_mode='wrap').
// It is a different operator from brdf.hip, which restates the CUDA kernels: pi is np.pi rounded to
// float, not the literal 3.14159; the normalisations are F.normalize's (eps 1e-12); a normal with
// n_z + 1 <= 0 turns the samples by -I (sh_utils.py:66-67); the global light may come from an
// environment map and the visibility from per-sample traced values; and only [P, 21] leaves the
// operator: the integrated colour, the Gaussian's own attributes and four means over the samples,
// in the order the composite renderer concatenates its rasterizer features (:129-133).
//
// Layout, as brdf_fwd_lane_kernel: one lane per (Gaussian, sample). While Ns <= 256 a workgroup of
// 256 lanes holds GB = 256 / Ns whole Gaussians, lane t = (Gaussian t / Ns, sample t % Ns); beyond
// that a workgroup walks one Gaussian's samples in passes of 256. Either way the lanes of a pass
// read one contiguous span of the traced visibility ([P, Ns], the large stream). The 16 per-sample
// contributions go to an LDS row per lane and are summed per (Gaussian, channel) from there in sample
// order r = 0, 1, ... with Kahan's compensation, continuing across the passes (from Ns = 26 on, where
// a workgroup holds few Gaussians, as runs of consecutive samples whose sums are then added in
// order). The shape of the sum depends on Ns alone, so a Gaussian's result depends neither on P nor
// on its neighbours in the workgroup. No atomics. The [ng, 21] rows of a workgroup are one span.
#include "r3dg_common.h"
#include "r3dg_kernels.h"
#include "sh_dirs.h"  // relight_fib_dir, the degree-4 SH constants (shared with bvh.hip, visibility.hip)

namespace r3dg {

constexpr float kPiF = 3.14159265358979323846f;      // float(np.pi)
constexpr float kTwoPiF = 2.0f * kPiF;               // exact: the reference's 2 * np.pi in float
constexpr int kRelightMaxSH = 25;                    // degree 4
constexpr int kRelightCh = 16;                       // per-sample contributions summed per Gaussian
constexpr int kRelightCols = 21;                     // feature row

// eval_sh_coef(4, d) (utils/sh_utils.py:131-182), the expressions as written there
__device__ __forceinline__ void sh_coef25(float x, float y, float z, float* coef) {
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    coef[0] = SH_C0;
    coef[1] = -SH_C1 * y; coef[2] = SH_C1 * z; coef[3] = -SH_C1 * x;
    coef[4] = SH_C2_0 * xy; coef[5] = SH_C2_1 * yz; coef[6] = SH_C2_2 * (2.0f * zz - xx - yy);
    coef[7] = SH_C2_3 * xz; coef[8] = SH_C2_4 * (xx - yy);
    coef[9] = SH_C3_0 * y * (3.0f * xx - yy); coef[10] = SH_C3_1 * xy * z;
    coef[11] = SH_C3_2 * y * (4.0f * zz - xx - yy); coef[12] = SH_C3_3 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
    coef[13] = SH_C3_4 * x * (4.0f * zz - xx - yy); coef[14] = SH_C3_5 * z * (xx - yy);
    coef[15] = SH_C3_6 * x * (xx - 3.0f * yy);
    coef[16] = SH_C4_0 * xy * (xx - yy); coef[17] = SH_C4_1 * yz * (3.0f * xx - yy);
    coef[18] = SH_C4_2 * xy * (7.0f * zz - 1.0f); coef[19] = SH_C4_3 * yz * (7.0f * zz - 3.0f);
    coef[20] = SH_C4_4 * (zz * (35.0f * zz - 30.0f) + 3.0f); coef[21] = SH_C4_5 * xz * (7.0f * zz - 3.0f);
    coef[22] = SH_C4_6 * (xx - yy) * (7.0f * zz - 1.0f); coef[23] = SH_C4_7 * xz * (xx - 3.0f * yy);
    coef[24] = SH_C4_8 * (xx * (xx - 3.0f * yy) - yy * (3.0f * xx - yy));
}

// EnvLight.direct_light for one direction (scene/envmap.py:31-48): optional rotation, to_opengl,
// lat-long texture coordinates, then nvdiffrast's linear filter with wrap in both axes. Every texel
// index is in range for every input: the float that becomes an index goes through fminf(fmaxf(.))
// first, which maps NaN (and +-Inf) into [0, n], and the wrap is done on the integer after it.
__device__ __forceinline__ void wrap_texels(float u, int n, int& i0, int& i1, float& w) {
    u = u - floorf(u);                       // [0, 1]; 1 when u is a tiny negative
    const float x = u * (float)n - 0.5f;     // [-0.5, n - 0.5]
    const float xf = floorf(x);
    w = x - xf;
    // xf + 1 lies in [0, n] for a finite u; the clamps make that hold for NaN / Inf and for an n
    // that float cannot hold exactly
    const float s = fminf(fmaxf(xf + 1.0f, 0.0f), (float)n);
    const int i = min(max((int)s, 0), n);
    i0 = i == 0 ? n - 1 : i - 1;             // texel floor(x), modulo n
    i1 = i == n ? 0 : i;                     // texel floor(x) + 1, modulo n
}

__device__ __forceinline__ float3 env_lookup(const float* __restrict__ map, int H, int W,
                                             const float* __restrict__ T, float3 d) {
    if (T) {  // dirs @ transform.T
        const float tx = T[0] * d.x + T[1] * d.y + T[2] * d.z;
        const float ty = T[3] * d.x + T[4] * d.y + T[5] * d.z;
        const float tz = T[6] * d.x + T[7] * d.y + T[8] * d.z;
        d = make_float3(tx, ty, tz);
    }
    // v = (d.x, d.z, -d.y); tu = atan2(v.x, -v.z) / 2 pi + 0.5; tv = acos(clamp(v.y)) / pi
    const float tu = atan2f(d.x, d.y) / kTwoPiF + 0.5f;
    const float tv = acosf(fminf(fmaxf(d.z, -1.0f), 1.0f)) / kPiF;
    int x0, x1, y0, y1;
    float fx, fy;
    wrap_texels(tu, W, x0, x1, fx);
    wrap_texels(tv, H, y0, y1, fy);
    const float* p00 = map + ((size_t)y0 * W + x0) * 3;
    const float* p10 = map + ((size_t)y0 * W + x1) * 3;
    const float* p01 = map + ((size_t)y1 * W + x0) * 3;
    const float* p11 = map + ((size_t)y1 * W + x1) * 3;
    const float w00 = (1.0f - fx) * (1.0f - fy), w10 = fx * (1.0f - fy), w01 = (1.0f - fx) * fy, w11 = fx * fy;
    float o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = p00[c] * w00 + p10[c] * w10 + p01[c] * w01 + p11[c] * w11;
    return make_float3(o[0], o[1], o[2]);
}

struct RelightKArgs {
    r3dg_brdf_inputs in;
    const float* envmap;  // [He, We, 3]
    int env_h, env_w;
    const float* xform;   // [3, 3] or null
    const float* traced;  // [P, Ns]
    float* features;      // [P, 21]
};

enum { kLightNone = R3DG_LIGHT_NONE, kLightSH = R3DG_LIGHT_SH, kLightMap = R3DG_LIGHT_MAP };

// sum_i coef[i] * sh[stride * i + c] over the first S coefficients. N > 0: S = N at compile time
// (register or scalar-path coefficients); N = 0: a runtime S <= 25, the loop still unrolled so that
// coef[] stays in registers. The FMAs round once per term where the reference's tensor product and
// sum round twice; the order is the coefficients'.
template <int N, int C>
__device__ __forceinline__ void sh_dot(const float* coef, const float* __restrict__ sh, int S, float init, float* out) {
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = init;
#pragma unroll
    for (int i = 0; i < (N > 0 ? N : kRelightMaxSH); ++i) {
        if (N > 0 || i < S) {
#pragma unroll
            for (int c = 0; c < C; ++c) out[c] = __builtin_fmaf(sh[C * i + c], coef[i], out[c]);
        }
    }
}

// acc + sum of n floats at p[0], p[stride], ... in that order with Kahan's compensation (starting from
// cmp); the sum goes to *out, the new compensation is returned
__device__ __forceinline__ float kahan_add(const float* p, int stride, int n, float acc, float cmp, float* out) {
#pragma unroll 8
    for (int i = 0; i < n; ++i) {
        const float y = p[i * stride] - cmp;
        const float s = acc + y;
        cmp = (s - acc) - y;
        acc = s;
    }
    *out = acc;
    return cmp;
}

// LIGHT: the global light's mode; TRACED: per-sample visibility from the caller, else the baked SH;
// S16: every SH width the modes read is 16 (the incident coefficients in registers, compile-time
// loop bounds), else runtime widths 0..25 read from memory.
template <int LIGHT, bool TRACED, bool S16>
__global__ void __launch_bounds__(256) relight_kernel(RelightKArgs a, int GB) {
    constexpr int NC = kRelightCh;
    __shared__ float s_c[256 * (NC + 1)];
    __shared__ float s_sum[256][NC];
    __shared__ float s_cmp[256];   // the running sums' compensations over the passes (SEG > 1)
    __shared__ float s_part[256];  // run sums (SEG > 1)
    const r3dg_brdf_inputs& in = a.in;
    const int Ns = in.sample_num;
    const int t = threadIdx.x;
    const bool multi = Ns > 256;  // GB == 1: passes of 256 samples over one Gaussian
    const int gl = multi ? 0 : t / Ns, r0 = multi ? t : t - gl * Ns;
    const int g0 = blockIdx.x * GB;
    const int ng = min(GB, in.P - g0);
    const bool lane_g = gl < ng;
    const int idx = g0 + (lane_g ? gl : 0);  // a valid Gaussian for every lane
    for (int e = t; e < ng * NC; e += 256) s_sum[e / NC][e % NC] = 0.f;
    s_cmp[t] = 0.f;
    // lanes per (Gaussian, channel) in the per-Gaussian sums: a power of two, GB * NC * SEG <= 256
    const int q = 256 / (GB * NC);
    const int SEG = q >= 16 ? 16 : q >= 8 ? 8 : q >= 4 ? 4 : q >= 2 ? 2 : 1;
    const int seg_len = (min(Ns, 256) + SEG - 1) / SEG;

    // per-Gaussian terms (neilf_composite.py:284-306)
    const float3 n = make_float3(in.normals[3 * idx], in.normals[3 * idx + 1], in.normals[3 * idx + 2]);
    const float3 v = make_float3(in.viewdirs[3 * idx], in.viewdirs[3 * idx + 1], in.viewdirs[3 * idx + 2]);
    const float base[3] = {in.base_color[3 * idx], in.base_color[3 * idx + 1], in.base_color[3 * idx + 2]};
    const float rough = in.roughness[idx], metal = in.metallic[idx];
    float inc_r[S16 ? 48 : 1], vis_r[S16 && !TRACED ? 16 : 1];
    if constexpr (S16) {
#pragma unroll
        for (int i = 0; i < 48; ++i) inc_r[i] = in.incidents_shs[(size_t)idx * 48 + i];
        if constexpr (!TRACED) {
#pragma unroll
            for (int i = 0; i < 16; ++i) vis_r[i] = in.visibility_shs[(size_t)idx * 16 + i];
        }
    }
    const float* inc_g = in.incidents_shs + (size_t)idx * 3 * in.S_incident;
    const float* vis_g = TRACED ? nullptr : in.visibility_shs + (size_t)idx * in.S_visibility;
    const float r2 = fmaxf(rough * rough, 1e-7f);
    const float amp = 1.0f / (r2 * kPiF), sharp = 2.0f / r2;
    const float r2v = (1.0f + rough) * (1.0f + rough) / 8.0f;
    const float ndo = fmaxf(n.x * v.x + n.y * v.y + n.z * v.z, 0.0f);
    const float Vo = 0.5f / fmaxf(ndo * (1.0f - r2v) + r2v, 1e-7f);
    float fd[3], F0[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        fd[k] = (1.0f - metal) * base[k] / kPiF;
        F0[k] = 0.04f * (1.0f - metal) + base[k] * metal;
    }

    for (int p0 = 0; p0 < (multi ? Ns : 1); p0 += 256) {
        const int r = r0 + p0;
        const bool active = lane_g && r < Ns;
        float c[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) c[k] = 0.f;
        if (active) {
            const float3 d = relight_fib_dir(n, r, Ns);
            float coef[kRelightMaxSH];
            sh_coef25(d.x, d.y, d.z, coef);
            float local[3], glob[3] = {0.f, 0.f, 0.f}, vis;
            if constexpr (S16) sh_dot<16, 3>(coef, inc_r, 16, 0.f, local);
            else sh_dot<0, 3>(coef, inc_g, in.S_incident, 0.f, local);
            if constexpr (LIGHT == kLightSH) {
                if constexpr (S16) sh_dot<16, 3>(coef, in.direct_shs, 16, 0.5f, glob);
                else sh_dot<0, 3>(coef, in.direct_shs, in.S_direct, 0.5f, glob);
#pragma unroll
                for (int k = 0; k < 3; ++k) glob[k] = fmaxf(glob[k], 0.0f);
            } else if constexpr (LIGHT == kLightMap) {
                const float3 g = env_lookup(a.envmap, a.env_h, a.env_w, a.xform, d);  // unclamped (:265)
                glob[0] = g.x; glob[1] = g.y; glob[2] = g.z;
            }
            if constexpr (TRACED) {
                vis = a.traced[(size_t)idx * Ns + r];  // the workgroup's lanes: one contiguous span
            } else {
                if constexpr (S16) sh_dot<16, 1>(coef, vis_r, 16, 0.5f, &vis);
                else sh_dot<0, 1>(coef, vis_g, in.S_visibility, 0.5f, &vis);
                vis = fminf(fmaxf(vis, 0.0f), 1.0f);
            }
            // half vector and cosines (:311-317)
            const float hx = d.x + v.x, hy = d.y + v.y, hz = d.z + v.z;
            const float hn = fmaxf(sqrtf(hx * hx + hy * hy + hz * hz), 1e-12f);
            const float h0 = hx / hn, h1 = hy / hn, h2 = hz / hn;
            const float hdn = fmaxf(h0 * n.x + h1 * n.y + h2 * n.z, 0.0f);
            const float hdo = fmaxf(h0 * v.x + h1 * v.y + h2 * v.z, 0.0f);
            const float ndi = fmaxf(n.x * d.x + n.y * d.y + n.z * d.z, 0.0f);
            const float D = amp * r3dg_expf_wide(sharp * (hdn - 1.0f));
            const float t1 = 1.0f - hdo, t2 = t1 * t1, p5 = t2 * t2 * t1;
            const float V = (0.5f / fmaxf(ndi * (1.0f - r2v) + r2v, 1e-7f)) * Vo;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float lo = fmaxf(local[k], 0.0f);
                const float gv = glob[k] * vis;
                const float light = lo + gv;
                const float tr = light * kTwoPiF * ndi;
                const float F = F0[k] + (1.0f - F0[k]) * p5;
                c[k] = fd[k] * tr;
                c[3 + k] = D * F * V * tr;
                c[6 + k] = light;
                c[9 + k] = lo;
                c[12 + k] = gv;
            }
            c[15] = vis;
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) s_c[t * (NC + 1) + k] = c[k];
        __syncthreads();
        // per (Gaussian, channel): this pass's samples added in sample order to the running sum, with
        // Kahan's compensation: a plain float sum of 384 visibilities in sample order is off by up
        // to ~1e-6 of the mean, more than the reference's own (pairwise) tensor sum
        const int np = multi ? min(256, Ns - p0) : Ns;
        if (SEG == 1) {
            for (int e = t; e < ng * NC; e += 256) {
                const int gg = e / NC, k = e - gg * NC;
                kahan_add(s_c + gg * Ns * (NC + 1) + k, NC + 1, np, s_sum[gg][k], 0.f, &s_sum[gg][k]);
            }
        } else {
            // few Gaussians in the workgroup (Ns > 25): 16 lanes per Gaussian would walk all its samples
            // while 240 wait (measured at Ns = 384: 1.5 x the per-sample time of Ns = 24). SEG lanes per
            // (Gaussian, channel) each sum a run of seg_len samples in order, then one lane adds the
            // SEG run sums in order to the running sum. SEG and seg_len depend on Ns alone.
            const int e = t, gg = e / (NC * SEG), rem = e - gg * (NC * SEG), sg = rem / NC, k = rem - sg * NC;
            if (gg < ng) {
                const int lo = min(sg * seg_len, np), hi = min(lo + seg_len, np);
                kahan_add(s_c + ((multi ? 0 : gg * Ns) + lo) * (NC + 1) + k, NC + 1, hi - lo, 0.f, 0.f, &s_part[e]);
            }
            __syncthreads();
            if (t < ng * NC) {
                const int g2 = t / NC, k2 = t - g2 * NC;
                s_cmp[t] = kahan_add(s_part + g2 * (NC * SEG) + k2, NC, SEG, s_sum[g2][k2], s_cmp[t], &s_sum[g2][k2]);
            }
        }
        __syncthreads();
    }

    // [ng, 21] rows, one contiguous span (neilf_composite.py:129-133)
    const float fNs = (float)Ns;
    for (int e = t; e < ng * kRelightCols; e += 256) {
        const int gg = e / kRelightCols, col = e - gg * kRelightCols;
        const int gi = g0 + gg;
        const float* s = s_sum[gg];
        float o;
        if (col < 3) o = s[col] / fNs + s[3 + col] / fNs;  // rgb_d + rgb_s
        else if (col < 6) o = in.normals[3 * gi + col - 3];
        else if (col < 9) o = in.base_color[3 * gi + col - 6];
        else if (col == 9) o = in.roughness[gi];
        else if (col == 10) o = in.metallic[gi];
        else o = s[col - 5] / fNs;  // 11..20: light, local, global, visibility means
        a.features[(size_t)gi * kRelightCols + col] = o;
    }
}

__global__ void __launch_bounds__(256) envmap_light_kernel(int nd, const float* __restrict__ dirs,
                                                           const float* __restrict__ map, int H, int W,
                                                           const float* __restrict__ T, float* __restrict__ light) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nd) return;
    const float3 o = env_lookup(map, H, W, T, make_float3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
    light[3 * i] = o.x; light[3 * i + 1] = o.y; light[3 * i + 2] = o.z;
}

// The environment behind the object (neilf_composite.py:209-215) without the direction image of
// Camera.get_world_directions (scene/cameras.py:87-99): one lane per pixel forms its direction from the
// intrinsics K and the rotation rows of c2w, both read on the device, and looks the light up. MAP: env_lookup,
// the function envmap_light_kernel runs; else clamp_min(eval_sh + 0.5, 0) of shs [S, 3] with the basis and
// the fused sum of relight_kernel's kLightSH branch.
template <bool MAP>
__global__ void __launch_bounds__(256) env_background_kernel(int H, int W, const float* __restrict__ K,
                                                             const float* __restrict__ c2w, int stride,
                                                             const float* __restrict__ map, int eh, int ew,
                                                             const float* __restrict__ T,
                                                             const float* __restrict__ shs, int S,
                                                             float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * W) return;
    const int v = (int)(i / W), u = (int)(i - (size_t)v * W);
    const float fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    const float c[3] = {((float)u - cx) / fx, ((float)v - cy) / fy, 1.0f};
    const float nrm = fmaxf(sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]), 1e-12f);  // F.normalize
    const float d0 = c[0] / nrm, d1 = c[1] / nrm, d2 = c[2] / nrm;
    const float3 w = make_float3((c2w[0] * d0 + c2w[1] * d1) + c2w[2] * d2,
                                 (c2w[stride] * d0 + c2w[stride + 1] * d1) + c2w[stride + 2] * d2,
                                 (c2w[2 * stride] * d0 + c2w[2 * stride + 1] * d1) + c2w[2 * stride + 2] * d2);
    float o[3];
    if constexpr (MAP) {
        const float3 g = env_lookup(map, eh, ew, T, w);
        o[0] = g.x; o[1] = g.y; o[2] = g.z;
    } else {
        float coef[kRelightMaxSH];
        sh_coef25(w.x, w.y, w.z, coef);
        // the 0.5 is added last, as the reference writes it (eval_sh(...) + 0.5): started from 0.5, as the kLightSH
        // branch starts, every partial sum is larger and the 16 or 25 roundings with it (measured on one pixel at
        // degree 3: 2.4e-7 of the value against 1.7e-7)
        sh_dot<0, 3>(coef, shs, S, 0.0f, o);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = fmaxf(o[k] + 0.5f, 0.0f);
    }
    out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
}

template <int LIGHT, bool TRACED>
static hipError_t launch_relight2(const RelightKArgs& a, hipStream_t st) {
    const r3dg_brdf_inputs& in = a.in;
    const bool s16 = in.S_incident == 16 && (LIGHT != kLightSH || in.S_direct == 16) &&
                     (TRACED || in.S_visibility == 16);
    const int GB = in.sample_num <= 256 ? 256 / in.sample_num : 1;
    const dim3 grid((in.P + GB - 1) / GB), block(256);
    if (s16)
        hipLaunchKernelGGL((relight_kernel<LIGHT, TRACED, true>), grid, block, 0, st, a, GB);
    else
        hipLaunchKernelGGL((relight_kernel<LIGHT, TRACED, false>), grid, block, 0, st, a, GB);
    return hipGetLastError();
}

template <int LIGHT>
static hipError_t launch_relight(const RelightKArgs& a, hipStream_t st) {
    return a.traced ? launch_relight2<LIGHT, true>(a, st) : launch_relight2<LIGHT, false>(a, st);
}

}  // namespace r3dg

using namespace r3dg;

static int check_envmap(const float* envmap, int env_h, int env_w, const char* who) {
    R3DG_REQUIRE(envmap && env_h >= 1 && env_w >= 1,
                 std::string(who) + ": the environment map needs a pointer and env_h, env_w >= 1");
    return R3DG_OK;
}

extern "C" int r3dg_render_equation_relight(const r3dg_relight_inputs* in, float* features, r3dg_stream_t stream) {
    R3DG_REQUIRE(in && in->struct_size == sizeof(r3dg_relight_inputs),
                 "render_equation_relight: r3dg_relight_inputs.struct_size does not match this library");
    const r3dg_brdf_inputs& b = in->brdf;
    R3DG_REQUIRE(b.P >= 0, "render_equation_relight: invalid P");
    R3DG_REQUIRE(b.S_incident >= 0 && b.S_direct >= 0 && b.S_visibility >= 0 && b.S_incident <= kRelightMaxSH &&
                     b.S_direct <= kRelightMaxSH && b.S_visibility <= kRelightMaxSH,
                 "render_equation_relight: at most 25 SH coefficients (degree 4) are supported, as the reference's "
                 "eval_sh_coef (utils/sh_utils.py:131-182)");
    R3DG_REQUIRE(in->light_mode == R3DG_LIGHT_NONE || in->light_mode == R3DG_LIGHT_SH ||
                     in->light_mode == R3DG_LIGHT_MAP,
                 "render_equation_relight: light_mode must be R3DG_LIGHT_NONE, _SH or _MAP");
    if (in->light_mode == R3DG_LIGHT_MAP) {
        int rc = check_envmap(in->envmap, in->env_h, in->env_w, "render_equation_relight");
        if (rc) return rc;
    }
    R3DG_REQUIRE(b.P == 0 || b.sample_num >= 1, "render_equation_relight: sample_num must be at least 1");
    if (b.P == 0) return R3DG_OK;
    R3DG_REQUIRE(features && b.base_color && b.roughness && b.metallic && b.normals && b.viewdirs,
                 "render_equation_relight: features or a per-Gaussian input is NULL");
    R3DG_REQUIRE((b.S_incident == 0 || b.incidents_shs) &&
                     (in->light_mode != R3DG_LIGHT_SH || b.S_direct == 0 || b.direct_shs) &&
                     (in->traced_visibility || b.S_visibility == 0 || b.visibility_shs),
                 "render_equation_relight: an SH tensor that the modes read is NULL");
    RelightKArgs a{};
    a.in = b;
    a.envmap = in->envmap;
    a.env_h = in->env_h;
    a.env_w = in->env_w;
    a.xform = in->env_transform;
    a.traced = in->traced_visibility;
    a.features = features;
    hipStream_t st = (hipStream_t)stream;
    if (in->light_mode == R3DG_LIGHT_MAP) R3DG_CHECK_HIP(launch_relight<kLightMap>(a, st));
    else if (in->light_mode == R3DG_LIGHT_SH) R3DG_CHECK_HIP(launch_relight<kLightSH>(a, st));
    else R3DG_CHECK_HIP(launch_relight<kLightNone>(a, st));
    return R3DG_OK;
}

extern "C" int r3dg_envmap_direct_light(int n, const float* dirs, const float* envmap, int env_h, int env_w,
                                        const float* env_transform, float* light, r3dg_stream_t stream) {
    R3DG_REQUIRE(n >= 0, "envmap_direct_light: invalid n");
    int rc = check_envmap(envmap, env_h, env_w, "envmap_direct_light");
    if (rc) return rc;
    if (n == 0) return R3DG_OK;
    R3DG_REQUIRE(dirs && light, "envmap_direct_light: dirs or light is NULL");
    hipLaunchKernelGGL(envmap_light_kernel, dim3((unsigned)(((size_t)n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, dirs,
                       envmap,
                       env_h, env_w, env_transform, light);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}

extern "C" int r3dg_env_background(int H, int W, const float* intrinsics, const float* c2w, int c2w_stride,
                                   int light_mode, const float* envmap, int env_h, int env_w,
                                   const float* env_transform, const float* env_shs, int S, float* out,
                                   r3dg_stream_t stream) {
    R3DG_REQUIRE(H >= 1 && W >= 1, "env_background: H, W >= 1 expected");
    R3DG_REQUIRE((long long)H * W <= 0x7fffffffll, "env_background: H * W exceeds int32");
    R3DG_REQUIRE(intrinsics && c2w && out, "env_background: intrinsics, c2w or out is NULL");
    R3DG_REQUIRE(c2w_stride == 3 || c2w_stride == 4, "env_background: c2w_stride must be 3 or 4");
    R3DG_REQUIRE(light_mode == R3DG_LIGHT_SH || light_mode == R3DG_LIGHT_MAP,
                 "env_background: light_mode must be R3DG_LIGHT_SH or _MAP");
    const dim3 grid((unsigned)(((size_t)H * W + 255) / 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (light_mode == R3DG_LIGHT_MAP) {
        int rc = check_envmap(envmap, env_h, env_w, "env_background");
        if (rc) return rc;
        hipLaunchKernelGGL(env_background_kernel<true>, grid, block, 0, st, H, W, intrinsics, c2w, c2w_stride, envmap,
                           env_h, env_w, env_transform, env_shs, S, out);
    } else {
        R3DG_REQUIRE(env_shs && S >= 1 && S <= kRelightMaxSH,
                     "env_background: the environment SH needs a pointer and 1 to 25 coefficients (degree 4)");
        hipLaunchKernelGGL(env_background_kernel<false>, grid, block, 0, st, H, W, intrinsics, c2w, c2w_stride, envmap,
                           env_h, env_w, env_transform, env_shs, S, out);
    }
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}
