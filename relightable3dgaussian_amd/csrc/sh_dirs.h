// sh_dirs.h -- sample directions and the degree-4 SH basis shared by relight.hip, bvh.hip and
// visibility.hip. Every file that includes it is built with -ffp-contract=off (build.py): the
// expressions below round where the reference's float32 tensor code rounds.
#pragma once

#include "r3dg_common.h"

namespace r3dg {

constexpr int kMaxSH = 25;  // degree 4

// degree-4 constants (utils/sh_utils.py:23-33); degrees 0..3 are r3dg_common.h's
__device__ constexpr float SH_C4_0 = 2.5033429417967046f;
__device__ constexpr float SH_C4_1 = -1.7701307697799304f;
__device__ constexpr float SH_C4_2 = 0.9461746957575601f;
__device__ constexpr float SH_C4_3 = -0.6690465435572892f;
__device__ constexpr float SH_C4_4 = 0.10578554691520431f;
__device__ constexpr float SH_C4_5 = -0.6690465435572892f;
__device__ constexpr float SH_C4_6 = 0.47308734787878004f;
__device__ constexpr float SH_C4_7 = -1.7701307697799304f;
__device__ constexpr float SH_C4_8 = 0.6258357354491761f;

// fibonacci_sphere_sampling(normals, Ns, random_rotate=False) (utils/graphics_utils.py:9-37) for one
// sample. theta = float(delta) * ray is one rounded product, as the reference's tensor-by-scalar
// product, so the sample angle carries the reference's own rounding (6e-5 rad at ray 383).
__device__ __forceinline__ float3 relight_fib_dir(float3 n, int ray, int Ns) {
    const float delta = (float)(3.14159265358979323846 * (3.0 - 2.23606797749978969641));
    const float idx = (float)ray;
    const float z = 1.0f - 2.0f * idx / (float)(2 * Ns - 1);
    const float rad = sqrtf(1.0f - z * z);
    const float theta = delta * idx;
    float sn, cs;
    sincosf(theta, &sn, &cs);
    const float x = sn * rad, y = cs * rad;
    float ox, oy, oz;
    if (n.z + 1.0f > 0.0f) {  // rotation_between_z (utils/sh_utils.py:36-65), v3 = 0
        const float v1 = -n.y, v2 = n.x;
        const float cp1 = fmaxf(n.z + 1.0f, 1e-7f);
        const float q12 = v1 * v2 / cp1;
        ox = (1.0f + (-(v2 * v2)) / cp1) * x + q12 * y + v2 * z;
        oy = q12 * x + (1.0f + (-(v1 * v1)) / cp1) * y + (-v1) * z;
        oz = (-v2) * x + v1 * y + (1.0f + (-(v2 * v2) - v1 * v1) / cp1) * z;
    } else {  // -I (:66-67)
        ox = -x; oy = -y; oz = -z;
    }
    const float rn = fmaxf(sqrtf(ox * ox + oy * oy + oz * oz), 1e-12f);  // F.normalize
    return make_float3(ox / rn, oy / rn, oz / rn);
}

// The same sample evaluated in double and rounded once at the end: the Fibonacci direction itself, to float32
// accuracy, for the directions that leave the library (r3dg_fibonacci_dirs) and the rays traced along them
// (r3dg_bvh_trace_opacity_centres). relight_fib_dir above keeps the reference's float32 evaluation, which the
// render equation's float32 reference shares; its sample angle float(delta) * r alone is off by up to 3e-5 rad
// at r = 383, and for a normal within 1e-3 of -z the rotation's division by 1 + n_z turns that into 1e-3 of
// the direction. The branch is the same decision: n.z + 1 is exact in float32 wherever its sign is in doubt.
__device__ __forceinline__ float3 fib_dir(float3 n, int ray, int Ns) {
    const double delta = 3.14159265358979323846 * (3.0 - 2.23606797749978969641);
    const double idx = (double)ray;
    const double z = 1.0 - 2.0 * idx / (double)(2 * Ns - 1);
    const double rad = sqrt(1.0 - z * z);
    double sn, cs;
    sincos(delta * idx, &sn, &cs);
    const double x = sn * rad, y = cs * rad;
    const double nx = n.x, ny = n.y, nz = n.z;
    double ox, oy, oz;
    if (nz + 1.0 > 0.0) {  // rotation_between_z, v3 = 0
        const double v1 = -ny, v2 = nx;
        const double cp1 = fmax(nz + 1.0, 1e-7);
        const double q12 = v1 * v2 / cp1;
        ox = (1.0 - v2 * v2 / cp1) * x + q12 * y + v2 * z;
        oy = q12 * x + (1.0 - v1 * v1 / cp1) * y - v1 * z;
        oz = -v2 * x + v1 * y + (1.0 + (-(v2 * v2) - v1 * v1) / cp1) * z;
    } else {  // -I
        ox = -x; oy = -y; oz = -z;
    }
    const double rn = fmax(sqrt(ox * ox + oy * oy + oz * oz), 1e-12);  // F.normalize
    return make_float3((float)(ox / rn), (float)(oy / rn), (float)(oz / rn));
}

// The call sites' hemisphere flip (neilf.py:336-337, gaussian_model.py:447-448): the direction is negated
// when its float32 dot product with the normal, summed as (x + y) + z, is negative. A dot product of 0
// (or NaN) does not flip.
__device__ __forceinline__ float3 flip_to_normal(float3 d, float3 n) {
    const float dot = (d.x * n.x + d.y * n.y) + d.z * n.z;
    return dot < 0.0f ? make_float3(-d.x, -d.y, -d.z) : d;
}

// The factor of coefficient k in eval_sh(deg, sh, d) (utils/sh_utils.py:71-128), K = (deg + 1)^2 values,
// each product in the order the reference writes it: eval_sh is b[0] * sh[0] + b[1] * sh[1] + ... added
// in that order (its "- C1 * y * sh[1]" is the exact "+ (-(C1 * y)) * sh[1]").
__device__ __forceinline__ void eval_sh_basis(int K, float x, float y, float z, float* b) {
    b[0] = SH_C0;
    if (K <= 1) return;
    b[1] = -(SH_C1 * y); b[2] = SH_C1 * z; b[3] = -(SH_C1 * x);
    if (K <= 4) return;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    b[4] = SH_C2_0 * xy; b[5] = SH_C2_1 * yz; b[6] = SH_C2_2 * (2.0f * zz - xx - yy);
    b[7] = SH_C2_3 * xz; b[8] = SH_C2_4 * (xx - yy);
    if (K <= 9) return;
    b[9] = SH_C3_0 * y * (3.0f * xx - yy); b[10] = SH_C3_1 * xy * z;
    b[11] = SH_C3_2 * y * (4.0f * zz - xx - yy); b[12] = SH_C3_3 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
    b[13] = SH_C3_4 * x * (4.0f * zz - xx - yy); b[14] = SH_C3_5 * z * (xx - yy);
    b[15] = SH_C3_6 * x * (xx - 3.0f * yy);
    if (K <= 16) return;
    b[16] = SH_C4_0 * xy * (xx - yy); b[17] = SH_C4_1 * yz * (3.0f * xx - yy);
    b[18] = SH_C4_2 * xy * (7.0f * zz - 1.0f); b[19] = SH_C4_3 * yz * (7.0f * zz - 3.0f);
    b[20] = SH_C4_4 * (zz * (35.0f * zz - 30.0f) + 3.0f); b[21] = SH_C4_5 * xz * (7.0f * zz - 3.0f);
    b[22] = SH_C4_6 * (xx - yy) * (7.0f * zz - 1.0f); b[23] = SH_C4_7 * xz * (xx - 3.0f * yy);
    b[24] = SH_C4_8 * (xx * (xx - 3.0f * yy) - yy * (3.0f * xx - yy));
}

}  // namespace r3dg
