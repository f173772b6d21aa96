// knn.hip -- mean squared distance to the three nearest neighbours (the reference's
// simple_knn._C.distCUDA2: submodules/simple-knn/spatial.cu:15-26, simple_knn.cu:131-221), which
// GaussianModel.create_from_pcd turns into the initial scales (scene/gaussian_model.py:537-580).
//
// out[i] = ((b0 + b1) + b2) / 3 with b0 <= b1 <= b2 the three smallest d2(i, j), j != i (by index: a
// duplicate at distance 0 counts), d2 = (dx dx + dy dy) + dz dz, d = p_j - p_i; a missing neighbour is
// FLT_MAX (the reference's initial value). The search is exact: boxes are skipped only on a lower bound
// of d2, so the result depends on neither the sort, the box size nor the visiting order. This file is
// compiled with -ffp-contract=off (build.py): the arithmetic above is what a numpy-f32 brute force does.
//
// MI355X design (not a translation: the reference runs one thread per point that walks every box
// serially and gathers candidates through indices[], which diverges on wave64):
//   * 5 launches + one rocPRIM radix sort on the caller's stream, no host round trip: partial bounds ->
//     final bounds + 30-bit Morton codes -> stable radix sort of (code, index) -> gather into a
//     Morton-ordered float4 array + one AABB per box of kKnnBox consecutive points -> one AABB per
//     super-box of kKnnBatch boxes -> search.
//   * search: one wave (= one workgroup) per box of 64 points, one lane per query, queries in Morton
//     order, so the vote across the workgroup is one ballot and nothing waits on another wave. The
//     lane's reject radius comes from its +-3 sorted neighbours (as the reference). The wave scans its
//     own box first (best[2] is tight before any vote), then walks the super-boxes outward from its
//     own. Per super-box it votes on the super-box's bound; if some lane can use it, the 64 lanes load
//     one box each and every lane tests all 64 (wave-uniform lane reads), a vote per box on
//     dist <= min(reject, best[2]) giving a 64-bit mask. A box some lane can still use when its turn
//     comes (best[2] tightens meanwhile) is staged in LDS as float4 and scanned by all lanes at the same
//     address (a broadcast: no bank conflicts). (Measured against 256-point boxes with four waves per
//     workgroup, and against one flat list of all boxes: DESIGN.md §2f.)
//   * every loop is bounded by P or the box count, never by data: non-finite input gives unspecified
//     values, but terminates and stays in bounds.
#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <cstring>  // rocprim's headers call memset

#include "r3dg_common.h"

#include <rocprim/rocprim.hpp>

namespace r3dg {
namespace {

constexpr int kKnnBox = 64;   // points per box = queries per wave; the search runs one wave per box
constexpr int kKnnBatch = 64; // boxes per super-box, voted on in one round (a lane and a mask bit each)

struct Bounds {
    float lx, ly, lz, ux, uy, uz;
};
__device__ __forceinline__ Bounds empty_bounds() { return Bounds{FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX}; }
__device__ __forceinline__ Bounds merge(const Bounds& a, const Bounds& b) {
    return Bounds{fminf(a.lx, b.lx), fminf(a.ly, b.ly), fminf(a.lz, b.lz),
                  fmaxf(a.ux, b.ux), fmaxf(a.uy, b.uy), fmaxf(a.uz, b.uz)};
}
__device__ __forceinline__ Bounds bounds_of(float x, float y, float z) { return Bounds{x, y, z, x, y, z}; }

// the merge of a workgroup's 256 bounds, valid in every thread
__device__ __forceinline__ Bounds block_merge(Bounds acc, Bounds* sb) {
    sb[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sb[threadIdx.x] = merge(sb[threadIdx.x], sb[threadIdx.x + s]);
        __syncthreads();
    }
    return sb[0];
}

// scene bounds (simple_knn.cu:193-200, two device reductions and two blocking copies there): per-block partials
__global__ void __launch_bounds__(256) knn_bounds_partial_kernel(int P, const float* __restrict__ points,
                                                                 Bounds* __restrict__ partial) {
    __shared__ Bounds sb[256];
    Bounds acc = empty_bounds();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (long long)gridDim.x * blockDim.x)
        acc = merge(acc, bounds_of(points[3 * i], points[3 * i + 1], points[3 * i + 2]));
    acc = block_merge(acc, sb);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {  // 10 bits -> every third bit
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

// one axis of coord2Morton (simple_knn.cu:54-61): 10 bits of (v - lo) / (hi - lo). A degenerate axis
// (hi == lo: 0 / 0 in the reference) and any non-finite quotient map to 0; the order only steers the
// search, never its result.
__device__ __forceinline__ uint32_t morton_axis(float v, float lo, float hi) {
    const float ext = hi - lo;
    const float t = ext > 0.0f ? (v - lo) / ext * 1023.0f : 0.0f;
    return (uint32_t)fminf(fmaxf(t, 0.0f), 1023.0f);  // fmaxf(NaN, 0) = 0
}

__global__ void __launch_bounds__(256) knn_morton_kernel(int P, int n_partial, const Bounds* __restrict__ partial,
                                                         const float* __restrict__ points, uint32_t* __restrict__ code,
                                                         uint32_t* __restrict__ index) {
    __shared__ Bounds sb[256];  // n_partial <= 256 partial bounds, reduced by every block
    const Bounds w = block_merge((int)threadIdx.x < n_partial ? partial[threadIdx.x] : empty_bounds(), sb);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    code[i] = expand_bits(morton_axis(x, w.lx, w.ux)) | (expand_bits(morton_axis(y, w.ly, w.uy)) << 1) |
              (expand_bits(morton_axis(z, w.lz, w.uz)) << 2);
    index[i] = (uint32_t)i;
}

// the merge of a wave's 64 boxes, valid in every lane
__device__ __forceinline__ void wave_merge(float4& lo, float4& hi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo.x = fminf(lo.x, __shfl_xor(lo.x, o));
        lo.y = fminf(lo.y, __shfl_xor(lo.y, o));
        lo.z = fminf(lo.z, __shfl_xor(lo.z, o));
        hi.x = fmaxf(hi.x, __shfl_xor(hi.x, o));
        hi.y = fmaxf(hi.y, __shfl_xor(hi.y, o));
        hi.z = fmaxf(hi.z, __shfl_xor(hi.z, o));
    }
}
__device__ __forceinline__ float4 empty_lo() { return make_float4(FLT_MAX, FLT_MAX, FLT_MAX, 0.0f); }
__device__ __forceinline__ float4 empty_hi() { return make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, 0.0f); }

// after the sort: the points in Morton order as float4 (w unused) and each box's AABB (lower, upper as
// float4 pairs; simple_knn.cu:78-117 boxMinMax). One wave per box.
__global__ void __launch_bounds__(256) knn_gather_kernel(int P, const float* __restrict__ points,
                                                         const uint32_t* __restrict__ index,
                                                         float4* __restrict__ sorted, float4* __restrict__ boxes) {
    static_assert(kKnnBox == 64, "one wave per box");
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float4 lo = empty_lo(), hi = empty_hi();
    if (i < P) {
        const size_t s = index[i];  // a permutation of [0, P): written by knn_morton_kernel, moved by the sort
        lo = hi = make_float4(points[3 * s], points[3 * s + 1], points[3 * s + 2], 0.0f);
        sorted[i] = lo;
    }
    wave_merge(lo, hi);
    const long long first = i & ~63ll;  // the wave's first point: its box exists if that point does
    if ((threadIdx.x & 63) == 0 && first < P) {
        boxes[2 * (size_t)(first / kKnnBox)] = lo;
        boxes[2 * (size_t)(first / kKnnBox) + 1] = hi;
    }
}

// The k-th box (k in [0, nb)) of the outward walk from box b: b, b+1, b-1, b+2, b-2, ... while both
// sides last, then the longer side alone. A bijection of [0, nb) onto [0, nb).
__device__ __forceinline__ int knn_visit_box(int b, int nb, int k) {
    const int left = b, right = nb - 1 - b, m = left < right ? left : right;
    if (k <= 2 * m) return (k & 1) ? b + (k + 1) / 2 : b - k / 2;
    return right > left ? b + (k - m) : b - (k - m);
}

// distBoxPoint (simple_knn.cu:119-129): per axis the distance to the nearer face when outside,
// max(lo - p, p - hi, 0). Every operation is monotone and d2 associates the same way, so it is a lower
// bound, in f32, of d2 to any point inside the box.
__device__ __forceinline__ float box_dist2(float4 lo, float4 hi, float4 p) {
    const float dx = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.0f);
    const float dy = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.0f);
    const float dz = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.0f);
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ float dist2(float4 c, float4 q) {
    const float dx = c.x - q.x, dy = c.y - q.y, dz = c.z - q.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// updateKBest<3> (simple_knn.cu:131-145): insert d into the ascending triple
__device__ __forceinline__ void insert3(float d, float& b0, float& b1, float& b2) {
    const float t0 = fmaxf(b0, d);
    b0 = fminf(b0, d);
    const float t1 = fmaxf(b1, t0);
    b1 = fminf(b1, t0);
    b2 = fminf(b2, t1);
}

// all lanes read the staged box at the same address; `self` < 0 when the lane's own point is not in it
template <bool SELF>
__device__ __forceinline__ void scan_box(const float4* s_pts, int count, int self, float4 q, float& b0, float& b1,
                                         float& b2) {
#pragma unroll 4
    for (int j = 0; j < count; ++j) {
        float d = dist2(s_pts[j], q);
        if (SELF && j == self) d = FLT_MAX;  // `if (i == idx) continue`: inserting the initial value changes nothing
        insert3(d, b0, b1, b2);
    }
}

// one AABB per super-box of kKnnBatch consecutive boxes. One wave per super-box.
__global__ void __launch_bounds__(64) knn_super_kernel(int nb, const float4* __restrict__ boxes,
                                                       float4* __restrict__ supers) {
    const int c = blockIdx.x * kKnnBatch + threadIdx.x;
    float4 lo = empty_lo(), hi = empty_hi();
    if (c < nb) {
        lo = boxes[2 * (size_t)c];
        hi = boxes[2 * (size_t)c + 1];
    }
    wave_merge(lo, hi);
    if (threadIdx.x == 0) {
        supers[2 * (size_t)blockIdx.x] = lo;
        supers[2 * (size_t)blockIdx.x + 1] = hi;
    }
}

__device__ __forceinline__ float lane_value(float v, int lane) {  // v of lane `lane` (wave-uniform), in every lane
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// One wave (= one workgroup) per box, one lane per query.
__global__ void __launch_bounds__(kKnnBox) knn_search_kernel(int P, int nb, int ns, const float4* __restrict__ sorted,
                                                             const float4* __restrict__ boxes,
                                                             const float4* __restrict__ supers,
                                                             const uint32_t* __restrict__ index,
                                                             float* __restrict__ out) {
    static_assert(kKnnBox == 64 && kKnnBatch == 64, "a lane per point of a box and per box of a super-box");
    __shared__ float4 s_pts[kKnnBox];
    const int own = blockIdx.x, lane = threadIdx.x;
    const long long i = (long long)own * kKnnBox + lane;
    const bool valid = i < P;
    const float4 q = valid ? sorted[i] : make_float4(0.f, 0.f, 0.f, 0.f);

    // reject radius: the third-best of the six neighbours in sorted order (simple_knn.cu:156-163)
    float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;
    if (valid) {
#pragma unroll
        for (int o = -3; o <= 3; ++o) {
            const long long j = i + o;
            if (o != 0 && j >= 0 && j < P) insert3(dist2(sorted[j], q), b0, b1, b2);
        }
    }
    const float reject = b2;
    b0 = b1 = b2 = FLT_MAX;

    // box c (wave-uniform) into LDS; returns its point count
    auto stage = [&](int c) {
        const long long base = (long long)c * kKnnBox;
        const int count = (int)min((long long)kKnnBox, (long long)P - base);
        __syncthreads();  // the previous box's scan is done
        if (lane < count) s_pts[lane] = sorted[base + lane];
        __syncthreads();
        return count;
    };

    // the wave's own box first: it holds most of the neighbours, so best[2] is tight before any vote
    scan_box<true>(s_pts, stage(own), lane, q, b0, b1, b2);

    // then the super-boxes outward from the wave's own
    const int own_s = own / kKnnBatch;
    for (int ks = 0; ks < ns; ++ks) {
        const int g = knn_visit_box(own_s, ns, ks);
        const float thr = fminf(reject, b2);
        const bool use_super = valid && !(box_dist2(supers[2 * (size_t)g], supers[2 * (size_t)g + 1], q) > thr);
        if (__ballot(use_super) == 0ull) continue;
        // lane l loads box c0 + l; every lane then tests all of them, one wave-uniform lane read each
        const int c0 = g * kKnnBatch, n = min(kKnnBatch, nb - c0);
        float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
        if (lane < n) {
            lo = boxes[2 * (size_t)(c0 + lane)];
            hi = boxes[2 * (size_t)(c0 + lane) + 1];
        }
        auto box_k = [&](int k, float bound) {  // can this lane use box c0 + k?
            const float4 klo = make_float4(lane_value(lo.x, k), lane_value(lo.y, k), lane_value(lo.z, k), 0.f);
            const float4 khi = make_float4(lane_value(hi.x, k), lane_value(hi.y, k), lane_value(hi.z, k), 0.f);
            return valid && !(box_dist2(klo, khi, q) > bound);
        };
        unsigned long long m = 0;  // bit k: some lane can use box c0 + k
#pragma unroll 8
        for (int k = 0; k < kKnnBatch; ++k)
            if (__ballot(box_k(k, thr)) != 0ull) m |= 1ull << k;
        if (n < kKnnBatch) m &= (1ull << n) - 1ull;      // only boxes that exist
        if (g == own_s) m &= ~(1ull << (own - c0));      // the own box is done
        while (m != 0ull) {  // at most 64 rounds: one bit leaves per round
            const int k = __builtin_ctzll(m);
            m &= m - 1ull;
            // best[2] has tightened since the vote: skip a box no lane needs any more
            if (__ballot(box_k(k, fminf(reject, b2))) == 0ull) continue;
            scan_box<false>(s_pts, stage(c0 + k), -1, q, b0, b1, b2);
        }
    }
    if (valid) out[index[i]] = ((b0 + b1) + b2) / 3.0f;
}

inline unsigned blocks(long long n) { return (unsigned)((n + 255) / 256); }
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace
}  // namespace r3dg

using namespace r3dg;

extern "C" int r3dg_knn_mean_dist2(int P, const float* points, float* mean_dist2, r3dg_alloc_fn scratch_alloc,
                                   void* scratch_ctx, r3dg_stream_t stream) {
    R3DG_REQUIRE(P >= 0, "knn_mean_dist2: negative point count");
    if (P == 0) return R3DG_OK;
    R3DG_REQUIRE(points && mean_dist2, "knn_mean_dist2: null points / mean_dist2");
    R3DG_REQUIRE(scratch_alloc, "knn_mean_dist2: null scratch_alloc");
    R3DG_REQUIRE(P < (1 << 30), "knn_mean_dist2: too many points");
    hipStream_t st = (hipStream_t)stream;
    const int n_partial = (int)std::min<long long>(256, blocks(P));
    const int nb = (P + kKnnBox - 1) / kKnnBox, ns = (nb + kKnnBatch - 1) / kKnnBatch;
    size_t sort_bytes = 0;
    R3DG_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)P, 0, 30, st));
    const size_t b_partial = align256(sizeof(Bounds) * (size_t)n_partial), b_u32 = align256(4 * (size_t)P),
                 b_sorted = align256(16 * (size_t)P), b_boxes = align256(32 * (size_t)nb),
                 b_supers = align256(32 * (size_t)ns);
    char* s = (char*)scratch_alloc(scratch_ctx, b_partial + 4 * b_u32 + b_sorted + b_boxes + b_supers +
                                                    align256(sort_bytes) + 256);
    if (!s) {
        set_error("knn_mean_dist2: scratch allocation failed");
        return R3DG_ERR_ALLOC;
    }
    s = (char*)(((uintptr_t)s + 255) & ~(uintptr_t)255);
    Bounds* partial = (Bounds*)s; s += b_partial;
    uint32_t* code = (uint32_t*)s; s += b_u32;
    uint32_t* index = (uint32_t*)s; s += b_u32;
    uint32_t* code_s = (uint32_t*)s; s += b_u32;
    uint32_t* index_s = (uint32_t*)s; s += b_u32;
    float4* sorted = (float4*)s; s += b_sorted;
    float4* boxes = (float4*)s; s += b_boxes;
    float4* supers = (float4*)s; s += b_supers;
    void* tmp = s;
    hipLaunchKernelGGL(knn_bounds_partial_kernel, dim3(n_partial), dim3(256), 0, st, P, points, partial);
    R3DG_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(knn_morton_kernel, dim3(blocks(P)), dim3(256), 0, st, P, n_partial, partial, points, code, index);
    R3DG_CHECK_HIP(hipGetLastError());
    // stable (LSD radix): equal codes keep their input order, so the order is a function of the input alone
    R3DG_CHECK_HIP(rocprim::radix_sort_pairs(tmp, sort_bytes, code, code_s, index, index_s, (size_t)P, 0, 30, st));
    hipLaunchKernelGGL(knn_gather_kernel, dim3(blocks(P)), dim3(256), 0, st, P, points, index_s, sorted, boxes);
    R3DG_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(knn_super_kernel, dim3(ns), dim3(64), 0, st, nb, boxes, supers);
    R3DG_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(knn_search_kernel, dim3(nb), dim3(kKnnBox), 0, st, P, nb, ns, sorted, boxes, supers, index_s,
                       mean_dist2);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}
