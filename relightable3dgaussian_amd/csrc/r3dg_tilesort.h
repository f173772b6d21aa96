// r3dg_tilesort.h -- the per-tile (depth bits, Gaussian id) sorts: the radix chunk sort of the
// depth-sort kernel (preprocess.hip), and the forward blend's fused sort (render_fwd.hip), a bucket
// sort that falls back to the chunk sort.
#pragma once

#include <rocprim/block/block_radix_sort.hpp>

#include "r3dg_common.h"

namespace r3dg {

constexpr int kSortBT = 256;  // threads of a tile-sorting workgroup
template <int IPT>
using TileSort = rocprim::block_radix_sort<uint32_t, kSortBT, IPT, uint32_t>;
template <int IPT>
union TileSortLds {
    typename TileSort<IPT>::storage_type sort;
    uint32_t keys[kSortBT * IPT];  // the sorted chunk's keys (tie test)
};

// One chunk of up to kSortBT * IPT (depth bits, Gaussian id) pairs held in the blocked arrangement
// (item t * IPT + k of thread t; the first n are real, pads are all-ones and sort last: visible
// depths < 0x7f800000), sorted by (depth bits, id) -- the reference's stable (tile << 32 | depth)
// sort of its Gaussian-major list breaks depth ties by Gaussian id. A rocPRIM block radix sort by
// depth over only the bits in which the chunk's keys differ (8 bits per pass: a tile's depths
// usually share their top 8 bits, so 3 passes instead of 4); a chunk in which two pairs share
// depth bits (cloned Gaussians do until they move) is sorted again, by id and then stably by
// depth. Called by every thread of the block, after a barrier that ends earlier uses of `lds`.
template <int IPT>
__device__ __forceinline__ void sort_pairs_chunk(uint32_t (&keys)[IPT], uint32_t (&vals)[IPT], int n,
                                                 TileSortLds<IPT>& lds) {
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    // the bit span in which the real keys differ: OR and AND over the chunk
    uint32_t ko = 0u, ka = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < IPT; ++k)
        if (t * IPT + k < n) { ko |= keys[k]; ka &= keys[k]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ko |= (uint32_t)__shfl_xor((int)ko, o);
        ka &= (uint32_t)__shfl_xor((int)ka, o);
    }
    if (l == 0) { lds.keys[2 * w] = ko; lds.keys[2 * w + 1] = ka; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSortBT / 64; ++k) { ko |= lds.keys[2 * k]; ka &= lds.keys[2 * k + 1]; }
    const uint32_t diff = ko ^ ka;
    const int b0 = diff ? __builtin_ctz(diff) : 0, b1 = diff ? 32 - __builtin_clz(diff) : 0;
    __syncthreads();  // lds.keys is the sort's storage too
    if (b1 > b0) TileSort<IPT>().sort(keys, vals, lds.sort, b0, b1);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < IPT; ++k) lds.keys[t * IPT + k] = keys[k];
    __syncthreads();
    bool tie = false;
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const int i = t * IPT + k;
        if (i + 1 < kSortBT * IPT && keys[k] != 0xffffffffu && lds.keys[i + 1] == keys[k]) tie = true;
    }
    if (__syncthreads_or(tie)) {  // block-uniform
        TileSort<IPT>().sort(vals, keys, lds.sort, 0, 32);
        __syncthreads();
        if (b1 > b0) TileSort<IPT>().sort(keys, vals, lds.sort, b0, b1);
    }
}

// ---------------------------------------------------------------------------------------------
// The forward blend's fused sort: a one-pass interpolation bucket sort.
// A tile's (depth bits, id) pairs are unique (a Gaussian occurs once per tile), so their sorted
// order is unique and any method that reaches it gives the radix sort's bits. The radix sort's
// time inside the blend is its passes' barriers and rank scans (3 passes of ~5 barriers, the tie
// test, two more sorts on ties); this one takes 5 barriers and a few instructions per item:
//   1. block minimum / maximum of the real keys; the bucket counters zeroed;
//   2. bucket b = (key - kmin) >> shift, shift = max(0, bitlen(kmax - kmin) - log2(kBktN)), so the
//      span fits the buckets; r = the item's arrival rank in its bucket (one LDS atomic add);
//   3. exclusive scan of the counters in place (four per thread: one ds_read_b128);
//   4. the pairs scattered to tmp[start[b] + r]: bucket order, arbitrary inside a bucket;
//   5. every position walks its own bucket's segment and counts the pairs lexicographically below
//      it by (key, id): its final rank is start[b] + that count. Depth ties need no special path.
// Fallback, block-uniform, to sort_pairs_chunk on the untouched registers: every depth equal
// (span 0), or a bucket above kBktCap (clustered depths, heavy ties).
// kBktN = 1024 with 32-bit counters: 4 KB of counters + 8 KB of pairs = 12 KB, exactly the two
// staging buffers of the S = 11 blend that the scratch aliases (no LDS added there); of the sizes
// that fit it has the shortest walks (M1-like tiles, n ~ Poisson(614), z ~ U(3, 8): the fullest
// bucket holds 5.0 pairs on average and 8 at worst over 3000 tiles, 1.9 compares per item, against
// 6.9 / 12 / 2.7 with 512 buckets), and four counters per thread make the scan one 128-bit read.
// kBktCap = 16, the low end of the useful range: twice the worst M1-like bucket, so such tiles
// never fall back, while the walk of a wave (as long as its fullest bucket) stays bounded.
// ---------------------------------------------------------------------------------------------
// (the radix sort, sort_pairs_chunk, as the fused sort: +0.037 ms of the forward blend at M1)
constexpr int kBktN = 1024;  // buckets (mirrored by tests/test_fwd_bucket_sort.py)
constexpr int kBktCap = 16;  // fullest bucket the fix-up walks; above it the radix sort
constexpr int kBktLog2 = 10;
static_assert(kBktN == 1 << kBktLog2 && kBktN == 4 * kSortBT, "four counters per thread");

template <int IPT>
struct TileBucketLds {
    uint32_t cnt[kBktN];       // bucket counts, then the buckets' first positions
    uint2 tmp[kSortBT * IPT];  // the pairs in bucket order (before the scatter: the exchange words)
};
template <int IPT>
union TileBucketSortLds {
    TileSortLds<IPT> radix;
    TileBucketLds<IPT> bkt;
};

// Wave-wide reductions by DPP (no LDS round trips, as ds_bpermute shuffles make); every lane active.
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF, bool BOUND = false>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, BANK_MASK, BOUND);
}
// unsigned maximum over the wave's 64 lanes (valid in lane 63)
__device__ __forceinline__ uint32_t wave_umax_to_lane63(uint32_t v) {
    v = max(v, dpp_u32<0xB1>(v));         // quad_perm [1,0,3,2]
    v = max(v, dpp_u32<0x4E>(v));         // quad_perm [2,3,0,1]
    v = max(v, dpp_u32<0x141>(v));        // row_half_mirror
    v = max(v, dpp_u32<0x140>(v));        // row_mirror   -> every lane: its 16-lane row's maximum
    v = max(v, dpp_u32<0x142, 0xA>(v));   // row_bcast:15 -> rows 1, 3 take in rows 0, 2
    v = max(v, dpp_u32<0x143, 0xC>(v));   // row_bcast:31 -> rows 2, 3 take in lane 31
    return v;
}
// inclusive prefix sum over the wave's 64 lanes
__device__ __forceinline__ uint32_t wave_scan_inclusive(uint32_t x) {
    x += dpp_u32<0x111, 0xF, 0xF, true>(x);  // row_shr:1, 2, 4, 8 (zero shifted in): the scan of each 16-lane row
    x += dpp_u32<0x112, 0xF, 0xF, true>(x);
    x += dpp_u32<0x114, 0xF, 0xF, true>(x);
    x += dpp_u32<0x118, 0xF, 0xF, true>(x);
    x += dpp_u32<0x142, 0xA>(x);             // row_bcast:15 -> rows 1, 3 += the total of rows 0, 2
    x += dpp_u32<0x143, 0xC>(x);             // row_bcast:31 -> rows 2, 3 += lane 31 (rows 0-1)
    return x;
}

// Up to kSortBT * IPT pairs in the blocked arrangement (the first n real), as sort_pairs_chunk;
// leaves the Gaussian ids in (depth bits, id) order in ids[0, n) (LDS, indexed by final rank; the
// caller's barrier publishes them). `lds` 16-byte aligned; called by every thread of the block,
// after a barrier that ends earlier uses of `lds`.
template <int IPT>
__device__ __forceinline__ void sort_tile_bucket(uint32_t (&keys)[IPT], uint32_t (&vals)[IPT], int n,
                                                 TileBucketSortLds<IPT>& lds, uint32_t* ids) {
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    uint32_t* const cnt = lds.bkt.cnt;
    uint2* const tmp = lds.bkt.tmp;
    uint32_t* const xch = reinterpret_cast<uint32_t*>(tmp);  // [0, 8): min / max per wave; [8, 12): scan sums
    // 1. minimum and maximum of the real keys, counters zeroed
    // (the minimum as the maximum of the complements: both reductions' identity is 0, what DPP
    // leaves in the rows a step masks off)
    uint32_t kmin = 0xffffffffu, kmax = 0u;
#pragma unroll
    for (int k = 0; k < IPT; ++k)
        if (t * IPT + k < n) { kmin = min(kmin, keys[k]); kmax = max(kmax, keys[k]); }
    kmin = ~wave_umax_to_lane63(~kmin);
    kmax = wave_umax_to_lane63(kmax);
    if (l == 63) { xch[2 * w] = kmin; xch[2 * w + 1] = kmax; }
    reinterpret_cast<uint4*>(cnt)[t] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    kmin = 0xffffffffu;
    kmax = 0u;
#pragma unroll
    for (int k = 0; k < kSortBT / 64; ++k) { kmin = min(kmin, xch[2 * k]); kmax = max(kmax, xch[2 * k + 1]); }
    kmin = (uint32_t)__builtin_amdgcn_readfirstlane((int)kmin);
    const uint32_t span = (uint32_t)__builtin_amdgcn_readfirstlane((int)(kmax - kmin));
    if (span != 0u) {  // block-uniform
        // 2. bucket and arrival rank (b < kBktN: span >> shift < 2^kBktLog2; r < n <= 2^16)
        const int shift = max(0, 32 - __builtin_clz(span) - kBktLog2);
        uint32_t br[IPT];
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            br[k] = 0u;
            if (t * IPT + k < n) {
                const uint32_t b = (keys[k] - kmin) >> shift;
                br[k] = b << 16 | atomicAdd(&cnt[b], 1u);
            }
        }
        __syncthreads();
        // 3. exclusive scan of the counters, in place; the fallback vote rides on its barrier
        const uint4 c = reinterpret_cast<const uint4*>(cnt)[t];
        const uint32_t sum = c.x + c.y + c.z + c.w;
        const uint32_t x = wave_scan_inclusive(sum);
        if (l == 63) xch[8 + w] = x;
        if (!__syncthreads_or((int)(max(max(c.x, c.y), max(c.z, c.w)) > (uint32_t)kBktCap))) {
            uint32_t run = x - sum;
            for (int k = 0; k < w; ++k) run += xch[8 + k];
            reinterpret_cast<uint4*>(cnt)[t] = make_uint4(run, run + c.x, run + c.x + c.y, run + c.x + c.y + c.z);
            __syncthreads();
            // 4. scatter into bucket order (start[b] + r < n)
#pragma unroll
            for (int k = 0; k < IPT; ++k)
                if (t * IPT + k < n) tmp[cnt[br[k] >> 16] + (br[k] & 0xffffu)] = make_uint2(keys[k], vals[k]);
            __syncthreads();
            // 5. the exact rank inside the bucket: consecutive lanes on consecutive positions
#pragma unroll
            for (int k = 0; k < IPT; ++k) {
                const int p = t + k * kSortBT;
                if (p < n) {
                    const uint2 me = tmp[p];
                    const uint32_t b = (me.x - kmin) >> shift;
                    const uint32_t e = b + 1 < (uint32_t)kBktN ? cnt[b + 1] : (uint32_t)n;
                    const uint32_t s = cnt[b];
                    const uint64_t me64 = (uint64_t)me.x << 32 | me.y;  // (key, id) order: one 64-bit compare
                    uint32_t rank = s;
                    for (uint32_t j = s; j < e; ++j) {
                        const uint2 q = tmp[j];
                        rank += (uint32_t)(((uint64_t)q.x << 32 | q.y) < me64);
                    }
                    ids[rank] = me.y;
                }
            }
            return;
        }
    } else {
        __syncthreads();  // the exchange words' reads end before the radix sort's first write
    }
    // 6. fallback: the radix sort on the untouched registers (nobody reads the scratch any more)
    sort_pairs_chunk<IPT>(keys, vals, n, lds.radix);
#pragma unroll
    for (int k = 0; k < IPT; ++k)
        if (t * IPT + k < n) ids[t * IPT + k] = vals[k];
}

}  // namespace r3dg
