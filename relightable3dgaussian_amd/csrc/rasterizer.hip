// rasterizer.hip -- host orchestration of the rasterizer and the C ABI (include/r3dg_hip.h).
//
// Restates CudaRasterizer::Rasterizer::forward / backward / markVisible
// (reference rasterizer_impl.cu:143-639) on one HIP stream (the caller's), with:
//   * no input clones when the SH shaders are the defaults (the reference clones six inputs
//     every call, rasterize_points.cu:117-122, only so shaders may mutate them);
//   * no RenderIntermediateTextures pass and no splat-shader launch when the splat shaders are
//     the defaults (their only outputs are then a stencil of zeros and shader_rgb == rgb);
//   * a single-pass inclusive scan (preprocess.hip scan_touched_kernel), then binning by per-tile
//     counters (counting and range passes overlapped with the num_rendered readback) and a per-tile
//     sort by (depth bits, Gaussian id) instead of a radix sort of L 64-bit keys (preprocess.hip
//     bin_count_kernel);
//   * one blocking D2H read of num_rendered, as the reference (rasterizer_impl.cu:347).
//
// The file holds the options, the state layouts, profiling, the readback, and the forward and the
// backward: each a plan (checks, path flags, sizes), one carver per buffer, and stages.
#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "r3dg_common.h"
#include "r3dg_kernels.h"
#include "shaders.h"

namespace r3dg {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

// ---- options (r3dg_get_options / r3dg_set_options) -------------------------------------------
// Read by the host code of each call as one snapshot. The environment is consulted once, when the
// library is loaded, and only for the supported runtime option R3DG_BWD_REDUCE.
static r3dg_options initial_options() {
    r3dg_options o{};
    o.struct_size = sizeof(r3dg_options);
    const char* e = getenv("R3DG_BWD_REDUCE");
    o.bwd_reduce = (e && e[0] == 'r') ? R3DG_REDUCE_ROWS : R3DG_REDUCE_ATOMIC;
    return o;
}
static std::mutex g_opt_mu;
static r3dg_options g_options = initial_options();
r3dg_options options() {
    std::lock_guard<std::mutex> lk(g_opt_mu);
    return g_options;
}

static inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

FeatureLayout make_feature_layout(int S, long long HW, bool native) {
    FeatureLayout f{};
    int groups[kMaxFeatures];
    const int ng = r3dg_feature_groups(S, groups);
    int c = 0;
    for (int gi = 0; gi < ng; ++gi)
        for (int k = 0; k < groups[gi]; ++k, ++c) {
            if (c >= kMaxFeatures) break;
            if (native) {
                f.a[c] = (int)(HW * (c - k) + k);
                f.m[c] = groups[gi];
            } else {  // planar [S, H, W]
                f.a[c] = (int)(HW * c);
                f.m[c] = 1;
            }
        }
    return f;
}

// ---- the backward's per-Gaussian sums ------------------------------------------------------------
// Row stride (floats) of the per-Gaussian sums of the atomic flush: [X part (f32) | 6 moments (f64) |
// pad], rows of 32 floats (128 B) so each 16-float X segment is one aligned 64-B atomic request and
// the moments are 8-B aligned (at least the X part and the 6 double moments: XW + 12 floats per row);
// test_bwd_srs (A/B) rounds up to 8 floats.
static int atomic_sums_min_stride(int S) { return 16 * bwd_xblocks(S) + 12; }
static int atomic_sums_stride(int S, const r3dg_options& opt) {
    const int srs_min = atomic_sums_min_stride(S);
    if (opt.test_bwd_srs > 0) return (std::max(srs_min, opt.test_bwd_srs) + 7) & ~7;
    return (std::max(part_row_stride(S), srs_min) + 31) & ~31;
}
// The second stage of the per-instance reduction (backward.cu:552-611 accumulates per pixel with
// atomics), decided here for the forward (which prepares the sums) and the backward alike. Default:
// the backward blend adds each (instance, wave) row into the per-Gaussian sums [P, SRS] with f32
// atomics (no partial rows, flags or row_sum_kernel; last bits depend on arrival order, as the
// reference's do; M1: step 2.00 -> 1.94 ms). bwd_reduce = R3DG_REDUCE_ROWS: partial rows [4L, RS]
// (one per instance and quadrant, written sparsely) summed in a fixed order by row_sum_kernel into
// sums [P, RS], bitwise reproducible run to run. The DPP cross-check kernel writes partial rows.
struct SumsPlan {
    bool atomic;
    int RS, SRS;                  // row strides (floats) of the partial rows / the atomic sums
    size_t row_bytes, sum_bytes;  // partial rows (none when atomic), per-Gaussian sums
};
static SumsPlan plan_sums(int P, int S, int L, const r3dg_options& opt) {
    SumsPlan p{};
    p.atomic = opt.bwd_reduce != R3DG_REDUCE_ROWS && !opt.test_bwd_dpp;
    p.RS = part_row_stride(S);
    p.SRS = atomic_sums_stride(S, opt);
    p.row_bytes = p.atomic ? 0 : sizeof(float) * (size_t)p.RS * 4 * L;
    p.sum_bytes = sizeof(float) * (size_t)(p.atomic ? p.SRS : p.RS) * P;
    return p;
}
// The hand-off of prepared sums. A default-shader forward of an atomic-mode run (no shaders, no post
// passes) appends the sums to its geometry state and has its blend zero them (the stores drain under
// the blend, which waits on latency, not on memory), so the backward launches no memset (M1: the
// 128 MB fill, 17 us per step). This map records which geometry states (by base address) hold such
// still-zero sums: the first backward on one takes them, any other backward (a second one on the same
// state, other options, a state moved to another address) zeroes scratch itself.
class PreparedSums {
    struct Entry {
        float* sums;
        int P, S, SRS;
        bool fresh;
    };
    std::mutex mu;
    std::map<uintptr_t, Entry> by_geom;

  public:
    // a forward's result for its geometry state; sums == nullptr: it prepared none. Either way a new
    // forward's state at a reused address replaces the old entry.
    void note(void* geom, float* sums, int P, int S, int SRS) {
        std::lock_guard<std::mutex> lk(mu);
        by_geom.erase((uintptr_t)geom);
        if (!sums) return;
        if (by_geom.size() >= 4096) by_geom.clear();  // entries are hints: a missing one costs a memset
        by_geom[(uintptr_t)geom] = Entry{sums, P, S, SRS, true};
    }
    // the still-zero sums behind this geometry state, once; null: the caller zeroes scratch
    float* take(void* geom, int P, int S, int SRS) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = by_geom.find((uintptr_t)geom);
        if (it == by_geom.end() || !it->second.fresh || it->second.P != P || it->second.S != S || it->second.SRS != SRS)
            return nullptr;
        it->second.fresh = false;
        return it->second.sums;
    }
};
static PreparedSums g_sums;

// ---- state buffer layouts --------------------------------------------------------------------
// the single-pass scan's status words (scan_touched_kernel): one per workgroup + the ticket counter
static size_t scan_temp_size(size_t P) { return sizeof(uint64_t) * ((size_t)scan_blocks(P) + 1); }

// Carving works on an integer cursor so the same code computes sizes (base 0) and pointers.
template <typename T>
static T* carve(uintptr_t& p, size_t count) {
    T* r = reinterpret_cast<T*>(p);
    p += align256(sizeof(T) * count);
    return r;
}

static GeomState carve_geom(uintptr_t p, size_t P, int S, uintptr_t* end) {
    GeomState g{};
    g.depths = carve<float>(p, P);
    g.internal_radii = carve<int>(p, P);
    g.means2D = carve<float2>(p, P);
    g.cov3D = carve<float>(p, 6 * P);
    g.conic_opacity = carve<float4>(p, P);
    g.rgb = carve<float>(p, 3 * P);
    g.shader_rgb = carve<float>(p, 3 * P);
    g.stencils = carve<float>(p, P);
    g.stencil_opacity = carve<float>(p, P);
    g.clamped = carve<uint8_t>(p, P);
    g.tiles_touched = carve<uint32_t>(p, P);
    g.point_offsets = carve<uint32_t>(p, P);
    g.depth_keys = carve<uint32_t>(p, P);
    g.scan_temp_bytes = scan_temp_size(P);
    g.scan_temp = carve<char>(p, g.scan_temp_bytes);
    // render records last: every other offset is independent of S
    g.records = S >= 0 ? carve<float4>(p, P * (size_t)record_f4(S)) : nullptr;
    if (end) *end = p;
    return g;
}
size_t geom_state_bytes(size_t P, int S) {
    uintptr_t end = 0;
    carve_geom(0, P, S, &end);
    return (size_t)end;
}
GeomState geom_state_from(void* base, size_t P, int S) { return carve_geom((uintptr_t)base, P, S, nullptr); }

static BinningState carve_binning(uintptr_t p, size_t L, uintptr_t* end) {
    BinningState b{};
    b.point_list = carve<uint32_t>(p, L);
    b.pairs = carve<uint2>(p, L);
    // sort_k1 | sort_v1 as one block: the two-pass scatter stages its bucketed pairs there (uint2[L])
    // before the long-tile depth sort uses them
    b.sort_k1 = reinterpret_cast<uint32_t*>(carve<uint2>(p, L));
    b.sort_v1 = b.sort_k1 + L;
    b.sort_k2 = carve<uint32_t>(p, L);
    b.flags = carve<uint32_t>(p, L);
    b.contrib = carve<uint8_t>(p, L);
    if (end) *end = p;
    return b;
}
size_t binning_state_bytes(size_t L) {
    uintptr_t end = 0;
    carve_binning(0, L, &end);
    return (size_t)end + 256;
}
BinningState binning_state_from(void* base, size_t L) { return carve_binning((uintptr_t)base, L, nullptr); }

static int num_tiles_of(int H, int W) { return ((W + kTileX - 1) / kTileX) * ((H + kTileY - 1) / kTileY); }
// the binning's per-workgroup tile counts, then (8-B aligned) bin_colscan_kernel's look-back status
// words and ticket
static size_t bin_hist_words(size_t T) { return ((size_t)bin_blocks_max((int)T) * T + 1) & ~(size_t)1; }
static size_t bin_hist_count(size_t T) { return bin_hist_words(T) + 2 * ((T + 63) / 64 + 1); }
static uint64_t* bin_tile_scan(uint32_t* hist, size_t T) { return reinterpret_cast<uint64_t*>(hist + bin_hist_words(T)); }

static ImageState carve_image(uintptr_t p, int H, int W, uintptr_t* end, bool with_hist = true) {
    ImageState s{};
    const size_t N = (size_t)H * W;
    s.final_T = carve<float>(p, N);
    s.n_contrib = carve<uint32_t>(p, N);
    const size_t T = (size_t)num_tiles_of(H, W);
    s.ranges = carve<uint2>(p, T);
    s.tile_order = carve<uint32_t>(p, padded_tile_grid((int)T));
    s.tile_work = carve<uint32_t>(p, T);
    s.bwd_work = carve<uint32_t>(p, T);
    s.bwd_rank = carve<uint32_t>(p, T);
    s.bwd_hist = carve<uint32_t>(p, kWorkBuckets);
    s.bwd_order = carve<uint32_t>(p, padded_tile_grid((int)T));
    // the binning's per-workgroup tile counts: last, so the backward's view of the buffer does
    // not depend on whether they live here (r3dg_rasterize_gaussians) or in transient scratch
    // (r3dg_rasterize_gaussians_ex)
    if (with_hist) s.bin_hist = carve<uint32_t>(p, bin_hist_count(T));
    if (end) *end = p;
    return s;
}
size_t image_state_bytes(int H, int W, bool with_hist) {
    uintptr_t end = 0;
    carve_image(0, H, W, &end, with_hist);
    return (size_t)end;
}
// the backward and the accessors never read the tile counts
ImageState image_state_from(void* base, int H, int W) { return carve_image((uintptr_t)base, H, W, nullptr, false); }

// ---- profiling events (r3dg_profile_*) -----------------------------------------------------------
struct Profiler {
    int max_records = 0;
    std::vector<hipEvent_t> ev[R3DG_PROF_KINDS][2];
    int n[R3DG_PROF_KINDS] = {0};
};
static Profiler g_prof;
static std::mutex g_prof_mu;

static thread_local LaunchEvents t_pending;
LaunchEvents take_launch_events() {
    const LaunchEvents e = t_pending;
    t_pending = LaunchEvents{};
    return e;
}

// A profiled stage. Kernel stages (the default) pass the events to their launch (launch_kernel,
// r3dg_kernels.h): timestamps inside the dispatch packet, no marker packets between kernels.
// Marker stages (library calls such as the rocPRIM sorts) record the events around the calls;
// they are recorded only with the prof_sort_markers option, since marker packets add gaps to the
// stream.
struct ProfScope {
    int k;
    hipStream_t st;
    bool marker;
    int idx = -1;
    ProfScope(int kind, hipStream_t s, bool markers = false, bool sort_markers = false)
        : k(kind), st(s), marker(markers) {
        if (marker && !sort_markers) return;
        if (g_prof.max_records > 0 && g_prof.n[k] < g_prof.max_records) {
            idx = g_prof.n[k]++;
            if (marker) (void)hipEventRecord(g_prof.ev[k][0][idx], st);
            else t_pending = LaunchEvents{g_prof.ev[k][0][idx], g_prof.ev[k][1][idx]};
        }
    }
    ~ProfScope() {
        if (idx < 0) return;
        if (marker) {
            (void)hipEventRecord(g_prof.ev[k][1][idx], st);
        } else if (t_pending.start) {  // no launch took the events (empty stage): zero duration
            (void)hipEventRecord(t_pending.start, st);
            (void)hipEventRecord(t_pending.stop, st);
            t_pending = LaunchEvents{};
        }
    }
};

// Pinned host words for the num_rendered readback, one per (host thread, device): a
// thread's calls on one device are issued in order, so the slot is free again by its next call.
struct Readback {
    uint32_t* host = nullptr;      // pinned, coherent host words (num_rendered, the error flag)
    uint32_t* host_dev = nullptr;  // the same words as the device addresses them
    uint32_t* dev_flag = nullptr;  // preprocess error flag (prefiltered runs only)
};
static hipError_t readback_slot(Readback** out) {
    constexpr int kMaxDevices = 64;
    thread_local Readback slots[kMaxDevices];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
    Readback& r = slots[dev];
    if (!r.host) {
        void* p = nullptr;
        if ((e = hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess) return e;
        void* d = nullptr;
        if ((e = hipHostGetDevicePointer(&d, p, 0)) != hipSuccess) {
            (void)hipHostFree(p);
            return e;
        }
        r.host = static_cast<uint32_t*>(p);
        r.host_dev = static_cast<uint32_t*>(d);
    }
    *out = &r;
    return hipSuccess;
}


// The host waits for scan_touched_kernel's word itself instead of an event behind the kernel: an
// event record between two kernels of the stream cost a 5.5 us dispatch gap at M1 (round 6). The
// word starts at kUnpublished (num_rendered < 2^31 never is); the stream is queried every few
// thousand spins so a failed launch or a fault surfaces as its error instead of a hang.
constexpr uint32_t kUnpublished = 0xffffffffu;
static hipError_t wait_published(const Readback* rb, hipStream_t st) {
    volatile uint32_t* w = rb->host;
    for (uint64_t spin = 1;; ++spin) {
        if (w[0] != kUnpublished) return hipSuccess;
        if ((spin & 4095) == 0) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) return w[0] != kUnpublished ? hipSuccess : hipErrorUnknown;  // drained, no word
            if (q != hipErrorNotReady) return q;
        }
    }
}


}  // namespace r3dg

using namespace r3dg;

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" int r3dg_abi_version(void) { return R3DG_ABI_VERSION; }
extern "C" const char* r3dg_last_error(void) { return g_last_error.c_str(); }

extern "C" int r3dg_get_options(r3dg_options* o) {
    R3DG_REQUIRE(o && o->struct_size == sizeof(r3dg_options), "get_options: struct_size must be sizeof(r3dg_options)");
    *o = options();
    return R3DG_OK;
}

extern "C" int r3dg_set_options(const r3dg_options* o) {
    R3DG_REQUIRE(o && o->struct_size == sizeof(r3dg_options), "set_options: struct_size must be sizeof(r3dg_options)");
    R3DG_REQUIRE(o->bwd_reduce == R3DG_REDUCE_ATOMIC || o->bwd_reduce == R3DG_REDUCE_ROWS,
                 "set_options: bwd_reduce must be R3DG_REDUCE_ATOMIC or R3DG_REDUCE_ROWS");
    R3DG_REQUIRE(o->test_bwd_wterms == 0 || o->test_bwd_wterms == 1 || o->test_bwd_wterms == 3,
                 "set_options: test_bwd_wterms must be 0, 1 or 3");
    R3DG_REQUIRE(o->test_bin_blocks >= 0 && o->test_bwd_srs >= 0 && o->test_bwd_srs <= 4096 &&
                     o->test_bvh_lanes >= 0 && o->test_bvh_lanes <= 64 && o->test_bvh_sort >= 0 &&
                     o->test_bvh_sort <= 2,
                 "set_options: option out of range");
    std::lock_guard<std::mutex> lk(g_opt_mu);
    g_options = *o;
    return R3DG_OK;
}

extern "C" int r3dg_feature_groups(int S, int* groups) {
    int n = 0;
    if (S == 21) {
        const int g[9] = {1, 1, 1, 3, 3, 3, 3, 3, 3};
        for (n = 0; n < 9; ++n) groups[n] = g[n];
    } else if (S == 11) {
        const int g[5] = {1, 1, 3, 3, 3};
        for (n = 0; n < 5; ++n) groups[n] = g[n];
    } else {
        for (n = 0; n < S; ++n) groups[n] = 1;
    }
    return n;
}

extern "C" size_t r3dg_image_state_n_contrib_offset(int H, int W) { return align256(4 * (size_t)H * W); }
extern "C" size_t r3dg_geom_state_bytes(int P, int S) { return geom_state_bytes(P > 0 ? (size_t)P : 0, S); }

extern "C" int r3dg_rasterize_gaussians(const r3dg_raster_settings* s, const r3dg_gaussians* g,
                                        const r3dg_forward_outputs* out, r3dg_alloc_fn geom_alloc, void* geom_ctx,
                                        r3dg_alloc_fn binning_alloc, void* binning_ctx, r3dg_alloc_fn image_alloc,
                                        void* image_ctx, int* num_rendered, r3dg_stream_t stream) {
    return r3dg_rasterize_gaussians_ex(s, g, out, geom_alloc, geom_ctx, binning_alloc, binning_ctx, image_alloc,
                                       image_ctx, nullptr, nullptr, num_rendered, stream);
}

// ---- forward: the plan ------------------------------------------------------------------------------
// Everything the forward decides before it allocates: sizes, the resolved shader and texture
// managers, the post-pass ids and every path flag.
struct ForwardPlan {
    int P, S, H, W, gx, gy, T;
    float focal_x, focal_y;
    size_t M3;  // floats per Gaussian of the SH block (0 with precomputed colours)
    // shaders (forward.cu:805-971): SH shaders shade working copies of the inputs before
    // preprocessing, splat shaders run after the intermediate depth/stencil pass
    const ShaderManagerObj *shm, *spm;
    const std::map<std::string, TexDesc>* tex_names;
    TexDesc tex_error, shadow_tex;
    std::vector<int> post_ids;  // post-process passes (rasterizer_impl.cu:485-529): registry ids in list order
    bool sh_active, splat_active, post_blur;
    // Only the inputs an active shader writes get a working copy (the others are read in place;
    // shaders.hip): positions (SH ExpPos / Heartbeat / GaussDissolve), scales (ExpPos / Heartbeat /
    // CullHalf), opacity (CullHalf / GaussDissolve), the SH block (GaussDissolve: sh0), features
    // (splat CrackNoRecon / RoughnessOnly / QuantizeLight); rotations never. The reference copies all
    // six (rasterize_points.cu:117-122): results are the same, the copies were 0.11 ms per frame at
    // M1 with S = 21.
    bool w_pos, w_scale, w_opac, w_sh, w_feat;
    // the splat shaders that read the intermediate depth image (Crack, CrackNoRecon: the depth at the
    // mean pixel); without them the pre-shader intermediate pass only yields a stencil of zeros (every
    // stencil opacity is still InitializeStencil's 0 there, so every stencil alpha is 0) and the
    // blend overwrites its depth, so it is replaced by a memset
    bool inter_pre;
    bool stencils;   // the shaders or the intermediate pass read the per-Gaussian stencils
    bool inter_rec;  // the intermediate depth / stencil pass runs: its packed per-Gaussian records
    // With depth-reading splat shaders the intermediate depth / stencil pass is the first consumer of
    // the sorted order: every tile is sorted by tile_depth_sort_kernel first (sorting in that pass's
    // prologue, as the blend does, measured slower: its larger LDS costs the pass more occupancy
    // than the separate sort, 0.43 + 0.10 -> 0.52 + 0.03 ms per frame at M1 / S = 21, round 5).
    // Otherwise the blend is the first consumer and sorts tiles of up to kFusedSortMax itself, but
    // only for S <= 12: with more feature channels its registers leave fewer waves to hide the
    // sort's barriers (M1 with S = 21: fused blend 0.78 ms vs 0.49 + 0.10 ms for the separate sort)
    bool fuse_sort;
    // With a scratch allocator (one call, stream-ordered memory freed when the call returns) the
    // forward-only transients live there instead of in the state autograd keeps until the
    // backward: the binning's per-workgroup tile counts (needed until the scatter) and the splat
    // shaders' / intermediate pass's per-Gaussian records (112 MB at 1M Gaussians with S = 21).
    bool use_scratch;
    // a default-shader forward of an atomic-mode run prepares the backward's zeroed sums at the end
    // of its geometry state (PreparedSums)
    bool prep_sums;
    SumsPlan sums;

    // TextureManager::GetTexture (texture.cu:298-314): the error texture for a missing name
    bool texture(const char* name, TexDesc* d) const {
        if (!name) return true;
        if (!tex_names) return false;
        auto it = tex_names->find(name);
        *d = it == tex_names->end() ? tex_error : it->second;
        return true;
    }
};

static bool check_shader(const ForwardPlan& p, int kind, int id) {
    const bool feats = kind == R3DG_SHADER_SH ? sh_shader_needs_features(id) : splat_shader_needs_features(id);
    if (feats && p.S < 21) {
        set_error("rasterize_gaussians: shader " + shader_names(kind)[id] +
                  " addresses the reference's 21-channel feature layout (ShShader.h/splatShader.h); S < 21");
        return false;
    }
    TexDesc d{};
    const char* t0 = kind == R3DG_SHADER_SH ? sh_shader_texture(id, 0) : splat_shader_texture(id);
    const char* t1 = kind == R3DG_SHADER_SH ? sh_shader_texture(id, 1) : nullptr;
    if (!p.texture(t0, &d) || !p.texture(t1, &d)) {
        set_error("rasterize_gaussians: shader " + shader_names(kind)[id] + " samples textures; pass a "
                  "texture manager (UploadTexturesToDevice)");
        return false;
    }
    return true;
}

static int plan_post_passes(const r3dg_raster_settings* s, const r3dg_forward_outputs* out, ForwardPlan& p) {
    for (int i = 0; i < s->n_post_passes; ++i) {
        const int64_t h = s->post_passes[i];
        const int id = handle_index(h);
        R3DG_REQUIRE(handle_kind(h) == R3DG_SHADER_POST && id >= 0 && id < (int)shader_names(R3DG_SHADER_POST).size(),
                     "rasterize_gaussians: unknown post-process pass handle (GetPostProcessShaderAddressMap)");
        const std::string& name = shader_names(R3DG_SHADER_POST)[id];
        if (post_pass_needs_features(id) && p.S != 21) {
            set_error("rasterize_gaussians: post-process pass " + name +
                      " reads the reference's 21-channel feature image (postProcessShader.cu:17-28); S != 21");
            return R3DG_ERR_ARG;
        }
        if (post_pass_needs_shadow(id) && !p.texture("shadow", &p.shadow_tex)) {
            set_error("rasterize_gaussians: post-process pass " + name +
                      " samples the \"shadow\" texture; pass a texture manager (UploadTexturesToDevice)");
            return R3DG_ERR_ARG;
        }
        p.post_blur = p.post_blur || id == kPpBlurLighting;
        p.post_ids.push_back(id);
    }
    R3DG_REQUIRE(p.post_ids.empty() || (out->color && out->opacity && out->depth && out->stencil && out->shader_color &&
                                        out->normal && out->surface_xyz && (p.S == 0 || out->feature)),
                 "rasterize_gaussians: post-process passes need every image output");
    return R3DG_OK;
}

static int plan_forward(const r3dg_raster_settings* s, const r3dg_gaussians* g, const r3dg_forward_outputs* out,
                        int* num_rendered, bool scratch_given, const r3dg_options& opt, ForwardPlan& p) {
    R3DG_REQUIRE(s && g && out && num_rendered, "rasterize_gaussians: null argument");
    R3DG_REQUIRE(s->struct_size == sizeof(r3dg_raster_settings),
                 "rasterize_gaussians: settings->struct_size must be sizeof(r3dg_raster_settings) (ABI 2)");
    const int P = p.P = s->P, S = p.S = s->S, H = p.H = s->H, W = p.W = s->W;
    R3DG_REQUIRE(P >= 0 && H > 0 && W > 0, "rasterize_gaussians: invalid sizes");
    R3DG_REQUIRE(S >= 0 && S <= kMaxFeatures, "rasterize_gaussians: at most 32 feature channels are supported");
    R3DG_REQUIRE((g->colors_precomp != nullptr) != (g->sh != nullptr) || P == 0,
                 "Please provide excatly one of either SHs or precomputed colors!");
    R3DG_REQUIRE(((g->scales && g->rotations) != (g->cov3D_precomp != nullptr)) || P == 0,
                 "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    R3DG_REQUIRE(S == 0 || P == 0 || g->features, "rasterize_gaussians: features missing");
    R3DG_REQUIRE(!g->sh || P == 0 || (s->D >= 0 && s->D <= 3 && (s->D + 1) * (s->D + 1) <= s->M && s->M <= 16),
                 "rasterize_gaussians: SH degree must be 0..3 with (degree+1)^2 <= M <= 16 coefficients");
    R3DG_REQUIRE((long long)H * W * (S > 3 ? S : 3) < (1ll << 31), "rasterize_gaussians: image too large");
    *num_rendered = 0;

    p.shm = lookup_manager(s->sh_shader_manager);
    p.spm = lookup_manager(s->splat_shader_manager);
    R3DG_REQUIRE(s->sh_shader_manager == 0 || p.shm, "rasterize_gaussians: unknown SH shader manager handle");
    R3DG_REQUIRE(s->splat_shader_manager == 0 || p.spm, "rasterize_gaussians: unknown splat shader manager handle");
    R3DG_REQUIRE(!p.shm || p.shm->kind == R3DG_SHADER_SH, "rasterize_gaussians: h_shShaderManager is not an SH manager");
    R3DG_REQUIRE(!p.spm || p.spm->kind == R3DG_SHADER_SPLAT,
                 "rasterize_gaussians: h_splatShaderManager is not a splat manager");
    R3DG_REQUIRE(s->n_post_passes >= 0 && (s->n_post_passes == 0 || s->post_passes),
                 "rasterize_gaussians: invalid post-process pass list");
    p.sh_active = P > 0 && p.shm && !p.shm->all_default;
    p.splat_active = P > 0 && p.spm && !p.spm->all_default;
    if (s->texture_manager)
        R3DG_REQUIRE(lookup_texture_manager(s->texture_manager, &p.tex_names, &p.tex_error),
                     "rasterize_gaussians: unknown texture manager handle");
    if (p.sh_active) {
        R3DG_REQUIRE(g->scales && g->rotations && g->sh,
                     "rasterize_gaussians: SH shaders need scales, rotations and SH coefficients");
        for (int id = 0; id < (int)p.shm->counts.size(); ++id)
            if (p.shm->counts[id] > 0 && id != kShDefault && !check_shader(p, R3DG_SHADER_SH, id)) return R3DG_ERR_ARG;
    }
    if (p.splat_active)
        for (int id = 0; id < (int)p.spm->counts.size(); ++id)
            if (p.spm->counts[id] > 0 && !check_shader(p, R3DG_SHADER_SPLAT, id)) return R3DG_ERR_ARG;
    if (int rc = plan_post_passes(s, out, p)) return rc;

    p.gx = (W + kTileX - 1) / kTileX;
    p.gy = (H + kTileY - 1) / kTileY;
    p.T = p.gx * p.gy;
    p.focal_y = H / (2.0f * s->tan_fovy);
    p.focal_x = W / (2.0f * s->tan_fovx);
    p.M3 = (size_t)3 * (g->sh ? s->M : 0);
    auto sh_on = [&](int id) { return p.sh_active && id < (int)p.shm->counts.size() && p.shm->counts[id] > 0; };
    auto sp_on = [&](int id) { return p.splat_active && id < (int)p.spm->counts.size() && p.spm->counts[id] > 0; };
    p.w_pos = sh_on(kShExpPos) || sh_on(kShHeartbeat) || sh_on(kShGaussDissolve);
    p.w_scale = sh_on(kShExpPos) || sh_on(kShHeartbeat) || sh_on(kShCullHalf);
    p.w_opac = sh_on(kShCullHalf) || sh_on(kShGaussDissolve);
    p.w_sh = sh_on(kShGaussDissolve);
    p.w_feat = sp_on(kSpCrackNoRecon) || sp_on(kSpRoughnessOnly) || sp_on(kSpQuantizeLight);
    p.inter_pre = sp_on(kSpCrack) || sp_on(kSpCrackNoRecon);
    p.stencils = P > 0 && (p.sh_active || p.splat_active || !p.post_ids.empty());
    p.inter_rec = P > 0 && (p.splat_active || !p.post_ids.empty());
    p.fuse_sort = !(p.splat_active && p.inter_pre) && S <= 12;
    p.use_scratch = scratch_given && P > 0;
    p.sums = plan_sums(P, S, 0, opt);
    p.prep_sums = P > 0 && p.sums.atomic && !p.sh_active && !p.splat_active && p.post_ids.empty();
    return R3DG_OK;
}

// ---- forward: the tail of the geometry state and the transient scratch -----------------------------
// The one place that lays these two allocations out (DESIGN.md §3 has the table of who writes and
// reads each region). After the geometry state proper (the backward never reads the rest):
//   floats, packed   the working copies of the inputs an active shader writes, then BlurLighting's
//                    incident-light snapshot [3, H, W]
//   16-B aligned     the per-Gaussian records: the splat shaders' [P, record_f4(S) - 2] float4, then
//                    the intermediate depth / stencil pass's [P] float4 (launch_intermediate)
//   256-B aligned    the backward's prepared sums [P, SRS]
// With a scratch allocator the records live in scratch instead, after the binning's per-workgroup
// tile counts (rounded to 256 B); without one the counts are the image state's last array.
struct ForwardRegions {
    float *means3D, *scales, *opacity, *sh, *features;  // working copies; null: read in place
    float* blur_snapshot;
    float4 *shader_rec, *inter_rec;
    float* sums;
    uint32_t* bin_hist;                // scratch only
    size_t geom_bytes, scratch_bytes;  // the two requests: geometry state with its tail, scratch
};
struct Cursor {
    uintptr_t base;
    size_t off = 0;
    template <typename T>
    T* take(size_t count, bool on = true) {
        if (!on) return nullptr;
        T* r = reinterpret_cast<T*>(base + off);
        off += sizeof(T) * count;
        return r;
    }
    void align(size_t a) { off = (off + a - 1) & ~(a - 1); }
};
// base 0 gives the sizes, the real bases the pointers (as carve_geom)
static ForwardRegions carve_forward(const ForwardPlan& p, void* geom_base, void* scratch_base) {
    ForwardRegions r{};
    const size_t P = (size_t)p.P, state = geom_state_bytes(P, p.S);
    Cursor g{(uintptr_t)geom_base + state}, s{(uintptr_t)scratch_base};
    r.means3D = g.take<float>(3 * P, p.w_pos);
    r.scales = g.take<float>(3 * P, p.w_scale);
    r.opacity = g.take<float>(P, p.w_opac);
    r.sh = g.take<float>(p.M3 * P, p.w_sh);
    r.features = g.take<float>((size_t)p.S * P, p.w_feat);
    r.blur_snapshot = g.take<float>((size_t)3 * p.H * p.W, p.post_blur);
    g.align(16);
    if (p.use_scratch) {
        r.bin_hist = s.take<uint32_t>(bin_hist_count((size_t)p.T));
        s.align(256);
    }
    Cursor& rec = p.use_scratch ? s : g;
    r.shader_rec = rec.take<float4>(P * (record_f4(p.S) - 2), p.splat_active);
    r.inter_rec = rec.take<float4>(P, p.inter_rec);
    g.align(256);
    r.sums = g.take<float>((size_t)p.sums.SRS * P, p.prep_sums);
    r.geom_bytes = state + g.off;
    r.scratch_bytes = s.off;
    return r;
}

// ---- forward: stages ----------------------------------------------------------------------------------
struct ForwardCtx {
    const r3dg_raster_settings* s;
    const r3dg_gaussians* g;
    const r3dg_forward_outputs* out;
    r3dg_options opt;  // one snapshot for the call
    hipStream_t st;
    ForwardPlan plan;
    ForwardRegions reg;
    GeomState geom;
    ImageState img;
    BinningState bin;  // carved by stage_binning, once num_rendered is known
    int* radii;
    // the inputs as the kernels read them: the working copy where a shader writes one
    const float *means3D, *scales, *rotations, *opacity, *shs;
    float* feats;
};

// working copies, InitializeStencil, RunSHShaders (forward.cu:805-877)
static int stage_sh_shaders(ForwardCtx& c) {
    const ForwardPlan& p = c.plan;
    const r3dg_gaussians* g = c.g;
    const size_t P = (size_t)p.P;
    hipError_t ce = hipSuccess;
    auto copy = [&](const float* src, float* dst, size_t n) -> const float* {
        if (!dst) return src;  // read in place: no active shader writes it
        if (src && n && ce == hipSuccess) ce = hipMemcpyAsync(dst, src, sizeof(float) * n, hipMemcpyDeviceToDevice, c.st);
        return src ? dst : nullptr;
    };
    c.means3D = copy(g->means3D, c.reg.means3D, 3 * P);
    c.scales = copy(g->scales, c.reg.scales, 3 * P);
    c.rotations = g->rotations;
    c.opacity = copy(g->opacity, c.reg.opacity, P);
    c.shs = copy(g->sh, c.reg.sh, p.M3 * P);
    c.feats = const_cast<float*>(copy(g->features, c.reg.features, (size_t)p.S * P));
    R3DG_CHECK_HIP(ce);
    // only the shaders and the intermediate depth / stencil pass read the per-Gaussian stencils; the
    // all-default path skips the launch
    if (p.stencils) {
        launch_init_stencil(p.P, c.geom.stencils, c.geom.stencil_opacity, c.st);
        R3DG_CHECK_LAUNCH(c.s->debug, c.st);
    }
    if (!p.sh_active) return R3DG_OK;
    for (int id = 0; id < (int)p.shm->counts.size(); ++id) {  // one launch per non-empty bucket
        if (p.shm->counts[id] == 0 || id == kShDefault) continue;
        ShShaderArgs sa{};
        sa.idx = p.shm->d_lists[id]; sa.n = p.shm->counts[id]; sa.time = c.s->time; sa.dt = c.s->dt;
        sa.pos = const_cast<float*>(c.means3D); sa.scale = const_cast<float*>(c.scales);
        sa.rot = const_cast<float*>(c.rotations); sa.opacity = const_cast<float*>(c.opacity);
        sa.sh = const_cast<float*>(c.shs); sa.M = c.s->M; sa.features = c.feats; sa.S = p.S;
        p.texture(sh_shader_texture(id, 0), &sa.tex0);
        p.texture(sh_shader_texture(id, 1), &sa.tex1);
        R3DG_CHECK_HIP(launch_sh_shader(id, sa, c.st));
        R3DG_CHECK_LAUNCH(c.s->debug, c.st);
    }
    return R3DG_OK;
}

static BinArgs binning_args(const ForwardCtx& c) {
    const ForwardPlan& p = c.plan;
    BinArgs b{};
    b.P = p.P; b.grid_x = p.gx; b.grid_y = p.gy; b.rec4 = record_f4(p.S); b.T = p.T;
    b.offsets = c.geom.point_offsets; b.means2D = c.geom.means2D; b.radii = c.radii;
    b.depth_keys = c.geom.depth_keys;
    b.tile_work = c.img.tile_work;
    const bool lds = bin_blocks_max(p.T) > 0 && !c.opt.test_bin_atomic;  // test_bin_atomic: the fallback (tests)
    int nb = bin_blocks_max(p.T);
    if (c.opt.test_bin_blocks > 0) nb = std::min(nb, c.opt.test_bin_blocks);  // experiments
    b.nblk = lds ? std::min(nb, (p.P + kBinSub - 1) / kBinSub) : 0;
    b.hist = lds && p.P > 0 ? c.img.bin_hist : nullptr;
    b.tile_scan = b.hist ? bin_tile_scan(c.img.bin_hist, (size_t)p.T) : nullptr;
    return b;
}

static PreprocessArgs preprocess_args(const ForwardCtx& c, const BinArgs& binning) {
    const ForwardPlan& p = c.plan;
    const r3dg_raster_settings* s = c.s;
    const GeomState& geom = c.geom;
    PreprocessArgs pa{};
    pa.P = p.P; pa.D = s->D; pa.M = s->M; pa.W = p.W; pa.H = p.H; pa.grid_x = p.gx; pa.grid_y = p.gy;
    pa.prefiltered = s->prefiltered;
    pa.focal_x = p.focal_x; pa.focal_y = p.focal_y; pa.tan_fovx = s->tan_fovx; pa.tan_fovy = s->tan_fovy;
    pa.scale_modifier = s->scale_modifier;
    pa.means3D = c.means3D; pa.scales = c.scales; pa.rotations = c.rotations; pa.opacity = c.opacity;
    pa.sh = c.shs; pa.cov3D_precomp = c.g->cov3D_precomp; pa.colors_precomp = c.g->colors_precomp;
    pa.view = s->viewmatrix; pa.proj = s->projmatrix; pa.campos = s->campos;
    pa.radii = c.radii; pa.tiles_touched = geom.tiles_touched; pa.depth_keys = geom.depth_keys;
    pa.records = geom.records; pa.rec4 = record_f4(p.S); pa.S = p.S; pa.features = c.g->features;
    pa.depths = geom.depths;
    pa.means2D = geom.means2D; pa.cov3D = geom.cov3D; pa.conic_opacity = geom.conic_opacity;
    pa.rgb = geom.rgb; pa.clamped = geom.clamped; pa.error_flag = nullptr;
    pa.tile_count = binning.hist ? nullptr : c.img.tile_work;  // the atomic binning's counters
    pa.num_tiles = p.T;
    pa.scan_status = reinterpret_cast<uint64_t*>(geom.scan_temp);  // zeroed for scan_touched_kernel
    pa.scan_words = scan_blocks((size_t)p.P) + 1;
    pa.work_hist = c.img.bwd_hist;  // the forward's work buckets start at zero
    return pa;
}

// preprocess, scan and the binning passes that need only the scan, then the num_rendered readback
static int project_and_count(ForwardCtx& c, const BinArgs& binning, int* L) {
    const r3dg_raster_settings* s = c.s;
    const int P = c.plan.P;
    hipStream_t st = c.st;
    PreprocessArgs pa = preprocess_args(c, binning);
    Readback* rb = nullptr;
    R3DG_CHECK_HIP(readback_slot(&rb));
    if (s->prefiltered) {
        // the reference __trap()s on a point the frustum test drops although the caller
        // promised a prefiltered set (auxiliary.h:154-160); here the kernel raises a flag and
        // the call fails with R3DG_ERR_ARG
        if (!rb->dev_flag) R3DG_CHECK_HIP(hipMalloc(&rb->dev_flag, sizeof(uint32_t)));
        R3DG_CHECK_HIP(hipMemsetAsync(rb->dev_flag, 0, sizeof(uint32_t), st));
        pa.error_flag = rb->dev_flag;
    }
    {
        ProfScope ps(R3DG_PROF_PREPROCESS, st);
        launch_kernel(preprocess_kernel, dim3((P + 255) / 256), dim3(256), st, pa);
    }
    R3DG_CHECK_LAUNCH(s->debug, st);

    // offsets = inclusive scan of tiles_touched; num_rendered (rasterizer_impl.cu:259-263 reads it
    // with a blocking cudaMemcpy) written by the scan's last workgroup into pinned coherent host
    // memory, which the host polls (wait_published)
    reinterpret_cast<volatile uint32_t*>(rb->host)[0] = kUnpublished;
    R3DG_CHECK_HIP(launch_scan_touched(c.geom.tiles_touched, c.geom.point_offsets, P,
                                       reinterpret_cast<uint64_t*>(c.geom.scan_temp),
                                       s->prefiltered ? rb->dev_flag : nullptr, rb->host_dev, st));
    // binning passes that need only the scan: per-tile counts, ranges, the tile order and the
    // scatter positions run on the device while the host waits for num_rendered and allocates
    {
        ProfScope ps(R3DG_PROF_SORT, st, true, c.opt.prof_sort_markers);
        R3DG_CHECK_HIP(launch_bin_prepare(binning, c.img.ranges, c.img.tile_order, st));
        R3DG_CHECK_LAUNCH(s->debug, st);
    }
    R3DG_CHECK_HIP(wait_published(rb, st));
    const uint32_t Lh = *reinterpret_cast<volatile uint32_t*>(rb->host);
    R3DG_REQUIRE(!s->prefiltered || reinterpret_cast<volatile uint32_t*>(rb->host)[1] == 0,
                 "rasterize_gaussians: point is filtered although prefiltered is set (the reference traps, "
                 "auxiliary.h:156-160)");
    R3DG_REQUIRE(Lh < (1u << 31), "rasterize_gaussians: too many tile instances");
    *L = (int)Lh;
    return R3DG_OK;
}

// preprocess to the sorted per-tile lists; the binning state is allocated once L is known
static int stage_binning(ForwardCtx& c, r3dg_alloc_fn binning_alloc, void* binning_ctx, int* L_out) {
    const ForwardPlan& p = c.plan;
    const ImageState& img = c.img;
    hipStream_t st = c.st;
    BinArgs binning = binning_args(c);
    int L = 0;
    if (p.P > 0) {
        if (int rc = project_and_count(c, binning, &L)) return rc;
    } else if (p.T > 0) {  // no Gaussians: every tile range empty
        R3DG_CHECK_HIP(hipMemsetAsync(img.tile_work, 0, sizeof(uint32_t) * (size_t)p.T, st));
        R3DG_CHECK_HIP(hipMemsetAsync(img.bwd_hist, 0, sizeof(uint32_t) * kWorkBuckets, st));  // (no preprocess)
        R3DG_CHECK_HIP(launch_bin_prepare(binning, img.ranges, img.tile_order, st));
        R3DG_CHECK_LAUNCH(c.s->debug, st);
    }

    void* bin_base = binning_alloc(binning_ctx, binning_state_bytes((size_t)L));
    if (!bin_base) {
        set_error("rasterize_gaussians: binning allocation failed");
        return R3DG_ERR_ALLOC;
    }
    c.bin = binning_state_from(bin_base, (size_t)L);
    if (L == 0) R3DG_CHECK_HIP(launch_bin_order(binning, img.ranges, img.tile_order, st));  // (no scatter)
    if (L > 0) {
        // every instance to its tile's next position (also records each Gaussian's first slot),
        // then every tile by (depth bits, Gaussian id): the
        // reference's 45-bit stable sort of (tile << 32 | depth bits) (rasterizer_impl.cu:366-374)
        ProfScope ps(R3DG_PROF_SORT, st, true, c.opt.prof_sort_markers);
        binning.pairs = c.bin.pairs;
        binning.flags = nullptr;  // the rows reduction zeroes its flags itself (backward)
        binning.L = (uint32_t)L;
        // two-pass scatter through tile buckets (the staged ids carry the tile's index in its bucket
        // in their top bits); test_bin_one_pass: straight to the tiles
        binning.stage = (!c.opt.test_bin_one_pass && p.P < (1 << kBinBucketShift))
                            ? reinterpret_cast<uint2*>(c.bin.sort_k1)
                            : nullptr;
        R3DG_CHECK_HIP(launch_bin_scatter(binning, img.ranges, img.tile_order, st));
        R3DG_CHECK_LAUNCH(c.s->debug, st);
        // the default-shader blend sorts the tiles of up to kFusedSortMax instances itself
        R3DG_CHECK_HIP(launch_tile_depth_sort(p.T, img.ranges, img.tile_order, c.bin.pairs, c.bin.point_list,
                                              c.bin.sort_k1, c.bin.sort_v1, c.bin.sort_k2,
                                              p.fuse_sort ? kFusedSortMax : 0, st));
        R3DG_CHECK_LAUNCH(c.s->debug, st);
    }
    *L_out = L;
    return R3DG_OK;
}

// RenderIntermediateTextures (forward.cu:271-383): depth + stencil images
static IntermediateArgs intermediate_args(const ForwardCtx& c) {
    const ForwardPlan& p = c.plan;
    const GeomState& geom = c.geom;
    IntermediateArgs ia{};
    ia.ranges = c.img.ranges; ia.point_list = c.bin.point_list; ia.means2D = geom.means2D;
    ia.conic_opacity = geom.conic_opacity; ia.depths = geom.depths; ia.stencils = geom.stencils;
    ia.stencil_opacity = geom.stencil_opacity; ia.W = p.W; ia.H = p.H; ia.grid_x = p.gx; ia.num_tiles = p.T;
    ia.out_depth = c.out->depth; ia.out_stencil = c.out->stencil;
    ia.records = geom.records; ia.rec4 = record_f4(p.S); ia.inter_rec = c.reg.inter_rec;
    ia.tile_order = c.img.tile_order;  // longest tiles first, as the blends
    return ia;
}

// the intermediate pass (or a memset), RunSplatShaders (forward.cu:907-971), the records' refresh
static int stage_splat_shaders(ForwardCtx& c) {
    const ForwardPlan& p = c.plan;
    const r3dg_raster_settings* s = c.s;
    const GeomState& geom = c.geom;
    hipStream_t st = c.st;
    if (!p.splat_active) return R3DG_OK;
    // the splat shaders read the intermediate depth / stencil images
    R3DG_REQUIRE(c.out->depth && c.out->stencil, "rasterize_gaussians: splat shaders need depth and stencil outputs");
    if (p.inter_pre) {
        R3DG_CHECK_HIP(launch_intermediate(intermediate_args(c), p.P, c.radii, st));
    } else {
        R3DG_CHECK_HIP(hipMemsetAsync(c.out->stencil, 0, sizeof(float) * (size_t)p.H * p.W, st));
    }
    R3DG_CHECK_LAUNCH(s->debug, st);
    for (int id = 0; id < (int)p.spm->counts.size(); ++id) {
        if (p.spm->counts[id] == 0) continue;
        SplatShaderArgs sp{};
        sp.idx = p.spm->d_lists[id]; sp.n = p.spm->counts[id]; sp.W = p.W; sp.H = p.H; sp.time = s->time;
        sp.dt = s->dt; sp.pos = c.means3D; sp.means2D = geom.means2D; sp.depth_tex = c.out->depth;
        sp.stencil_tex = c.out->stencil; sp.viewmatrix_inv = s->viewmatrix_inv; sp.depths = geom.depths;
        // the reference passes geomState.rgb even with precomputed colours (then uninitialised)
        sp.rgb = c.g->colors_precomp ? c.g->colors_precomp : geom.rgb;
        sp.conic_opacity = geom.conic_opacity; sp.features = c.feats; sp.S = p.S; sp.stencils = geom.stencils;
        sp.stencil_opacity = geom.stencil_opacity; sp.out_rgb = geom.shader_rgb;
        p.texture(splat_shader_texture(id), &sp.tex0);
        R3DG_CHECK_HIP(launch_splat_shader(id, sp, st));
        R3DG_CHECK_LAUNCH(s->debug, st);
    }
    launch_shader_records(p.P, p.S, record_f4(p.S), c.radii, geom.conic_opacity, geom.records, geom.shader_rgb,
                          c.feats, c.reg.shader_rec, st);
    R3DG_CHECK_LAUNCH(s->debug, st);
    return R3DG_OK;
}

static RenderFwdArgs render_fwd_args(const ForwardCtx& c) {
    const ForwardPlan& p = c.plan;
    const GeomState& geom = c.geom;
    const ImageState& img = c.img;
    const r3dg_forward_outputs* out = c.out;
    RenderFwdArgs ra{};
    ra.records = geom.records;
    ra.ranges = img.ranges;
    ra.point_list = c.bin.point_list;
    ra.means2D = geom.means2D;
    ra.conic_opacity = geom.conic_opacity;
    ra.depths = geom.depths;
    ra.colors = c.g->colors_precomp ? c.g->colors_precomp : geom.rgb;
    ra.shader_colors = p.splat_active ? geom.shader_rgb : ra.colors;
    ra.features = c.feats;
    ra.bg = c.s->bg;
    ra.S = p.S; ra.W = p.W; ra.H = p.H; ra.grid_x = p.gx; ra.num_tiles = p.T;
    ra.cull = c.opt.test_no_cull ? 0 : 1;
    // forward: longest tiles first, as the backward (round 6: render_fwd 0.507 -> 0.495 ms at M1,
    // profiles/r06/fwd_order_ab; rounds 2-4 measured the spatial order faster, before the fused sort)
    ra.tile_order = img.tile_order;
    ra.final_T = img.final_T;
    ra.n_contrib = img.n_contrib;
    ra.out_color = out->color;
    ra.out_opacity = out->opacity;
    ra.out_depth = out->depth;
    ra.out_feature = out->feature;
    ra.out_shader_color = out->shader_color;
    ra.flay = make_feature_layout(p.S, (long long)p.H * p.W, true);
    // default splat shaders leave every stencil value 0 (InitializeStencil, rasterizer_impl.cu:203-209):
    // the blend writes those zeros with its other outputs (no separate memset launch)
    ra.zero_stencil = p.splat_active ? nullptr : out->stencil;
    ra.contrib = c.bin.contrib;
    ra.pairs = p.fuse_sort ? c.bin.pairs : nullptr;  // fused depth sort (render_fwd_glds_kernel)
    ra.point_list_out = c.bin.point_list;
    ra.shader_rec = c.reg.shader_rec;
    ra.bwd_work = p.T > 0 ? img.bwd_work : nullptr;
    ra.bwd_rank = img.bwd_rank;
    ra.bwd_hist = img.bwd_hist;
    if (c.reg.sums && p.T > 0) {
        ra.zero_sums = reinterpret_cast<float4*>(c.reg.sums);
        ra.zero_n4 = (uint32_t)((size_t)p.sums.SRS * (size_t)p.P / 4);
        ra.zero_chunk = (ra.zero_n4 + (uint32_t)p.T - 1) / (uint32_t)p.T;
    }
    return ra;
}

// the blend, then the backward's tile order with the pseudo normals (or on its own)
static int stage_blend(ForwardCtx& c) {
    const ForwardPlan& p = c.plan;
    const r3dg_raster_settings* s = c.s;
    const ImageState& img = c.img;
    const r3dg_forward_outputs* out = c.out;
    hipStream_t st = c.st;
    const int T = p.T;
    {
        ProfScope ps(R3DG_PROF_RENDER_FWD, st);
        R3DG_CHECK_HIP(launch_render_forward(render_fwd_args(c), p.splat_active, st));
    }
    R3DG_CHECK_LAUNCH(s->debug, st);

    if (s->compute_pseudo_normal) {
        XyzNormalArgs xa{};
        xa.W = p.W; xa.H = p.H; xa.view = s->viewmatrix; xa.focal_x = p.focal_x; xa.focal_y = p.focal_y;
        xa.cx = s->cx; xa.cy = s->cy; xa.opacity = out->opacity; xa.depth = out->depth;
        xa.normal = out->normal; xa.xyz = out->surface_xyz;
        // kOrderSlices leading workgroups sort the backward's tile order (tile_order_by_work) meanwhile
        xa.num_tiles = T; xa.bwd_work = img.bwd_work; xa.bwd_rank = img.bwd_rank; xa.bwd_hist = img.bwd_hist;
        xa.bwd_order = T > 0 ? img.bwd_order : nullptr;
        xa.blocks_x = p.gx;
        hipLaunchKernelGGL(xyz_normal_kernel,
                           dim3((T > 0 ? kOrderSlices : 0) + p.gx * ((p.gy + kXyzRows - 1) / kXyzRows)), dim3(256),
                           0, st, xa);
        R3DG_CHECK_LAUNCH(s->debug, st);
    } else {
        const size_t img3 = sizeof(float) * 3 * (size_t)p.H * p.W;
        if (T > 0) R3DG_CHECK_HIP(launch_bwd_order(T, img.bwd_work, img.bwd_rank, img.bwd_hist, img.bwd_order, st));
        if (out->normal) R3DG_CHECK_HIP(hipMemsetAsync(out->normal, 0, img3, st));
        if (out->surface_xyz) R3DG_CHECK_HIP(hipMemsetAsync(out->surface_xyz, 0, img3, st));
    }
    return R3DG_OK;
}

// rasterizer_impl.cu:485-529: depth and stencil are rendered again (now with the splat
// shaders' stencils) and replace the blended depth, then the passes run in list order
static int stage_post_passes(ForwardCtx& c) {
    const ForwardPlan& p = c.plan;
    const r3dg_forward_outputs* out = c.out;
    if (p.post_ids.empty()) return R3DG_OK;
    R3DG_CHECK_HIP(launch_intermediate(intermediate_args(c), p.P, c.radii, c.st));
    R3DG_CHECK_LAUNCH(c.s->debug, c.st);
    PostArgs pp{};
    pp.W = p.W; pp.H = p.H; pp.sh_color = out->color; pp.opacity = out->opacity; pp.depth = out->depth;
    pp.stencil = out->stencil; pp.surface_xyz = out->surface_xyz; pp.pseudonormal = out->normal;
    pp.shader_color = out->shader_color; pp.features = p.S == 21 ? out->feature : nullptr;
    pp.shadow = p.shadow_tex;
    R3DG_CHECK_HIP(launch_post_passes(p.post_ids.data(), (int)p.post_ids.size(), pp, c.reg.blur_snapshot, c.st));
    R3DG_CHECK_LAUNCH(c.s->debug, c.st);
    return R3DG_OK;
}

extern "C" int r3dg_rasterize_gaussians_ex(const r3dg_raster_settings* s, const r3dg_gaussians* g,
                                           const r3dg_forward_outputs* out, r3dg_alloc_fn geom_alloc, void* geom_ctx,
                                           r3dg_alloc_fn binning_alloc, void* binning_ctx, r3dg_alloc_fn image_alloc,
                                           void* image_ctx, r3dg_alloc_fn scratch_alloc, void* scratch_ctx,
                                           int* num_rendered, r3dg_stream_t stream) {
    ForwardCtx c{};
    c.s = s; c.g = g; c.out = out; c.st = (hipStream_t)stream;
    c.opt = options();
    ForwardPlan& p = c.plan;
    if (int rc = plan_forward(s, g, out, num_rendered, scratch_alloc != nullptr, c.opt, p)) return rc;

    const ForwardRegions sizes = carve_forward(p, nullptr, nullptr);
    void* geom_base = geom_alloc(geom_ctx, sizes.geom_bytes);
    void* img_base = image_alloc(image_ctx, image_state_bytes(p.H, p.W, !p.use_scratch));
    void* scratch_base = p.use_scratch ? scratch_alloc(scratch_ctx, sizes.scratch_bytes) : nullptr;
    if (!geom_base || !img_base || (p.use_scratch && !scratch_base)) {
        set_error("rasterize_gaussians: state allocation failed");
        return R3DG_ERR_ALLOC;
    }
    c.reg = carve_forward(p, geom_base, scratch_base);
    c.geom = geom_state_from(geom_base, (size_t)p.P, p.S);
    c.img = carve_image((uintptr_t)img_base, p.H, p.W, nullptr, !p.use_scratch);
    if (p.use_scratch) c.img.bin_hist = c.reg.bin_hist;
    c.radii = out->radii ? out->radii : c.geom.internal_radii;

    int L = 0, rc = stage_sh_shaders(c);
    if (!rc) rc = stage_binning(c, binning_alloc, binning_ctx, &L);
    if (!rc) rc = stage_splat_shaders(c);
    if (!rc) rc = stage_blend(c);
    if (!rc) rc = stage_post_passes(c);
    if (rc) return rc;
    // the prepared sums (zeroed by the blend) are the first backward's on this state; none: forget the
    // address's earlier entry
    g_sums.note(geom_base, p.T > 0 ? c.reg.sums : nullptr, p.P, p.S, p.sums.SRS);
    *num_rendered = L;
    return R3DG_OK;
}

extern "C" int r3dg_state_view(int P, int H, int W, int L, void* geom, void* binning, void* image,
                               r3dg_binning_view* v) {
    R3DG_REQUIRE(v, "state_view: null");
    GeomState gs = geom_state_from(geom, (size_t)P);
    BinningState bs = binning_state_from(binning, (size_t)L);
    ImageState is = image_state_from(image, H, W);
    v->point_list = bs.point_list;
    v->ranges = reinterpret_cast<const uint32_t*>(is.ranges);
    v->point_offsets = gs.point_offsets;
    v->depths = gs.depths;
    v->means2D = reinterpret_cast<const float*>(gs.means2D);
    v->conic_opacity = reinterpret_cast<const float*>(gs.conic_opacity);
    v->rgb = gs.rgb;
    v->cov3D = gs.cov3D;
    v->clamped = gs.clamped;
    return R3DG_OK;
}

// ---- backward ---------------------------------------------------------------------------------------
struct BackwardStates {
    GeomState gs;
    BinningState bs;
    ImageState is;
    const int* radii;
    int gx, gy;
};

static RenderBwdArgs render_bwd_args(const r3dg_raster_settings* s, const r3dg_gaussians* g,
                                     const r3dg_backward_grads* gr, const BackwardStates& b, const SumsPlan& sp,
                                     float* rows, float* sums, int backward_geometry, const r3dg_options& opt) {
    const GeomState& gs = b.gs;
    RenderBwdArgs ba{};
    ba.records = gs.records;
    ba.ranges = b.is.ranges;
    ba.point_list = b.bs.point_list;
    ba.offsets = gs.point_offsets;
    ba.radii = b.radii;
    ba.means2D = gs.means2D;
    ba.conic_opacity = gs.conic_opacity;
    ba.depths = gs.depths;
    ba.colors = g->colors_precomp ? g->colors_precomp : gs.rgb;
    ba.features = g->features;
    ba.bg = s->bg;
    ba.final_T = b.is.final_T;
    ba.n_contrib = b.is.n_contrib;
    ba.dL_dpix = gr->dL_dout_color;
    const long long HW = (long long)s->H * s->W;
    for (int c = 0; c < 3; ++c) {
        ba.ca[c] = gr->color_hwc ? c : (int)(c * HW);
        ba.cm[c] = gr->color_hwc ? 3 : 1;
    }
    ba.dL_dpix_o = gr->dL_dout_opacity;
    ba.dL_dpix_d = gr->dL_dout_depth;
    ba.dL_dpix_f = gr->dL_dout_feature;
    ba.gflay = make_feature_layout(s->S, HW, gr->feature_native != 0);
    ba.S = s->S; ba.W = s->W; ba.H = s->H; ba.grid_x = b.gx; ba.grid_y = b.gy; ba.num_tiles = b.gx * b.gy;
    // most backward work first (the forward's visit counts); test_tile_order_spatial: the XCD-aware
    // spatial order (the instance-count and per-XCD-band orders measured and dropped)
    ba.tile_order = opt.test_tile_order_spatial ? nullptr : b.is.bwd_order;
    ba.cull = opt.test_no_cull ? 0 : 1;
    ba.variant_dpp = opt.test_bwd_dpp;
    ba.wterms = opt.test_bwd_wterms;
    ba.backward_geometry = backward_geometry;
    ba.RS = sp.RS;
    ba.rows = rows;
    ba.flags = reinterpret_cast<uint8_t*>(b.bs.flags);
    ba.contrib = b.bs.contrib;
    ba.sums_atomic = sp.atomic;
    ba.sums = sums;
    ba.SRS = sp.SRS;
    return ba;
}

static GatherBwdArgs gather_bwd_args(const r3dg_raster_settings* s, const r3dg_gaussians* g,
                                     const r3dg_backward_outputs* out, const BackwardStates& b, const SumsPlan& sp,
                                     float* rows, float* sums) {
    const GeomState& gs = b.gs;
    GatherBwdArgs ga{};
    ga.P = s->P; ga.D = s->D; ga.M = s->M; ga.S = s->S; ga.RS = sp.RS;
    ga.W = s->W; ga.H = s->H; ga.grid_x = b.gx; ga.grid_y = b.gy;
    ga.rows = rows;
    ga.sums = sums;
    ga.sums_moments = sp.atomic;
    ga.SRS = sp.SRS;
    ga.flags = b.bs.flags;
    ga.means2D = gs.means2D;
    ga.conic_opacity = gs.conic_opacity;
    ga.offsets = gs.point_offsets;
    ga.radii = b.radii;
    ga.means3D = g->means3D;
    ga.sh = g->sh;
    ga.clamped = gs.clamped;
    ga.scales = g->scales;
    ga.rotations = g->rotations;
    ga.scale_modifier = s->scale_modifier;
    ga.cov3D = g->cov3D_precomp ? g->cov3D_precomp : gs.cov3D;
    ga.view = s->viewmatrix;
    ga.proj = s->projmatrix;
    ga.campos = s->campos;
    ga.focal_x = s->W / (2.0f * s->tan_fovx);
    ga.focal_y = s->H / (2.0f * s->tan_fovy);
    ga.tan_fovx = s->tan_fovx;
    ga.tan_fovy = s->tan_fovy;
    ga.use_scales = (g->scales != nullptr && g->cov3D_precomp == nullptr);
    ga.dL_dmeans2D = out->dL_dmeans2D;
    ga.dL_dcolors = out->dL_dcolors;
    ga.dL_dopacity = out->dL_dopacity;
    ga.dL_dmeans3D = out->dL_dmeans3D;
    ga.dL_dfeatures = out->dL_dfeatures;
    ga.dL_dcov3D = out->dL_dcov3D;
    ga.dL_dsh = (s->M > 0) ? out->dL_dsh : nullptr;
    ga.dL_dscales = out->dL_dscales;
    ga.dL_drotations = out->dL_drotations;
    if (out->dense_stride > 0) {
        ga.ld_m3 = ga.ld_op = ga.ld_sc = ga.ld_rot = ga.ld_f = out->dense_stride;
    } else {
        ga.ld_m3 = 3; ga.ld_op = 1; ga.ld_sc = 3; ga.ld_rot = 4; ga.ld_f = s->S;
    }
    return ga;
}

extern "C" int r3dg_rasterize_gaussians_backward(const r3dg_raster_settings* s, const r3dg_gaussians* g,
                                                 const int* radii_in, const r3dg_backward_grads* gr, void* geom,
                                                 void* binning, void* image, int num_rendered,
                                                 int backward_geometry, r3dg_alloc_fn scratch_alloc,
                                                 void* scratch_ctx, const r3dg_backward_outputs* out,
                                                 r3dg_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    R3DG_REQUIRE(s && g && gr && out, "rasterize_gaussians_backward: null argument");
    R3DG_REQUIRE(s->struct_size == sizeof(r3dg_raster_settings),
                 "rasterize_gaussians_backward: settings->struct_size must be sizeof(r3dg_raster_settings) (ABI 2)");
    R3DG_REQUIRE(out->struct_size == sizeof(r3dg_backward_outputs),
                 "rasterize_gaussians_backward: out->struct_size must be sizeof(r3dg_backward_outputs) (ABI 2)");
    const r3dg_options opt = options();
    const int P = s->P, S = s->S, L = num_rendered;
    R3DG_REQUIRE(P >= 0 && L >= 0 && S >= 0 && S <= kMaxFeatures, "rasterize_gaussians_backward: invalid sizes");
    R3DG_REQUIRE(out->dense_stride == 0 || out->dense_stride == 11 + S,
                 "rasterize_gaussians_backward: dense_stride must be 0 or 11 + S");
    R3DG_REQUIRE(!g->sh || P == 0 || (s->D >= 0 && s->D <= 3 && (s->D + 1) * (s->D + 1) <= s->M && s->M <= 16),
                 "rasterize_gaussians_backward: SH degree must be 0..3 with (degree+1)^2 <= M <= 16 coefficients");
    if (P == 0) return R3DG_OK;
    BackwardStates b{};
    b.gx = (s->W + kTileX - 1) / kTileX;
    b.gy = (s->H + kTileY - 1) / kTileY;
    b.gs = geom_state_from(geom, (size_t)P, S);
    b.bs = binning_state_from(binning, (size_t)L);
    b.is = image_state_from(image, s->H, s->W);
    b.radii = radii_in ? radii_in : b.gs.internal_radii;
    const SumsPlan sp = plan_sums(P, S, L, opt);
    // the backward blend addresses partial rows with 32-bit offsets in float4 units
    R3DG_REQUIRE((size_t)sp.RS * (size_t)L < (1ull << 32), "rasterize_gaussians_backward: too many tile instances");
    R3DG_REQUIRE(sp.SRS >= atomic_sums_min_stride(S) && sp.SRS % 8 == 0,
                 "rasterize_gaussians_backward: sums row stride too small");

    // scratch: the partial rows, then the per-Gaussian sums unless the forward prepared them behind
    // this geometry state (PreparedSums; the forward's blend zeroed those, the others are zeroed here).
    // The rows' presence flags live in the binning state, zeroed here (rows reduction only: the atomic
    // flush has no flags, so the forward's scatter does not write the 4L bytes)
    float* prepared = sp.atomic ? g_sums.take(geom, P, S, sp.SRS) : nullptr;
    char* scratch = (char*)scratch_alloc(scratch_ctx, sp.row_bytes + (prepared ? 0 : sp.sum_bytes));
    if (!scratch) {
        set_error("rasterize_gaussians_backward: scratch allocation failed");
        return R3DG_ERR_ALLOC;
    }
    float* rows = L > 0 && !sp.atomic ? reinterpret_cast<float*>(scratch) : nullptr;
    float* sums = prepared ? prepared : reinterpret_cast<float*>(scratch + sp.row_bytes);
    if (sp.atomic && !prepared) {
        ProfScope ps(R3DG_PROF_ROW_SUM, st);
        R3DG_CHECK_HIP(hipMemsetAsync(sums, 0, sp.sum_bytes, st));
    }
    if (!sp.atomic && L > 0) R3DG_CHECK_HIP(hipMemsetAsync(b.bs.flags, 0, sizeof(uint32_t) * (size_t)L, st));

    if (L > 0) {  // the blend
        const RenderBwdArgs ba = render_bwd_args(s, g, gr, b, sp, rows, sums, backward_geometry, opt);
        {
            ProfScope ps(R3DG_PROF_RENDER_BWD, st);
            R3DG_CHECK_HIP(launch_render_backward(ba, st));
        }
        R3DG_CHECK_LAUNCH(s->debug, st);
    }
    // per-Gaussian phase over n_chunks 256-aligned ranges; chunk_done after each range's launch
    GatherBwdArgs ga = gather_bwd_args(s, g, out, b, sp, rows, sums);
    const int nchunks = std::max(1, std::min(out->n_chunks, (P + 255) / 256));
    const int per = ((P + nchunks - 1) / nchunks + 255) & ~255;
    for (int c = 0, g0 = 0; g0 < P; ++c, g0 += per) {
        ga.g_begin = g0;
        ga.g_end = std::min(P, g0 + per);
        if (!sp.atomic) {
            ProfScope ps(R3DG_PROF_ROW_SUM, st);
            R3DG_CHECK_HIP(launch_row_sum(ga, st));
        }
        {
            ProfScope ps(R3DG_PROF_GATHER_BWD, st);
            R3DG_CHECK_HIP(launch_gather_backward(ga, st));
        }
        R3DG_CHECK_LAUNCH(s->debug, st);
        if (out->chunk_done) out->chunk_done(out->chunk_ctx, c, ga.g_begin, ga.g_end);
    }
    return R3DG_OK;
}

extern "C" int r3dg_sh_color_grads(int P, int g0, int n, void* geom, const float* dL_dcolors, float* drgb,
                                   r3dg_stream_t stream) {
    R3DG_REQUIRE(P >= 0 && g0 >= 0 && n >= 0 && g0 + n <= P && geom && (n == 0 || (dL_dcolors && drgb)),
                 "sh_color_grads: invalid arguments");
    const GeomState gs = geom_state_from(geom, (size_t)P);
    R3DG_CHECK_HIP(launch_sh_color_grads(n, gs.clamped + g0, dL_dcolors + 3 * (size_t)g0, drgb, (hipStream_t)stream));
    return R3DG_OK;
}

extern "C" int r3dg_sh_grad_from_views(int g0, int n, int degree, int M, int N, const float* means3D,
                                       const float* campos, const float* drgb, float* dL_dsh, r3dg_stream_t stream) {
    R3DG_REQUIRE(g0 >= 0 && n >= 0 && N >= 1 && degree >= 0 && degree <= 3 && (degree + 1) * (degree + 1) <= M &&
                     M <= 16 && (n == 0 || (means3D && campos && drgb && dL_dsh)),
                 "sh_grad_from_views: invalid arguments (degree 0..3, (degree+1)^2 <= M <= 16)");
    R3DG_CHECK_HIP(launch_sh_grad_views(g0, n, degree, M, N, means3D, campos, drgb, dL_dsh, (hipStream_t)stream));
    return R3DG_OK;
}

extern "C" int r3dg_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                                 uint8_t* present, r3dg_stream_t stream) {
    (void)projmatrix;
    if (P <= 0) return R3DG_OK;
    hipLaunchKernelGGL(mark_visible_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, means3D,
                       viewmatrix, present);
    R3DG_CHECK_HIP(hipGetLastError());
    return R3DG_OK;
}

extern "C" int r3dg_profile_enable(int max_records) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (int k = 0; k < R3DG_PROF_KINDS; ++k) {
        for (int e = 0; e < 2; ++e) {
            for (hipEvent_t ev : g_prof.ev[k][e]) R3DG_CHECK_HIP(hipEventDestroy(ev));
            g_prof.ev[k][e].clear();
        }
        g_prof.n[k] = 0;
    }
    g_prof.max_records = max_records > 0 ? max_records : 0;
    for (int k = 0; k < R3DG_PROF_KINDS; ++k)
        for (int e = 0; e < 2; ++e) {
            g_prof.ev[k][e].resize(g_prof.max_records);
            for (auto& ev : g_prof.ev[k][e]) R3DG_CHECK_HIP(hipEventCreate(&ev));
        }
    return R3DG_OK;
}

extern "C" int r3dg_profile_read(int kernel, int* count, float* total_ms) {
    R3DG_REQUIRE(kernel >= 0 && kernel < R3DG_PROF_KINDS && count && total_ms, "profile_read: bad arguments");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    float sum = 0.f;
    const int n = g_prof.n[kernel];
    for (int i = 0; i < n; ++i) {
        R3DG_CHECK_HIP(hipEventSynchronize(g_prof.ev[kernel][1][i]));
        float ms = 0.f;
        R3DG_CHECK_HIP(hipEventElapsedTime(&ms, g_prof.ev[kernel][0][i], g_prof.ev[kernel][1][i]));
        sum += ms;
    }
    g_prof.n[kernel] = 0;
    *count = n;
    *total_ms = sum;
    return R3DG_OK;
}
