/*
 * r3dg_hip.h -- C ABI of the MI355X-native relightable Gaussian-splat rasterizer.
 *
 * This is the drop-in boundary. Every entry point here is the plain-pointer form of one
 * function of the reference's pybind module `r3dg_rasterization._C`
 * (reference: r3dg-rasterization/ext.cu:21-35). The torch binding
 * relightable3dgaussian_amd/csrc/torch_ext.cpp re-exports them under the reference's names
 * with the reference's argument order and return tuples. No torch types appear here: device
 * buffers are raw pointers, the stream is a hipStream_t passed as void*, and the three opaque
 * state buffers of the reference (geomBuffer / binningBuffer / imgBuffer,
 * rasterize_points.cu:104-111) are obtained through caller-supplied allocation callbacks, the
 * C form of the reference's std::function<char*(size_t)> resize functors
 * (rasterize_points.cu:31-37).
 *
 * Conventions (as in the reference):
 *   - all float data is fp32, contiguous, on the current device;
 *   - an absent optional tensor (reference: empty tensor -> nullptr) is passed as NULL;
 *   - view/proj matrices are the transposed 4x4 torch matrices of scene/cameras.py:63-79
 *     (element m[4*c + r] multiplies coordinate c for output r);
 *   - image outputs are HWC (rasterize_points.cu:94-101); the feature output uses the layout
 *     documented at r3dg_feature_groups().
 * All functions return R3DG_OK (0) or a negative error code; r3dg_last_error() has the text.
 */
#ifndef R3DG_HIP_H
#define R3DG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: r3dg_raster_settings and r3dg_backward_outputs start with struct_size; r3dg_options */
#define R3DG_ABI_VERSION 2

enum {
    R3DG_OK = 0,
    R3DG_ERR_ARG = -1,         /* shape / argument error (reference: AT_ERROR -> RuntimeError) */
    R3DG_ERR_HIP = -2,         /* HIP runtime or kernel launch failure */
    R3DG_ERR_UNSUPPORTED = -3, /* feature outside this build's scope (DESIGN.md "Scope") */
    R3DG_ERR_ALLOC = -4        /* an allocation callback returned NULL */
};

typedef void* r3dg_stream_t;                                 /* hipStream_t */
typedef void* (*r3dg_alloc_fn)(void* ctx, size_t nbytes);    /* returns device memory, >= 256-B aligned */

int r3dg_abi_version(void);
const char* r3dg_last_error(void);

/* ---- library options (process-wide) ----------------------------------------------------------
 * Extensible structs carry their own size as the first field: a caller sets
 * struct_size = sizeof(the struct) as its header declares it, and the library rejects (R3DG_ERR_ARG)
 * a struct_size it does not know, so a binding built against another version of this header, or one
 * that forgot to zero-initialise the struct, fails loudly instead of reading garbage.
 *
 * No option is read from the environment on a launch. The one supported runtime option, the
 * backward's second reduction stage, starts from R3DG_BWD_REDUCE=rows|atomic, read once when the
 * library is loaded (default atomic); every field can be changed with r3dg_set_options. The test_*
 * fields select cross-check, negative-test and experiment variants for the test suite and the
 * measurement tools; production callers leave them 0. */
enum { R3DG_REDUCE_ATOMIC = 0, R3DG_REDUCE_ROWS = 1 };
typedef struct r3dg_options {
    size_t struct_size;       /* sizeof(r3dg_options) */
    int bwd_reduce;           /* R3DG_REDUCE_ATOMIC: (instance, wave) rows added into per-Gaussian sums with
                                 atomics (default, fastest; last bits depend on arrival order, as the
                                 reference's per-pixel atomicAdd); R3DG_REDUCE_ROWS: partial rows summed in a
                                 fixed order, bitwise reproducible */
    int prof_sort_markers;    /* r3dg_profile_*: also time the binning / sort stages (marker events) */
    int test_bwd_dpp;         /* backward blend by the DPP-reduction cross-check kernel (rows reduction) */
    int test_bwd_wterms;      /* 0 default (w in two bf16 terms); 1 / 3 (S 9..11, atomic): one term, the
                                 inexact reduction the gradient bar must reject, or three (exact) */
    int test_no_cull;         /* blends without the exact per-quadrant cull (same results) */
    int test_bin_atomic;      /* the global-atomic binning (the fallback above the LDS binning's tiles) */
    int test_bin_blocks;      /* > 0: cap on the LDS binning's workgroups (experiments) */
    int test_tile_order_spatial; /* backward tiles in the XCD-aware spatial order, not longest first */
    int test_bwd_srs;         /* > 0: row stride (floats) of the atomic per-Gaussian sums, rounded up to a
                                 multiple of 8 and to at least the X part + the six f64 moments */
    int test_bvh_lanes;       /* > 0: lanes per ray of the BVH opacity tracer (1, 2, 4, .. 64) */
    int test_bvh_sort;        /* 0 auto (Morton-sorted rays from 256k); 1 off; 2 on */
    int test_bvh_split;       /* 1: the static subtree-split tracer instead of the shared-stack groups */
    int test_bin_one_pass;    /* 1: the one-pass binning scatter (per-(workgroup, tile) runs) instead of the
                                 two passes through tile buckets (same results after the depth sort) */
} r3dg_options;
int r3dg_get_options(r3dg_options* out);   /* out->struct_size must be set */
int r3dg_set_options(const r3dg_options* in);

/* Feature output layout (replaces forward.cu:537-558, DESIGN.md "Feature layout").
 * Writes the channel-group sizes for S channels into groups[] and returns their count.
 * A group of size n starting at channel c0 is stored as a [H*W, n] block at offset c0*H*W
 * of the flat feature output. S=21 reproduces the reference's 3 scalar planes + six [HW,3]
 * blocks exactly; S=11 (training) uses [1,1,3,3,3]; any other S is planar [S,H,W]. */
int r3dg_feature_groups(int S, int* groups);

/* ---- rasterizer (rasterize_points.cu:39-181, rasterizer_impl.cu:213-529) ------------------- */

typedef struct r3dg_raster_settings {
    size_t struct_size; /* sizeof(r3dg_raster_settings) (ABI 2; checked) */
    int P;  /* number of Gaussians (means3D.size(0)) */
    int S;  /* feature channels (features.size(1)) */
    int D;  /* active SH degree */
    int M;  /* SH coefficients per Gaussian (sh.size(1)), 0 if sh absent */
    int W, H;
    float tan_fovx, tan_fovy, cx, cy;
    float scale_modifier;
    float time, dt;
    int prefiltered;
    int compute_pseudo_normal; /* reference spelling: computer_pseudo_normal */
    int debug;                 /* synchronise and check after every launch */
    const float* bg;           /* [3] */
    const float* viewmatrix;   /* [16] */
    const float* viewmatrix_inv;
    const float* projmatrix;
    const float* projmatrix_inv;
    const float* campos;       /* [3] */
    int64_t sh_shader_manager;    /* handle from r3dg_preprocess_model, 0 = all ShDefault */
    int64_t splat_shader_manager; /* handle from r3dg_preprocess_model, 0 = all SplatDefault */
    int64_t texture_manager;      /* 0 = none */
    const int64_t* post_passes;   /* host array of post-process pass handles, run in order after the
                                     blend (FORWARD::RunPostProcessShaders, forward.cu:973-1047);
                                     a non-empty list re-renders depth + stencil first
                                     (rasterizer_impl.cu:485-502) */
    int n_post_passes;
} r3dg_raster_settings;

typedef struct r3dg_gaussians {
    const float* means3D;        /* [P,3] */
    const float* features;       /* [P,S] or NULL when S == 0 */
    const float* colors_precomp; /* [P,3] or NULL (exactly one of colors_precomp / sh) */
    const float* opacity;        /* [P,1] */
    const float* scales;         /* [P,3] or NULL (exactly one of scales+rotations / cov3D_precomp) */
    const float* rotations;      /* [P,4] or NULL */
    const float* cov3D_precomp;  /* [P,6] or NULL */
    const float* sh;             /* [P,M,3] or NULL */
} r3dg_gaussians;

typedef struct r3dg_forward_outputs {
    float* color;        /* [H,W,3] */
    float* opacity;      /* [H,W,1] */
    float* depth;        /* [H,W,1] */
    float* stencil;      /* [H,W,1] */
    float* feature;      /* [H,W,S] storage, layout per r3dg_feature_groups */
    float* shader_color; /* [H,W,3] */
    float* normal;       /* [H,W,3] pseudo normal (zero where undefined) */
    float* surface_xyz;  /* [H,W,3] */
    int* radii;          /* [P] */
} r3dg_forward_outputs;

/* RasterizeGaussiansCUDA (rasterize_points.cu:39-181). The image state buffer holds n_contrib
 * (int32 [H,W]) at byte offset r3dg_image_state_n_contrib_offset(H, W). */
int r3dg_rasterize_gaussians(const r3dg_raster_settings* settings, const r3dg_gaussians* g,
                             const r3dg_forward_outputs* out, r3dg_alloc_fn geom_alloc, void* geom_ctx,
                             r3dg_alloc_fn binning_alloc, void* binning_ctx, r3dg_alloc_fn image_alloc,
                             void* image_ctx, int* num_rendered, r3dg_stream_t stream);

/* r3dg_rasterize_gaussians with a scratch allocator, called once per call: the forward-only
 * transients -- the binning's per-workgroup tile counts (up to 8 MiB, [workgroups, tiles] u32, used
 * only until the instances are scattered) and, with non-default splat shaders or post passes, the
 * shader colour / intermediate-pass records (16 B * P * (record float4s - 2) + 16 B * P) -- come
 * from scratch_alloc, which may hand out stream-ordered memory the caller frees as soon as the call
 * returns (the torch binding passes the caching allocator), instead of the tails of the image and
 * geometry states, which live as long as the autograd context. scratch_alloc NULL =
 * r3dg_rasterize_gaussians. */
int r3dg_rasterize_gaussians_ex(const r3dg_raster_settings* settings, const r3dg_gaussians* g,
                                const r3dg_forward_outputs* out, r3dg_alloc_fn geom_alloc, void* geom_ctx,
                                r3dg_alloc_fn binning_alloc, void* binning_ctx, r3dg_alloc_fn image_alloc,
                                void* image_ctx, r3dg_alloc_fn scratch_alloc, void* scratch_ctx, int* num_rendered,
                                r3dg_stream_t stream);

size_t r3dg_image_state_n_contrib_offset(int H, int W);

/* Bytes of the geometry state buffer for P Gaussians with S features (S < 0: the S-independent
 * part every per-Gaussian accessor reads, i.e. without the render records). Lets a binding check
 * a caller-supplied geomBuffer before handing it to r3dg_sh_color_grads. */
size_t r3dg_geom_state_bytes(int P, int S);

/* Debug / parity accessors into the opaque state buffers (tile keys, sort order, ranges). */
typedef struct r3dg_binning_view {
    const uint32_t* point_list;   /* [L] Gaussian ids in sorted order (reference point_list); the
                                     reference's sort key of position i is tile << 32 | depth bits
                                     of point_list[i], with the tile given by ranges */
    const uint32_t* ranges;       /* [tiles,2] from the image buffer */
    const uint32_t* point_offsets;/* [P] inclusive scan of tiles touched */
    const float* depths;          /* [P] */
    const float* means2D;         /* [P,2] */
    const float* conic_opacity;   /* [P,4] */
    const float* rgb;             /* [P,3] */
    const float* cov3D;           /* [P,6] */
    const uint8_t* clamped;       /* [P] bit c = channel c clamped */
} r3dg_binning_view;
int r3dg_state_view(int P, int H, int W, int L, void* geom, void* binning, void* image, r3dg_binning_view* view);

typedef struct r3dg_backward_grads {
    const float* dL_dout_color;   /* colour gradient */
    int color_hwc;                /* 0: [3,H,W] planar (reference contract, rasterize_points.cu:214-215); 1: [H,W,3] */
    const float* dL_dout_opacity; /* [H*W] */
    const float* dL_dout_depth;   /* [H*W] */
    const float* dL_dout_feature; /* feature gradient */
    int feature_native;           /* 0: [S,H,W] planar (reference, backward.cu:470-471); 1: forward output layout */
} r3dg_backward_grads;

typedef struct r3dg_backward_outputs {
    size_t struct_size;   /* sizeof(r3dg_backward_outputs) (ABI 2; checked) */
    float* dL_dmeans2D;   /* [P,3] (x, y, depth) */
    float* dL_dcolors;    /* [P,3] */
    float* dL_dopacity;   /* [P,1] */
    float* dL_dmeans3D;   /* [P,3] */
    float* dL_dfeatures;  /* [P,S] */
    float* dL_dcov3D;     /* [P,6] */
    float* dL_dsh;        /* [P,M,3] (may be NULL when M == 0) */
    float* dL_dscales;    /* [P,3] */
    float* dL_drotations; /* [P,4] */
    /* Optional chunked delivery (zero-initialised: one chunk, no callback). The per-Gaussian phase
     * (partial-row sums, cov2D / projection / SH / cov3D backward) runs over n_chunks contiguous
     * Gaussian ranges, 256-aligned, in order; after the kernels of [g_begin, g_end) are enqueued
     * on the stream, chunk_done(chunk_ctx, chunk, g_begin, g_end) is called on the host, so the
     * caller can start exchanging that range's gradients (an RCCL all-reduce on another stream)
     * while the next range computes. Results do not depend on n_chunks. */
    int n_chunks;
    void (*chunk_done)(void* ctx, int chunk, int g_begin, int g_end);
    void* chunk_ctx;
    /* Optional packed layout of the dense per-Gaussian gradients (0: dL_dmeans3D [P,3],
     * dL_dopacity [P,1], dL_dscales [P,3], dL_drotations [P,4], dL_dfeatures [P,S] as above). The
     * value 11 + S (the only other one accepted) is the row stride, in floats, of all five: the
     * caller points them at the columns 0, 3, 4, 7 and 11 of one [P, 11 + S] array, so a Gaussian
     * range of the five is one contiguous span -- one collective per chunk for the view-parallel
     * exchange (relightable3dgaussian_amd/view_parallel.py). */
    int dense_stride;
} r3dg_backward_outputs;

/* RasterizeGaussiansBackwardCUDA (rasterize_points.cu:183-275). Every output element is written
 * (no pre-zeroing needed). With r3dg_options.bwd_reduce = R3DG_REDUCE_ROWS the per-Gaussian sums
 * have a fixed order and the result is bitwise reproducible; the default R3DG_REDUCE_ATOMIC adds
 * them with f32 atomics, so last bits depend on arrival order (as the reference's).
 *
 * Prepared sums: a forward with the default shaders and no post passes, under R3DG_REDUCE_ATOMIC,
 * stores the zeroed per-Gaussian sums behind the geometry state it returns. The first backward on
 * that state, at that address, consumes them; every other backward (a second one on the same
 * state, a state from another kind of forward, other options) zeroes its own scratch. A caller
 * that moves a geometry state to another address before the backward loses nothing but that
 * saving: the call takes the memset path. */
int r3dg_rasterize_gaussians_backward(const r3dg_raster_settings* settings, const r3dg_gaussians* g,
                                      const int* radii, const r3dg_backward_grads* grads, void* geom,
                                      void* binning, void* image, int num_rendered, int backward_geometry,
                                      r3dg_alloc_fn scratch_alloc, void* scratch_ctx,
                                      const r3dg_backward_outputs* out, r3dg_stream_t stream);

/* View-parallel SH-gradient exchange (relightable3dgaussian_amd/view_parallel.py). The SH part of
 * a view's gradient is rank-1 per Gaussian: dL/dsh[k][c] = Y_k(dir) * dRGB[c] with dir =
 * normalize(mean - campos) and dRGB the clamp-masked colour gradient (backward.cu:20-139). So
 * instead of all-reducing 3*M floats per Gaussian, ranks all-gather dRGB (3 floats) and every
 * rank rebuilds the sum over views.
 *   r3dg_sh_color_grads: dRGB of Gaussians [g0, g0 + n) of this view: dL_dcolors (the backward's
 *     output) with the channels whose SH colour the forward clamped at 0 zeroed (geom state).
 *   r3dg_sh_grad_from_views: dL_dsh rows [g0, g0 + n) = sum over the N views, in view order, of
 *     Y_k(normalize(mean - campos[v])) * drgb[v][i][c] for k < (degree+1)^2, 0 for k < M beyond;
 *     drgb is [N][n][3] (the views' dRGB of these Gaussians), campos [N][3]. */
int r3dg_sh_color_grads(int P, int g0, int n, void* geom, const float* dL_dcolors, float* drgb, r3dg_stream_t stream);
int r3dg_sh_grad_from_views(int g0, int n, int degree, int M, int N, const float* means3D, const float* campos,
                            const float* drgb, float* dL_dsh, r3dg_stream_t stream);

/* markVisible (rasterize_points.cu:277-295): present[i] = view-space z > 0.2 */
int r3dg_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                      uint8_t* present, r3dg_stream_t stream);

/* ---- render equation (render_equation.cu) ---------------------------------------------- */

typedef struct r3dg_brdf_inputs {
    int P, S_incident, S_direct, S_visibility, sample_num;
    const float* base_color;     /* [P,3] */
    const float* roughness;      /* [P,1] */
    const float* metallic;       /* [P,1] */
    const float* normals;        /* [P,3] */
    const float* viewdirs;       /* [P,3] */
    const float* incidents_shs;  /* [P,S_incident,3] */
    const float* direct_shs;     /* [1,S_direct,3] */
    const float* visibility_shs; /* [P,S_visibility,1] */
} r3dg_brdf_inputs;

/* RenderEquationForwardCUDA (render_equation.cu:688-726). rand_float [P,sample_num] is read
 * only when is_training (reference draws it with torch::rand at :708). */
int r3dg_render_equation_forward(const r3dg_brdf_inputs* in, int is_training, const float* rand_float,
                                 float* pbr, float* incident_dirs, float* diffuse_light, r3dg_stream_t stream);

/* RenderEquationForwardCUDA_complex (render_equation.cu:220-274), outputs in reference order. */
typedef struct r3dg_brdf_complex_outputs {
    float* pbr;                    /* [P,3] */
    float* incident_dirs;          /* [P,Ns,3] */
    float* incident_lights;        /* [P,Ns,3] */
    float* local_incident_lights;  /* [P,Ns,3] */
    float* global_incident_lights; /* [P,Ns,3] */
    float* incident_visibility;    /* [P,Ns,1] */
    float* diffuse_light;          /* [P,3] */
    float* local_diffuse_light;    /* [P,3] */
    float* accum;                  /* [P,1] */
    float* rgb_d;                  /* [P,3] */
    float* rgb_s;                  /* [P,3] */
} r3dg_brdf_complex_outputs;
int r3dg_render_equation_forward_complex(const r3dg_brdf_inputs* in, const r3dg_brdf_complex_outputs* out,
                                         r3dg_stream_t stream);

/* RenderEquationBackwardCUDA (render_equation.cu:494-547). Bug-compatible with the reference
 * kernel except that dL_ddirect_shs is reduced deterministically (the reference races). */
typedef struct r3dg_brdf_grads {
    float* dL_dbase_color;     /* [P,3] */
    float* dL_droughness;      /* [P,1] */
    float* dL_dmetallic;       /* [P,1] */
    float* dL_dnormals;        /* [P,3] */
    float* dL_dviewdirs;       /* [P,3] */
    float* dL_dincidents_shs;  /* [P,S_incident,3] */
    float* dL_ddirect_shs;     /* [1,S_direct,3] */
    float* dL_dvisibility_shs; /* [P,S_visibility,1] */
} r3dg_brdf_grads;
int r3dg_render_equation_backward(const r3dg_brdf_inputs* in, const float* incident_dirs, const float* dL_dpbr,
                                  const float* dL_ddiffuse_light, r3dg_alloc_fn scratch_alloc, void* scratch_ctx,
                                  const r3dg_brdf_grads* out, r3dg_stream_t stream);

/* ---- relighting render equation (gaussian_renderer/neilf_composite.py, scene/envmap.py) ------
 * The forward-only operator of the reference's relighting script: its Python render equation
 * (neilf_composite.py:241-334 with is_training=False, np.pi rather than the CUDA kernels' 3.14159),
 * with SH widths up to degree 4 (25 coefficients, utils/sh_utils.py:131-182), the global light from
 * nothing, the environment SH or a lat-long environment map, and the incident visibility from the
 * baked SH or from per-sample traced values. Added within ABI 2: nothing existing changes. */
enum { R3DG_LIGHT_NONE = 0, R3DG_LIGHT_SH = 1, R3DG_LIGHT_MAP = 2 };
typedef struct r3dg_relight_inputs {
    size_t struct_size;             /* sizeof(r3dg_relight_inputs); checked */
    r3dg_brdf_inputs brdf;          /* P, the three SH widths (each 0..25 here), sample_num >= 1, the tensors;
                                       direct_shs is read in R3DG_LIGHT_SH only, visibility_shs only without
                                       traced_visibility */
    int light_mode;                 /* R3DG_LIGHT_NONE: no global light (neilf_composite.py:267);
                                       _SH: max(sum + 0.5, 0) of direct_shs (:260-263);
                                       _MAP: the environment lookup below, unclamped (:265) */
    const float* envmap;            /* [env_h, env_w, 3] lat-long map (R3DG_LIGHT_MAP) */
    int env_h, env_w;
    const float* env_transform;     /* device [3,3] row-major light rotation (light.transform), or NULL */
    const float* traced_visibility; /* [P, sample_num] (pc._visibility_tracing, :121 / :274), or NULL for the
                                       baked clamp(sum + 0.5, 0, 1) of visibility_shs (:270-271) */
} r3dg_relight_inputs;

/* Replaces the chunk loop over rendering_equation_python and the torch.cat of nine tensors
 * (neilf_composite.py:106-133). features is one row-major [P,21] array in the order of :129-133:
 * 0:3 rgb (:323-325), 3:6 normal, 6:9 base_color, 9 roughness, 10 metallic, 11:14 mean incident
 * light, 14:17 mean local light, 17:20 mean global light (after the visibility product, :278),
 * 20 mean visibility (:327-332); it is the rasterizer's S = 21 `features` as it stands.
 * R3DG_ERR_ARG before any device work: a wrong struct_size, a width above 25, R3DG_LIGHT_MAP without a
 * map or with env_h or env_w < 1, sample_num < 1 with P > 0. P = 0 returns at once. */
int r3dg_render_equation_relight(const r3dg_relight_inputs* in, float* features, r3dg_stream_t stream);

/* EnvLight.direct_light (scene/envmap.py:31-48) for n directions dirs [n,3] -> light [n,3]: d' = T d
 * when env_transform is given, v = (d'.x, d'.z, -d'.y), tu = atan2(v.x, -v.z) / 2 pi + 0.5,
 * tv = acos(clamp(v.y, -1, 1)) / pi, then nvdiffrast's dr.texture(filter_mode='linear') with its
 * default boundary_mode='wrap' in both axes. The composite renderer's per-pixel background
 * (neilf_composite.py:215) and the lookup of R3DG_LIGHT_MAP above. A texel index is in range for
 * every direction, NaN and Inf included. */
int r3dg_envmap_direct_light(int n, const float* dirs, const float* envmap, int env_h, int env_w,
                             const float* env_transform, float* light, r3dg_stream_t stream);

/* ---- shader manager (shaderManager.cu, preprocessModel.cu, ShShader.cu, splatShader.cu) ---- */

enum { R3DG_SHADER_SH = 0, R3DG_SHADER_SPLAT = 1, R3DG_SHADER_POST = 2 };
/* Name -> handle maps (GetShShaderAddressMap & co., ShShader.cu:196-230, splatShader.cu:283-333,
 * postProcessShader.cu). Handles are opaque shader ids, not device function pointers. */
int r3dg_shader_count(int kind);
const char* r3dg_shader_name(int kind, int index);
int64_t r3dg_shader_handle(int kind, int index);

/* PreprocessModel (preprocessModel.cu:156-213): assigns SH and splat shaders by position
 * (SelectShadersCUDA, :17-59) and buckets splat indices per shader. Returns two manager
 * handles (host objects owning device index lists). */
int r3dg_preprocess_model(int P, const float* xyz, int64_t* sh_manager, int64_t* splat_manager,
                          r3dg_stream_t stream);
/* Build a manager from explicit per-splat shader handles (host array [P]); the GPU-bucketing
 * half of PreprocessModel without the position rules. */
int r3dg_create_shader_manager(int kind, int P, const int64_t* shader_handles_host, int64_t* manager,
                               r3dg_stream_t stream);
int r3dg_shader_manager_info(int64_t manager, int* n_shaders, int64_t* handles, int* instance_counts);

/* ---- profiling ------------------------------------------------------------------------------ */
/* When enabled, HIP events are recorded on the caller's stream immediately before and after the
 * tile-blend kernels (the roofline kernels of DESIGN.md), up to max_records launches each.
 * r3dg_profile_read synchronises on the recorded events, returns the launch count and summed
 * device time in ms for one kernel, and resets that kernel's records. */
enum { R3DG_PROF_RENDER_FWD = 0, R3DG_PROF_RENDER_BWD = 1, R3DG_PROF_GATHER_BWD = 2, R3DG_PROF_SORT = 3,
       R3DG_PROF_PREPROCESS = 4, R3DG_PROF_ROW_SUM = 5, R3DG_PROF_KINDS = 6 };
int r3dg_profile_enable(int max_records);
int r3dg_profile_read(int kernel, int* count, float* total_ms);

/* Texture mode helpers (utils/texture.cu EncodeTextureMode / EncodeWrapMode). */
/* ---- textures (utils/texture.cu, asset_processing/textureImport.py) ----------------------- */
/* AllocateTexture (texture.cu:86-101,103-226): a texture from a device pixel array [H, W, C],
 * C the channel count of the PIL mode `mode` (r3dg_encode_texture_mode: 1 for 1/L/P/I/F, 3 for
 * RGB/YCbCr/LAB/HSV, 4 for RGBA/CMYK). Stored as float4 texels (3-channel modes get alpha 1 as
 * CreatPaddedArrayFromBase does) and sampled in software with the CUDA texture rules: wrap_u/v
 * from r3dg_encode_wrap_mode, normalized or texel coordinates, bilinear filtering with 8-bit
 * fractional weights (point sampling for LAB/HSV). Returns an opaque handle. */
int r3dg_texture_create(const float* pixels, int width, int height, int mode, int wrap_u, int wrap_v,
                        int normalized, int64_t* texture, r3dg_stream_t stream);
/* UploadTexturesToDevice (texture.cu:237-246): named textures + the error texture a shader gets
 * for a missing name (TextureManager::GetTexture, texture.cu:298-314). Shaders resolve their
 * texture names against it at launch. */
int r3dg_texture_manager_create(int n, const char* const* names, const int64_t* textures, int64_t error_texture,
                                int64_t* manager);
int r3dg_encode_texture_mode(const char* mode);
int r3dg_encode_wrap_mode(const char* mode);

/* ---- training step on the device -------------------------------------
 * The reference keeps one nn.Parameter per attribute group and steps them with torch.optim.Adam
 * (scene/gaussian_model.py:581-620); densification edits every group and the Adam states with
 * boolean-mask indexing and torch.cat (gaussian_model.py:795-1062). Here all groups of one model
 * live in ONE flat fp32 buffer: group g is a [P, width[g]] block starting at P * sum(width[<g])
 * (the layout below), with exp_avg / exp_avg_sq buffers of the same layout. */
#define R3DG_MAX_GROUPS 16
typedef struct r3dg_param_layout {
    int P;                        /* Gaussians */
    int n_groups;                 /* <= R3DG_MAX_GROUPS */
    int width[R3DG_MAX_GROUPS];   /* floats per Gaussian of each group */
    int xyz, scaling, rotation, opacity; /* group index of these roles (scaling / opacity raw,
                                             i.e. before exp / sigmoid as the reference stores them) */
} r3dg_param_layout;

/* One torch.optim.Adam step (gaussian_model.py:615-620 `step`, lr per param group) over the
 * flat elements [lo, hi) of `param` (global indices; a rank of the sharded optimizer passes its
 * shard). grad, exp_avg, exp_avg_sq are shard-local arrays of hi - lo floats. lr_host[g] is group
 * g's learning rate; step is Adam's 1-based step count. Arithmetic as torch's Adam:
 * m = lerp(m, g, 1 - b1); v = b2 v + (1 - b2) g^2; p += -(lr / (1 - b1^t)) m / (sqrt(v) /
 * sqrt(1 - b2^t) + eps), the bias corrections in double on the host. */
int r3dg_adam_step(const r3dg_param_layout* layout, float* param, const float* grad, float* exp_avg,
                   float* exp_avg_sq, int64_t lo, int64_t hi, const float* lr_host, double beta1, double beta2,
                   double eps, int step, r3dg_stream_t stream);

/* r3dg_adam_step with one Adam step count per group (torch keeps `state['step']` per parameter):
 * steps_host[g] is group g's 1-based count for this step, or <= 0 when the group has no gradient
 * this iteration -- torch.optim.Adam skips a parameter whose .grad is None (gaussian_model.py:615-617
 * zero_grad(set_to_none=True)), so its param, exp_avg and exp_avg_sq stay untouched. */
int r3dg_adam_step_groups(const r3dg_param_layout* layout, float* param, const float* grad, float* exp_avg,
                          float* exp_avg_sq, int64_t lo, int64_t hi, const float* lr_host, const int* steps_host,
                          double beta1, double beta2, double eps, r3dg_stream_t stream);

/* train.py:172-176 + add_densification_stats (gaussian_model.py:1055-1062) for the Gaussians
 * with radii > 0 (visibility_filter): max_radii2D = max(max_radii2D, radii); xyz_accum +=
 * |dL/dmeans2D[:, :2]| (rows of stride2d floats); normal_accum += |normalize(normal_grad, eps=1e-3)|
 * (skipped when normal_grad is NULL); denom += 1. */
int r3dg_densification_stats(int P, const float* dL_dmeans2D, int stride2d, const float* normal_grad,
                             const int* radii, float* xyz_accum, float* normal_accum, float* denom,
                             float* max_radii2D, r3dg_stream_t stream);

typedef struct r3dg_densify_args {
    float grad_threshold, grad_normal_threshold, percent_dense, extent, min_opacity;
    float max_screen_size; /* 0 = no screen/world size pruning (the reference's None) */
    int N;                 /* split children per Gaussian (2) */
    int prune_only;        /* 1: `prune` (gaussian_model.py:1045-1053), no clone / split */
} r3dg_densify_args;

/* densify_and_prune (gaussian_model.py:1025-1043; densify_and_clone :982-1023, densify_and_split
 * :926-980, prune_points :822-848, densification_postfix :880-924) or `prune` in one device pass
 * over the flat buffers. Result order is the reference's: surviving originals, then the clones,
 * then the split children (child k of every split Gaussian, k = 0..N-1). max_radii2D may be
 * NULL; as in the reference densify_and_prune's screen-size test never fires (the postfix has
 * zeroed max_radii2D), `prune` uses it. The split samples come from `randn`: called once with
 * n = 3 * N * n_split, it returns n standard-normal floats on the device (the reference draws
 * torch.normal(0, std)); the new buffers come from `alloc` (param, exp_avg, exp_avg_sq, each
 * P_new * sum(width) floats; clones and children get zero Adam state) and, when out_source is not
 * NULL, an int32 [P_new] map: the source Gaussian of each surviving original, -1 for new rows (the
 * caller slices its statistics with it, as prune_points does). counts = {originals kept, clones
 * kept, Gaussians split, children kept per k}. */
int r3dg_densify_and_prune(const r3dg_param_layout* layout, const float* param, const float* exp_avg,
                           const float* exp_avg_sq, const float* xyz_accum, const float* normal_accum,
                           const float* denom, const float* max_radii2D, const r3dg_densify_args* args,
                           r3dg_alloc_fn alloc, void* alloc_ctx, r3dg_alloc_fn randn, void* randn_ctx,
                           float** out_param, float** out_exp_avg, float** out_exp_avg_sq, int** out_source,
                           int* P_new, int* counts, r3dg_stream_t stream);

/* reset_opacity (gaussian_model.py:688-691): opacity = inverse_sigmoid(min(sigmoid(opacity), 0.01))
 * and the opacity group's Adam state zeroed (replace_tensor_to_optimizer). */
int r3dg_reset_opacity(const r3dg_param_layout* layout, float* param, float* exp_avg, float* exp_avg_sq,
                       r3dg_stream_t stream);

/* ---- parameter activations (scene/gaussian_model.py:23-44, 331-413, gaussian_renderer/neilf.py:102) ----
 * Everything between the flat parameter buffer and the per-Gaussian inputs of the rasterizer, the render
 * equation and the tracer, in at most two launches per direction. Forward, per Gaussian p (NULL output:
 * skipped):
 *   out_scaling [P,3] = expf(raw); out_rotation [P,4] = q / max(|q|, 1e-12); out_normal [P,3] = n /
 *   max(|n|, 1e-3); out_opacity [P,1], out_base_color [P,3], out_roughness [P,1], out_metallic [P,1] =
 *   1 / (1 + expf(-x)); out_shs [P,16,3], out_incidents [P,16,3], out_visibility [P,16,1]: row p of the dc
 *   group followed by row p of the rest group (copies); out_viewdirs [P,3] = v / max(|v|, 1e-12), v = campos -
 *   xyz; out_symm_inv [P,6] = get_inverse_covariance(): L = R(q^ / |q^|) diag(1 / s) of the activated q^, s
 *   (build_rotation's own normalisation included), the upper triangle of L L^T in strip_symmetric's order.
 * Every group of the layout must be named by exactly one role (xyz, scaling, rotation, opacity in the layout,
 * the others here) with the widths 3, 3, 4, 1, normal 3, f_dc 3, f_rest 45, base_color 3, roughness 1,
 * metallic 1, incidents_dc 3, incidents_rest 45, visibility_dc 1, visibility_rest 15; normal, f_dc and f_rest
 * are required, the seven others are present together or all absent (-1). */
typedef struct r3dg_activation_io {
    size_t struct_size;               /* sizeof(r3dg_activation_io); checked */
    const r3dg_param_layout* layout;
    int normal, f_dc, f_rest;         /* group index of each role */
    int base_color, roughness, metallic, incidents_dc, incidents_rest, visibility_dc, visibility_rest; /* or -1 */
    const float* campos;              /* device, 3 floats; NULL: no viewdirs */
    float *out_scaling, *out_rotation, *out_normal, *out_opacity, *out_shs;
    float *out_base_color, *out_roughness, *out_metallic, *out_incidents, *out_visibility;
    float* out_viewdirs;              /* needs campos */
    float* out_symm_inv;              /* forward only: it has no gradient */
} r3dg_activation_io;

/* R3DG_ERR_ARG before any device work: a wrong struct_size, a layout that breaks the rule above, a NULL
 * param with P > 0, out_viewdirs without campos. P == 0: R3DG_OK, nothing launched. No allocation, no
 * atomics, no host synchronisation; every launch is on stream. */
int r3dg_activate_forward(const r3dg_activation_io* io, const float* param, r3dg_stream_t stream);

/* One upstream gradient: row p starts at ptr + p * stride floats and is dense (stride >= the row's width,
 * so a column block of a wider row-major array passes as it is). ptr NULL: the gradient is zero. */
typedef struct r3dg_grad_rows {
    const float* ptr;
    int64_t stride;
} r3dg_grad_rows;

typedef struct r3dg_activation_grads {
    size_t struct_size;               /* sizeof(r3dg_activation_grads); checked */
    r3dg_grad_rows xyz, scaling, rotation, normal, opacity, shs;      /* widths 3, 3, 4, 3, 1, 48 */
    r3dg_grad_rows base_color, roughness, metallic, incidents, visibility; /* 3, 1, 1, 48, 16 */
    r3dg_grad_rows viewdirs;          /* 3; needs io->campos */
} r3dg_activation_grads;

/* The gradient of every group into `grad`, laid out as param. With r = |x|, y = x / r and upstream g:
 * normalise (normal eps 1e-3, rotation and viewdirs 1e-12): (g - y (y.g)) / r where r >= eps, else g / eps
 * (torch's clamp_min mask, decided on the float32 norm; a zero vector gets g / eps); exp: g * out; sigmoid:
 * g * s * (1 - s); the SH rows split into the dc and the rest row (copies); xyz: g_xyz - J(v)^T g_viewdirs.
 * Two of these are evaluated more exactly than the float32 reference evaluates them, so results differ from
 * it towards the exact value: the sigmoid slope s (1 - s) is computed as t / (1 + t)^2, t = expf(-|x|),
 * which does not cancel at large |x| (float32 autograd gives 0 at x = 20, this gives 2.1e-9 g); the
 * normalise projection, v = campos - xyz included, is computed in double from the float32 inputs and rounded
 * to float32 once (in float32 it loses all digits where g is nearly parallel to x). Everything is recomputed from
 * param: io's output pointers are not read, and param must be what the forward saw. accumulate == 0: every
 * element of grad[0, P * sum(width)) is written, zeros where the upstream is NULL, and nothing behind it;
 * accumulate != 0: the gradients are added to grad, and a NULL upstream leaves its group untouched.
 * R3DG_ERR_ARG before any device work: a wrong struct_size of either struct, what r3dg_activate_forward
 * refuses, a stride below the row's width, viewdirs without campos, an upstream of an absent role. */
int r3dg_activate_backward(const r3dg_activation_io* io, const float* param, const r3dg_activation_grads* grads,
                           float* grad, int accumulate, r3dg_stream_t stream);

/* ---- scene composition and the points capture (relighting.py:31-55, 89-123; scene/gaussian_model.py:237-262
 *      set_transform, :464-476 create_from_gaussians; utils/general_utils.py:105-149) -----------------------
 * A transform is 19 floats on the device, xform = M (4x4, row-major) followed by c (3), and a flag word that
 * says what of them applies. Vectors are columns: x' = M[:3,:3] x + M[:3,3].
 *   R3DG_XF_TRANSFORM (alone)  set_transform(transform=M): A = M[:3,:3], t = M[:3,3], s[i] = |row i of A|,
 *       R = A with row i divided by s[i], q_T = rotation_to_quaternion(R) = normalize((qw, (R21 - R12) / 4qw,
 *       (R02 - R20) / 4qw, (R10 - R01) / 4qw)), qw = sqrt(max(1 + R00 + R11 + R22, 1e-7)) / 2. Per Gaussian:
 *       scaling[j] <- expf(scaling[j]) * s[j] (the raw group stores its logf); xyz <- A xyz + t; normal <- R normal;
 *       rotation <- quaternion_multiply(q_T, rotation), not normalised. M's last row and c are not read,
 *       so the 16 floats of a 4x4 may be passed as they are.
 *   otherwise any of, applied in this order (the reference's):
 *   R3DG_XF_CENTER    xyz <- xyz - c
 *   R3DG_XF_ROTATION  R = M[:3,:3]: xyz <- R xyz, normal <- R normal, rotation <- q_R x rotation
 *   R3DG_XF_SCALE     s = M[3,0:3]: xyz <- xyz * s, scaling[j] <- expf(scaling[j]) * s[j]
 *   R3DG_XF_OFFSET    xyz <- xyz + M[:3,3]
 * s, R and the quaternion are uniform over a launch and computed in the kernel; every operation rounds on its
 * own, sums run left to right. The quaternion formula is ill-conditioned where 1 + trace(R) is small, as the
 * reference's is. The SH groups are NOT rotated (the reference rotates none either). flags == 0: no transform. */
#define R3DG_XF_TRANSFORM 1
#define R3DG_XF_CENTER 2
#define R3DG_XF_ROTATION 4
#define R3DG_XF_SCALE 8
#define R3DG_XF_OFFSET 16

/* set_transform in place on the flat parameter buffer, one launch: the groups layout->xyz, layout->scaling,
 * layout->rotation and `normal` (widths 3, 3, 4, 3) are rewritten (a group only when the flags touch it), every
 * other group, everything behind P * sum(width) and the Adam moments are not touched. Any number of groups
 * (7 or 14). R3DG_ERR_ARG before any device work: a bad layout, a role outside it or of the wrong width, unknown
 * flags, R3DG_XF_TRANSFORM with another flag, flags without xform. P == 0 or flags == 0: nothing launched. */
int r3dg_set_transform(const r3dg_param_layout* layout, int normal, float* param, const float* xform, int flags,
                       r3dg_stream_t stream);

/* The composite's arrays, each contiguous [P_total, ...] float32; an object writes rows [row, row + P). */
typedef struct r3dg_compose_out {
    size_t struct_size;  /* sizeof(r3dg_compose_out); checked */
    float *xyz;          /* [.,3]    moved */
    float *scaling;      /* [.,3]    expf(raw) * s: the reference's exp(log(exp(raw) * s)) within a few ulp */
    float *rotation;     /* [.,4]    (q_T x raw) / max(|.|, 1e-12) */
    float *normal;       /* [.,3]    (R raw) / max(|.|, 1e-3) */
    float *opacity, *base_color, *roughness, *metallic; /* [.,1] [.,3] [.,1] [.,1]  1 / (1 + expf(-raw)) */
    float *shs;          /* [.,16,3] row of f_dc, then row of f_rest */
    float *incidents;    /* [.,16,3] zeros (relighting.py:52-53) */
    float *visibility_dc;   /* [.,1,1]  raw copy */
    float *visibility_rest; /* [.,24,1] raw copy of the 15, then 9 zeros (relighting.py:46-50) */
    float *symm_inv;     /* [.,6]    get_inverse_covariance() of the moved Gaussian as r3dg_activate_forward
                                     computes it from the rotation and scaling above; NULL: skipped */
} r3dg_compose_out;

/* One object of scene_composition: reads the 14-group flat buffer `param` of io->layout (io names the roles as
 * for r3dg_activate_forward; its campos and output pointers are not read), applies the transform and the
 * activations with the device functions of r3dg_set_transform and r3dg_activate_forward, and writes rows
 * [row, row + P) of the composite. Two launches (the per-Gaussian groups; the wide SH rows as coalesced
 * copies); param is read-only and nothing else is allocated or written. The output row blocks may start at any
 * 4-byte-aligned address. R3DG_ERR_ARG before any device work: what r3dg_activate_forward refuses in io, a
 * 7-group layout, bad flags, a wrong struct_size, row < 0, a NULL array other than symm_inv (also with P == 0),
 * a NULL param with P > 0. P == 0: nothing launched. The caller guarantees row + P rows in every array. */
int r3dg_compose_object(const r3dg_activation_io* io, const float* param, const float* xform, int flags,
                        const r3dg_compose_out* out, int64_t row, r3dg_stream_t stream);

/* render_points (relighting.py:89-123), the z-buffered point cloud, without its loop. world_view is the
 * reference's transposed [4,4] (16 floats) and intrinsics [3,3] (9), both on the device. The background is bg,
 * 3 floats on the device, or, when bg is NULL, the 3 host floats bg_value, passed to the kernel by value (no
 * copy). Per point i:
 *   (xc, yc, z) = the first three components of [x, y, z, 1] @ world_view;  (uh, vh, wh) = K (xc, yc, z);
 *   u = uh / wh, v = vh / wh (wh is z bit for bit when K's last row is (0, 0, 1));
 *   dropped when u or v is not finite (this covers z == 0, where the reference's .long() is undefined);
 *   px = trunc(u), py = trunc(v), toward zero as .long(): a coordinate in (-1, 0) lands in column / row 0;
 *   a candidate when 0 <= px < W, 0 <= py < H and z < 10000 (the reference's initial depth, strict).
 * There is no near plane, as in the reference: a point behind the camera takes part with its negative z and
 * beats every point in front. Every pixel takes color[i] of its candidate with the smallest z, the smallest i
 * among bit-equal z (the reference's two scatters leave that case undefined), bg where it has none;
 * out_rgb is [3,H,W], out_depth (may be NULL) [H,W] with 10000 at empty pixels. Deterministic and
 * bit-reproducible. Scratch: H * W 64-bit keys (order-preserving bits of z : i) from scratch_alloc, cleared by
 * a memset; one pass of one global 64-bit atomic min per candidate (skipped when a plain load shows that the
 * key already loses); one resolve pass. No loop, no host synchronisation. H * W < 2^31. */
int r3dg_render_points(int P, const float* xyz, const float* color, const float* world_view,
                       const float* intrinsics, int H, int W, const float* bg, const float* bg_value, float* out_rgb,
                       float* out_depth, r3dg_alloc_fn scratch_alloc, void* scratch_ctx, r3dg_stream_t stream);

/* ---- BVH visibility tracer (reference module bvh_tracing._C,
 *      bvh/src/bindings.cpp:9-11) ------------------------------------------------------------
 * Tree layout (the reference's, bvh/__init__.py:31-37): nodes int32 [2P-1, 5] rows
 * {parent, left, right, gaussian, leaf count}, internal nodes 0..P-2, leaf P-1+i holds the i-th
 * Gaussian in Morton order; aabbs f32 [2P-1, 6] rows {lower xyz, upper xyz}; morton u64 [P]
 * sorted keys (30-bit Morton code << 31 | Gaussian index). */

/* RayTracer.__init__ leaf boxes (bvh/__init__.py:29-59): per Gaussian the min / max of the 8
 * corners mean ± 3 s_k R[:, k] (R = build_rotation of the re-normalised quaternion, r x y z),
 * written as [P, 6] rows to leaf_aabbs (pass aabbs + 6 (P - 1) to fill the tree's leaf rows). */
int r3dg_bvh_leaf_aabbs(int P, const float* means3D, const float* scales, const float* rotations,
                        float* leaf_aabbs, r3dg_stream_t stream);

/* create_bvh (bvh/src/bvh.cu:8-26, construct.cu:148-265): Karras LBVH over the leaf boxes in
 * aabbs rows P-1..2P-2 (input, in Gaussian order). Writes every field of nodes, the internal and
 * (Morton-sorted) leaf rows of aabbs, and morton. P >= 1. Scratch from scratch_alloc. */
int r3dg_bvh_build(int P, int32_t* nodes, float* aabbs, uint64_t* morton, r3dg_alloc_fn scratch_alloc,
                   void* scratch_ctx, r3dg_stream_t stream);

/* trace_bvh_opacity (bvh/src/bvh.cu:87-117, trace.cu:199-286): per ray the transmittance through
 * the Gaussians it meets (cov3D_inv: [P, 6] upper-triangular inverse covariance, the
 * get_inverse_covariance of gaussian_model.py:410-413). Outputs: num_contributes int32 [R],
 * rendered_opacity f32 [R] (0 and 0 once the transmittance drops below 0.9). num_gaussians = P of
 * the tree (2P-1 nodes); it bounds the traversal, so a malformed tree cannot hang the GPU.
 * Scratch from scratch_alloc: 128 B per Gaussian (packed node and Gaussian records), plus 16 B per
 * ray and a radix-sort workspace when the rays are traced in Morton order (>= 256k rays). */
int r3dg_bvh_trace_opacity(int num_rays, int num_gaussians, const int32_t* nodes, const float* aabbs, const float* rays_o,
                           const float* rays_d, const float* means3D, const float* cov3D_inv,
                           const float* opacities, const float* normals, int32_t* num_contributes,
                           float* rendered_opacity, r3dg_alloc_fn scratch_alloc, void* scratch_ctx,
                           r3dg_stream_t stream);

/* Rays that start at Gaussian centres, for r3dg_bvh_trace_opacity_centres: no origin array exists.
 * Ray r belongs to Gaussian g = index[r / sample_num] (g = r / sample_num when index is NULL, and
 * then num_rays == sample_num * num_gaussians); its origin is means3D[g]. Its direction is
 *   dirs != NULL: dirs[r], used as given (not normalised); with flip != 0 it is negated when
 *                 (d.x * n.x + d.y * n.y) + d.z * n.z < 0 for n = normals[g], the sum in float32 in
 *                 that order without contraction (a dot product of 0 does not flip): the call
 *                 sites' `rays_d[(rays_d * normal).sum(-1) < 0] *= -1`
 *   dirs == NULL: sample r % sample_num of fibonacci_sphere_sampling(normals[g], sample_num,
 *                 random_rotate=False) (utils/graphics_utils.py:9-37), r3dg_fibonacci_dirs' values
 * An index entry outside [0, num_gaussians) is the caller's error; it is not checked on the host (the
 * array is on the device). Nothing is read for such a ray and its outputs are NaN and -1. */
typedef struct r3dg_centre_rays {
    size_t struct_size;   /* sizeof(r3dg_centre_rays); checked */
    int num_rays;         /* R, a multiple of sample_num */
    int sample_num;       /* Ns >= 1 rays per index entry */
    const float* dirs;    /* [R, 3] or NULL (Fibonacci) */
    const int32_t* index; /* [R / Ns] or NULL */
    int flip;             /* given directions only */
} r3dg_centre_rays;

/* r3dg_bvh_trace_opacity for r3dg_centre_rays: the same traversal and outputs (rendered_opacity f32
 * [R], num_contributes int32 [R] or NULL when the caller has no use for it). Nothing proportional
 * to R is allocated: scratch is the 128 B per Gaussian of the packed records, plus, when the rays are
 * traced in Morton order (>= 256k rays), 16 B per index entry (R / Ns sort keys; slot s then traces
 * sample s % Ns of entry perm[s / Ns]) and the radix sort's workspace. R3DG_ERR_ARG: a wrong
 * struct_size, sample_num < 1, num_rays no multiple of sample_num, num_rays != sample_num *
 * num_gaussians without index. */
int r3dg_bvh_trace_opacity_centres(const r3dg_centre_rays* rays, int num_gaussians, const int32_t* nodes,
                                   const float* aabbs, const float* means3D, const float* cov3D_inv,
                                   const float* opacities, const float* normals, int32_t* num_contributes,
                                   float* rendered_opacity, r3dg_alloc_fn scratch_alloc, void* scratch_ctx,
                                   r3dg_stream_t stream);

/* fibonacci_sphere_sampling(normals, sample_num, random_rotate=False) as dirs [P, sample_num, 3] in one
 * launch: what sample_incident_rays(normals, False, sample_num) returns as directions. Each direction is
 * evaluated in double and rounded once, so it is the Fibonacci sample to float32 accuracy for every normal.
 * r3dg_render_equation_relight evaluates the same samples in float32 as the reference's tensor code does
 * (its sample angle is one rounded float32 product), which differs from these by up to 3e-5 rad at sample
 * 383, and by up to 1e-3 of the direction for a normal within 1e-3 of -z. */
int r3dg_fibonacci_dirs(int P, int sample_num, const float* normals, float* dirs, r3dg_stream_t stream);

/* ---- visibility baking (gaussian_renderer/neilf.py:323-348, scene/gaussian_model.py:428-462) ----
 * The L1 loss between traced visibility and the baked visibility SH. Per ray r of Gaussian
 * g = index[r] (g = r without index, then R == P): d = dirs[r], flipped as r3dg_centre_rays' flip when
 * normals is given; raw = eval_sh(sqrt(K) - 1, sh[g], d) in the operation order of
 * utils/sh_utils.py:71-128, sh[g] = {sh_dc[g], sh_rest[g][0..K-2]}; s = clamp(raw + 0.5, 0, 1);
 * term = |traced[r] - s|. K is 1, 4, 9, 16 or 25. An index entry outside [0, P) is the caller's error
 * (not checked on the host); the loss is then NaN and the row is left out of the gradient. */
typedef struct r3dg_visibility_sh_inputs {
    size_t struct_size;   /* sizeof(r3dg_visibility_sh_inputs); checked */
    int P, K, R;          /* Gaussians, coefficients per Gaussian, rays; P >= 1, R >= 1 */
    float* sh_dc;         /* [P, 1, 1] visibility_dc; written by r3dg_visibility_sh_fit_step only */
    float* sh_rest;       /* [P, K - 1, 1] visibility_rest (unused when K == 1); as sh_dc */
    const float* dirs;    /* [R, 3] */
    const float* traced;  /* [R] traced visibility */
    const float* normals; /* [P, 3], or NULL: no flip */
    const int32_t* index; /* [R], or NULL */
} r3dg_visibility_sh_inputs;

/* *loss (device) = mean over the rays of term. Deterministic: per-workgroup partial sums, added in a
 * fixed order in f64 by a finishing workgroup; scratch is 4 B per 256 rays. */
int r3dg_visibility_sh_loss_forward(const r3dg_visibility_sh_inputs* in, float* loss, r3dg_alloc_fn scratch_alloc,
                                    void* scratch_ctx, r3dg_stream_t stream);

/* Dense gradients grad_dc [P, 1, 1], grad_rest [P, K - 1, 1] of upstream * loss, every element written:
 * d/dsh_k = *upstream * sign(s - traced) * [0 <= raw + 0.5 <= 1] * basis_k(d) / R (sign(0) = 0, the clamp
 * bounds inclusive as torch's clamp backward), basis_k the factor of sh_k in eval_sh. upstream is a
 * device scalar. Rows that index does not name are zero; a row named more than once accumulates (float
 * atomics: reproducible bit for bit when the entries are distinct). */
int r3dg_visibility_sh_loss_backward(const r3dg_visibility_sh_inputs* in, const float* upstream, float* grad_dc,
                                     float* grad_rest, r3dg_stream_t stream);

/* The Adam state of the two SH tensors for r3dg_visibility_sh_fit_step, in their layouts. */
typedef struct r3dg_visibility_fit {
    size_t struct_size;   /* sizeof(r3dg_visibility_fit); checked */
    float* exp_avg_dc;    /* [P, 1, 1] */
    float* exp_avg_rest;  /* [P, K - 1, 1] */
    float* exp_avg_sq_dc;
    float* exp_avg_sq_rest;
    int step;             /* Adam's 1-based step count */
    float lr;
    double beta1, beta2, eps;
} r3dg_visibility_fit;

/* One iteration of finetune_visibility after its trace (gaussian_model.py:449-462), R == P and no index:
 * one launch computes the gradient above with upstream 1 and applies one torch.optim.Adam step (the
 * arithmetic of r3dg_adam_step) to the K coefficients of every Gaussian in place, a Gaussian with a zero
 * gradient included (its moments decay and it moves, as for zero entries of a present gradient); the same
 * launch leaves the loss partials, and *loss (device) is the mean L1 before the step. */
int r3dg_visibility_sh_fit_step(const r3dg_visibility_sh_inputs* in, const r3dg_visibility_fit* fit, float* loss,
                                r3dg_alloc_fn scratch_alloc, void* scratch_ctx, r3dg_stream_t stream);

/* trace_bvh (bvh/src/bvh.cu:28-85, trace.cu:8-196): per ray the Gaussians of every crossed
 * subtree of <= 4 leaves, sorted by (ray, t); num_contributes int32 [R] is their count per ray.
 * The three lists (int32 [L], f32 [L, 3], int32 [L]) come from alloc; *num_rendered = L (one
 * blocking device-to-host copy, as the reference). The reference's covs3D / opacities arguments
 * do not enter its arithmetic and are not taken here. */
int r3dg_bvh_trace(int num_rays, int num_gaussians, const int32_t* nodes, const float* aabbs, const float* rays_o,
                   const float* rays_d, const float* means3D, int32_t* num_contributes, r3dg_alloc_fn alloc,
                   void* alloc_ctx, int* num_rendered, int32_t** point_list, float** position_list,
                   int32_t** ray_id_list, r3dg_stream_t stream);

/* ---- nearest-neighbour distances (reference module simple_knn._C) --------------------------- */

/* distCUDA2 (submodules/simple-knn/spatial.cu:15-26, simple_knn.cu:185-221): mean squared distance
 * of every point to its three nearest other points, mean_dist2[i] = ((b0 + b1) + b2) / 3.0f with
 * b0 <= b1 <= b2 the three smallest d2(i, j) over j != i, d2 = (dx*dx + dy*dy) + dz*dz, d = p_j - p_i,
 * all in f32 without FMA contraction and an IEEE division. Exclusion is by index: a duplicate point
 * at distance 0 counts. A missing neighbour is FLT_MAX (P = 1, 2: +inf; P = 3: about FLT_MAX / 3).
 * The search is exact (boxes are pruned on a lower bound of d2 only), so the result is that of a
 * brute force and does not depend on the internal ordering. Inputs are expected finite; with NaN /
 * Inf coordinates the values are unspecified, but the call terminates and stays in bounds.
 * points f32 [P, 3], mean_dist2 f32 [P]. P < 0, a NULL points / mean_dist2 / scratch_alloc with
 * P > 0: R3DG_ERR_ARG; P == 0: R3DG_OK, nothing launched. Everything is enqueued on stream, with no
 * host synchronisation. Scratch from scratch_alloc: 32 B per point (two (code, index) pairs and the
 * Morton-ordered float4 copy), 32 B per 64 points (box bounds) and per 4096 points (super-box
 * bounds), and the radix sort's workspace. */
int r3dg_knn_mean_dist2(int P, const float* points /* [P,3] */, float* mean_dist2 /* [P] */,
                        r3dg_alloc_fn scratch_alloc, void* scratch_ctx, r3dg_stream_t stream);

/* ---- image loss (reference: utils/loss_utils.py, utils/image_utils.py) ----------------------- */

/* The L1 + SSIM loss of calculate_loss (gaussian_renderer/neilf.py:216-222) in fused form: ssim
 * (utils/loss_utils.py:31-62: 11x11 Gaussian window of sigma 1.5, zero padding 5, C1 = 0.01^2,
 * C2 = 0.03^2, all in f32), F.l1_loss and the squared error behind psnr (utils/image_utils.py:24-29).
 *
 * An image is `planes` (= batch * channels) independent [H, W] planes. Element (p, y, x) of img is
 * img[p * img_plane_stride + y * img_row_stride + x * img_px_stride] (strides in elements), gt
 * likewise: CHW is (H*W, W, 1), the rasterizer's HWC is (1, W*C, C).
 *
 * forward: sums f32 [planes, 3] = per plane the sums over its pixels of ssim_map, |img - gt| and
 * (img - gt)^2 (divide by H*W for the means). Tile partials are added in a fixed order in f64, so the
 * result is bitwise reproducible. dmaps: NULL (evaluation: nothing but sums is written) or f32
 * [3, planes, H, W] receiving per pixel the derivatives of ssim_map by mu1, by the window mean of
 * img^2 and by the window mean of img*gt, which the backward consumes. Scratch from scratch_alloc:
 * 12 B per 16x16 tile.
 *
 * backward: dL_dimg (addressed with img's strides) =
 *   scale[p] * (w_ssim[p] * d(sum of ssim_map over plane p)/d img + w_abs[p] * sign(img - gt)),
 * sign(0) = 0 as F.l1_loss differentiates. w_ssim, w_abs f32 [planes] and the optional scale f32
 * [planes] (NULL: 1) are device arrays; scale multiplies last, so a loss scaled by k gives
 * fl(k * gradient) exactly. There is no gradient with respect to gt.
 *
 * Negative planes / H / W, planes*H*W > INT32_MAX, a NULL required pointer or a NULL scratch_alloc:
 * R3DG_ERR_ARG before any device work. planes, H or W == 0: R3DG_OK, nothing launched or allocated.
 * Everything is enqueued on stream, with no host synchronisation. */
int r3dg_image_loss_forward(int planes, int H, int W, const float* img, int64_t img_plane_stride,
                            int64_t img_row_stride, int64_t img_px_stride, const float* gt,
                            int64_t gt_plane_stride, int64_t gt_row_stride, int64_t gt_px_stride,
                            float* sums /* [planes,3] */, float* dmaps /* [3,planes,H,W] or NULL */,
                            r3dg_alloc_fn scratch_alloc, void* scratch_ctx, r3dg_stream_t stream);
int r3dg_image_loss_backward(int planes, int H, int W, const float* img, int64_t img_plane_stride,
                             int64_t img_row_stride, int64_t img_px_stride, const float* gt,
                             int64_t gt_plane_stride, int64_t gt_row_stride, int64_t gt_px_stride,
                             const float* dmaps /* [3,planes,H,W] */, const float* w_ssim /* [planes] */,
                             const float* w_abs /* [planes] */, const float* scale /* [planes] or NULL */,
                             float* dL_dimg, r3dg_stream_t stream);
/* the 11 window weights the kernels use: gaussian(11, 1.5) of utils/loss_utils.py:19-21 in f32 (host memory) */
const float* r3dg_image_loss_window(void);

/* ---- image-space regularisers (reference: gaussian_renderer/neilf.py:233-321) ---------------- */

/* The eight image terms of calculate_loss beside L1 + SSIM, in fused form: one forward launch pair and
 * one backward launch for whichever are enabled. A map is n planes of [H, W]; element (c, y, x) is
 * ptr[c * plane_stride + y * row_stride + x * px_stride] (strides in elements): CHW is (H*W, W, 1), a
 * rasterizer feature group [H*W, n] is (1, W*n, n). Both run the same code and give the same bits.
 *
 * Rendered maps (differentiable): opacity 1, depth 1, normal 3, base_color 3, roughness 1, metallic 1
 * planes; pseudo_normal 3 (the reference detaches it: no gradient). Targets: gt_image 3, gt_depth 1,
 * image_mask 1 (ptr NULL: 1 everywhere, scene/cameras.py:55), mvs_normal 3. With m the mask value,
 * N = H * W and all arithmetic in f32 with the accurate expf / logf:
 *   DEPTH (neilf.py:233-241)  over the pixels where (m != 0) == (gt_depth > 0):
 *       sum |depth - gt_depth| / their count; no such pixel: 0 / 0 = NaN, as F.l1_loss of an empty
 *       selection, with an all-zero gradient. The count is an exact integer.
 *   MASK_ENTROPY (243-248)  o' = clamp(opacity, (float)1e-6, (float)(1 - 1e-6));
 *       -sum (m log o' + (1 - m) log(1 - o')) / N; gradient only where opacity is within the bounds
 *       (inclusive), as torch's clamp. A NaN opacity stays NaN through the clamp, as in torch: the term
 *       is NaN and that pixel's gradient 0.
 *   NORMAL_RENDER_DEPTH (250-256)  sum (normal m - pseudo_normal m)^2 / 3N.
 *   NORMAL_MVS_DEPTH (258-276)  the same with dm = (gt_depth > 0) and mvs_normal (the caller supplies
 *       mvs_normal; the kornia branch is not part of this).
 *   BASE_COLOR (285-303)  gm = gt_image m, v = max over channels of gm, w = 1 / (1 + exp(-5 (v - 0.5))),
 *       t = w gm^2 + (1 - w)(1 - (1 - gm)^2); sum |t - base_color| / 3N.
 *   BASE_COLOR_SMOOTH, METALLIC_SMOOTH, ROUGHNESS_SMOOTH (305-321; utils/loss_utils.py:65-96
 *       bilateral_smooth_loss)  G(x) = |Sobel_x| + |Sobel_y| of the channel mean of x with zero "same"
 *       padding; sum G(data) exp(-G(gt_image)) m / N. A 3x3 neighbourhood of equal means gives
 *       exactly 0 and no gradient.
 * sign(0) = 0 wherever torch has it (abs, l1_loss). The two normal terms add into one normal
 * gradient, the guide and the smoothness term into one base_color gradient.
 *
 * forward: values f32 [R3DG_REG_TERMS] = each enabled term's value (a disabled term's slot is 0),
 * depth_count int32 [1] = the depth term's selected pixels. Tile partials are added in a fixed order
 * in f64: two calls give the same bits. Scratch from scratch_alloc: 36 B per 16x16 tile.
 *
 * backward: for every map an enabled term reaches and whose pointer in `out` is not NULL, writes
 *   scale[0] * sum over its terms of weights[term] * d(term value)/d(map)
 * once (overwrite), addressed with that map's own strides. weights f32 [R3DG_REG_TERMS] and the
 * optional scale f32 [1] (NULL: 1) are device arrays: lambda and the upstream gradient, or their
 * product in weights. scale multiplies last, so a loss scaled by k gives fl(k * gradient) exactly.
 * depth_count is the forward's. Nothing is saved by the forward; both calls take the same inputs.
 *
 * Checked in this order, before any device work. (1) A NULL or wrongly sized struct (struct_size other
 * than sizeof as declared here), negative H / W, unknown bits in terms: R3DG_ERR_ARG. (2) H or W == 0,
 * or no term enabled: R3DG_OK, nothing launched or allocated, whatever the remaining arguments are (so
 * an image beyond int32 with no term enabled is R3DG_OK). (3) H*W > INT32_MAX, a NULL map that an
 * enabled term needs, a NULL values / depth_count / weights or a NULL scratch_alloc: R3DG_ERR_ARG.
 * Everything is enqueued on stream, with no host synchronisation. */
enum {
    R3DG_REG_DEPTH = 0,               /* tb_dict "loss_depth" */
    R3DG_REG_MASK_ENTROPY = 1,        /* "loss_mask_entropy" */
    R3DG_REG_NORMAL_RENDER_DEPTH = 2, /* "loss_normal_render_depth" */
    R3DG_REG_NORMAL_MVS_DEPTH = 3,    /* "loss_normal_mvs_depth" */
    R3DG_REG_BASE_COLOR = 4,          /* "loss_base_color" */
    R3DG_REG_BASE_COLOR_SMOOTH = 5,   /* "loss_base_color_smooth" */
    R3DG_REG_METALLIC_SMOOTH = 6,     /* "loss_metallic_smooth" */
    R3DG_REG_ROUGHNESS_SMOOTH = 7,    /* "loss_roughness_smooth" */
    R3DG_REG_TERMS = 8
};
typedef struct r3dg_map {
    const float* ptr; /* NULL: absent */
    int64_t plane_stride, row_stride, px_stride;
} r3dg_map;
typedef struct r3dg_reg_loss_inputs {
    size_t struct_size; /* sizeof(r3dg_reg_loss_inputs) (checked) */
    int H, W;
    unsigned terms;     /* bit (1 << R3DG_REG_*) set: the term is evaluated */
    r3dg_map opacity, depth, normal, pseudo_normal, base_color, roughness, metallic; /* rendered */
    r3dg_map gt_image, gt_depth, image_mask, mvs_normal;                             /* targets */
} r3dg_reg_loss_inputs;
typedef struct r3dg_reg_loss_grads {
    size_t struct_size; /* sizeof(r3dg_reg_loss_grads) (checked) */
    float *opacity, *depth, *normal, *base_color, *roughness, *metallic; /* NULL: not wanted */
} r3dg_reg_loss_grads;
int r3dg_reg_loss_forward(const r3dg_reg_loss_inputs* in, float* values /* [R3DG_REG_TERMS] */,
                          int32_t* depth_count /* [1] */, r3dg_alloc_fn scratch_alloc, void* scratch_ctx,
                          r3dg_stream_t stream);
int r3dg_reg_loss_backward(const r3dg_reg_loss_inputs* in, const int32_t* depth_count,
                           const float* weights /* [R3DG_REG_TERMS] */, const float* scale /* [1] or NULL */,
                           const r3dg_reg_loss_grads* out, r3dg_stream_t stream);

/* ---- PBR image head and light regulariser (reference: gaussian_renderer/neilf.py:169-175, 278-283) -- */

/* The composite over the background and the tone step between the rasterizer's feature output and the
 * image loss (neilf.py:169-175; scene/gamma_trans.py:45-51 hdr2ldr; the captures' composite of
 * relighting.py:225-229; the evaluation grid's clamp and the ACES hdr2ldr of
 * utils/graphics_utils.py:197-201), one launch:
 *   x = pbr + (1 - opacity) * bg      three float32 operations, each rounded on its own
 *   TONE_NONE   y = x
 *   TONE_GAMMA  y = clamp(x, lo, 1) ** gamma[0], lo = (float)1e-9, gamma a device float (never read on
 *               the host)
 *   TONE_ACES   s = x * 0.666667; y = (s (2.51 s + 0.03)) / (s (2.43 s + 0.59) + 0.14), the constants
 *               rounded to float32                                                    (forward only)
 *   TONE_CLAMP  y = clamp(x, 0, 1)                                                    (forward only)
 * A NaN x gives a NaN y in every mode, as torch.clamp passes it on. TONE_NONE and TONE_CLAMP use exactly
 * rounded operations only: their y is torch's bit for bit.
 *
 * All maps are dense: LAYOUT_HWC is pixel-major, pbr [H*W, 3] (the rasterizer's block as it is: no
 * alignment beyond 4 bytes is assumed) and opacity [H*W]; LAYOUT_CHW is planar, pbr [3, H*W] and opacity
 * [H*W]. bg is 3 floats, or with bg_per_pixel != 0 an image in pbr's shape and layout (the environment
 * behind the object). image, dL_dimage and dL_dpbr have pbr's shape and layout, dL_dopacity opacity's.
 * The layout flag fixes every address, so there are no strides.
 *
 * backward (TONE_NONE or TONE_GAMMA), with G = dL_dimage and xc the clamped x:
 *   dL/dx = G                                   TONE_NONE
 *   dL/dx = G * gamma * xc ** (gamma - 1)       TONE_GAMMA where lo <= x <= 1 (bounds included), else 0
 *   dL_dpbr = dL/dx;  dL_dopacity = -sum_c dL/dx_c * bg_c;  bg gets no gradient
 *   dL_dgamma [1] = sum over all elements of G * y * ln(xc), clamped elements included (ln(lo) at lo, 0
 *   at 1), from per-workgroup partial sums added in a fixed order in f64 by a second small launch: two
 *   runs give the same bits. No float atomics.
 * Each of dL_dpbr, dL_dopacity, dL_dgamma may be NULL (not wanted; all three NULL: R3DG_OK, nothing
 * launched). Nothing is saved by the forward: both calls take the same inputs; TONE_NONE reads neither
 * pbr, opacity nor gamma (they may be NULL). Launches: forward 1, backward 1, or 2 with dL_dgamma.
 * Scratch from scratch_alloc (only with dL_dgamma): 8 B per 1024 pixels.
 *
 * Checked before any device work, R3DG_ERR_ARG: an unknown layout or tone (backward: a forward-only
 * tone), H or W < 1, H*W > INT32_MAX, a NULL required pointer, dL_dgamma without TONE_GAMMA, dL_dgamma
 * with a NULL scratch_alloc. Everything is enqueued on stream, with no host synchronisation. */
enum { R3DG_PBR_TONE_NONE = 0, R3DG_PBR_TONE_GAMMA = 1, R3DG_PBR_TONE_ACES = 2, R3DG_PBR_TONE_CLAMP = 3 };
enum { R3DG_PBR_LAYOUT_CHW = 0, R3DG_PBR_LAYOUT_HWC = 1 };
int r3dg_pbr_head_forward(int H, int W, int layout, int tone, const float* pbr, const float* opacity,
                          const float* bg, int bg_per_pixel, const float* gamma /* [1] or NULL */,
                          float* image, r3dg_stream_t stream);
int r3dg_pbr_head_backward(int H, int W, int layout, int tone, const float* pbr, const float* opacity,
                           const float* bg, int bg_per_pixel, const float* gamma /* [1] or NULL */,
                           const float* dL_dimage, float* dL_dpbr, float* dL_dopacity,
                           float* dL_dgamma /* [1] */, r3dg_alloc_fn scratch_alloc, void* scratch_ctx,
                           r3dg_stream_t stream);

/* The lambda_light term of calculate_loss (neilf.py:278-283): with d = diffuse_light [P, 3] dense and m
 * the mean of a row's three channels,
 *   loss [1] = sum over the 3 P elements of |d_c - m| / (3 P).
 * The mean, the distances and their signs are evaluated in f64 from the float32 inputs, so a row of
 * equal channels contributes exactly 0; per-workgroup partial sums are added in a fixed order in f64 by
 * a second small launch and rounded once: two runs give the same bits. No float atomics. Scratch from
 * scratch_alloc: 8 B per 1024 rows.
 *
 * backward: with s_c = sign(d_c - m), sign(0) = 0,
 *   grad [P, 3] = upstream[0] * (s_c - (s_0 + s_1 + s_2) / 3) / (3 P),
 * dense, which is the dL_ddiffuse_light r3dg_render_equation_backward takes. upstream is a device
 * float. One launch.
 *
 * P < 0, a NULL pointer or a NULL scratch_alloc: R3DG_ERR_ARG before any device work. P == 0: R3DG_OK,
 * nothing launched, allocated or written. Everything is enqueued on stream, with no host
 * synchronisation. */
int r3dg_light_loss_forward(int P, const float* diffuse_light, float* loss /* [1] */,
                            r3dg_alloc_fn scratch_alloc, void* scratch_ctx, r3dg_stream_t stream);
int r3dg_light_loss_backward(int P, const float* diffuse_light, const float* upstream /* [1] */,
                             float* grad /* [P,3] */, r3dg_stream_t stream);

/* ---- display and capture head (gui.py:138-172, relighting.py:222-230 with torchvision's save_image,
 * train.py:243-272) and the environment background (neilf_composite.py:209-215, scene/cameras.py:87-99) ----
 * Added within ABI 2: nothing existing changes.
 *
 * r3dg_display_frame turns the rasterizer's buffers into the K images a frame shows or saves, out
 * [K, H*W, 3], in one launch. Per spec k and pixel, with s the source value (a one-channel source gives
 * three equal channels), o = opacity, b = bg, every operation float32 and rounded on its own:
 *   MODE_PLAIN        y = s
 *   MODE_OVER         y = s + (1 - o) * b                        relighting.py:229
 *   MODE_NORMAL_OVER  y = (s * 0.5 + 0.5) + (1 - o) * b          relighting.py:226-227
 *   MODE_NORMAL_MASK  y = s * 0.5 + 0.5 * o                      gui.py:167, train.py:249-250
 *   MODE_RANGE        y = (s - mn) / (mx - mn)                   gui.py:145, train.py:248; mn, mx the minimum
 *                     and maximum over every element of that spec's source; a NaN anywhere in the source
 *                     makes mn and mx NaN (torch.min / torch.max), so every y of the spec; mx == mn gives
 *                     what the division gives
 *   MODE_COUNT        y = (float)min(s, 1000) / 1000             gui.py:147; the source is int32
 * then the tone:  TONE_NONE y | TONE_CLAMP clamp(y, 0, 1), a NaN stays NaN | TONE_ACES the hdr2ldr of
 * r3dg_pbr_head_forward's TONE_ACES (the same device function),
 * then the encoding:
 *   ENC_F32  out is float32 and holds y
 *   ENC_U8   out is uint8 and holds floor(clamp(y * 255 + 0.5, 0, 255)) (save_image's
 *            mul(255).add_(0.5).clamp_(0, 255).to(uint8)); NaN gives 0 (the reference's cast of NaN is
 *            undefined)
 * Every mode but the ACES tone uses exactly rounded operations only: their out is torch's bit for bit.
 *
 * A source is dense: channels 1 ([H*W]) or 3; three channels are pixel-major [H*W, 3] with
 * R3DG_PBR_LAYOUT_HWC (the rasterizer's block as it is: no alignment beyond 4 bytes is assumed) or planar
 * [3, H*W] with R3DG_PBR_LAYOUT_CHW. opacity is [H*W], read by MODE_OVER, _NORMAL_OVER and _NORMAL_MASK, once
 * per pixel for all specs. bg is read by MODE_OVER and _NORMAL_OVER: BG_VECTOR 3 device floats, BG_IMAGE a
 * device [H*W, 3] image (r3dg_env_background's result), BG_HOST 3 HOST floats read during the call and passed
 * to the kernel by value.
 *
 * Launches: 1, plus 2 when any spec is MODE_RANGE, however many are: per-workgroup (min, max) partials of
 * all range specs, then one workgroup that finishes them into scratch the main kernel reads. Scratch from
 * scratch_alloc (only with MODE_RANGE): 128 B, and 12 B per 1024 elements of the largest range source for
 * every range spec. Min and max do not depend on
 * the order, so two runs give the same bits. Everything is enqueued on stream, with no host synchronisation.
 *
 * Checked before any device work, R3DG_ERR_ARG: H or W < 1, H*W > INT32_MAX, n_specs outside
 * 1..R3DG_DISPLAY_MAX_SPECS, a NULL specs, out or source, channels other than 1 or 3, an unknown layout,
 * mode, tone, encoding or bg_kind, a bg_kind other than BG_NONE with a NULL bg, a mode that reads opacity
 * or bg without it, MODE_RANGE with a NULL scratch_alloc. */
enum { R3DG_DISPLAY_MODE_PLAIN = 0, R3DG_DISPLAY_MODE_OVER = 1, R3DG_DISPLAY_MODE_NORMAL_OVER = 2,
       R3DG_DISPLAY_MODE_NORMAL_MASK = 3, R3DG_DISPLAY_MODE_RANGE = 4, R3DG_DISPLAY_MODE_COUNT = 5 };
enum { R3DG_DISPLAY_TONE_NONE = 0, R3DG_DISPLAY_TONE_CLAMP = 1, R3DG_DISPLAY_TONE_ACES = 2 };
enum { R3DG_DISPLAY_ENC_F32 = 0, R3DG_DISPLAY_ENC_U8 = 1 };
enum { R3DG_DISPLAY_BG_NONE = 0, R3DG_DISPLAY_BG_VECTOR = 1, R3DG_DISPLAY_BG_IMAGE = 2, R3DG_DISPLAY_BG_HOST = 3 };
#define R3DG_DISPLAY_MAX_SPECS 16
typedef struct r3dg_display_spec {
    const void* source; /* float32, or int32 with MODE_COUNT */
    int channels;       /* 1 or 3 */
    int layout;         /* R3DG_PBR_LAYOUT_HWC or _CHW (the same memory for one channel) */
    int mode;           /* R3DG_DISPLAY_MODE_* */
    int tone;           /* R3DG_DISPLAY_TONE_* */
} r3dg_display_spec;
int r3dg_display_frame(int H, int W, int n_specs, const r3dg_display_spec* specs, const float* opacity,
                       const float* bg, int bg_kind, int encoding, void* out /* [n_specs, H*W, 3] */,
                       r3dg_alloc_fn scratch_alloc, void* scratch_ctx, r3dg_stream_t stream);

/* The environment behind the object as an image, out [H*W, 3], in one launch and without a direction image:
 * per pixel (v, u), scene/cameras.py:91-97,
 *   d = F.normalize(((u - cx) / fx, (v - cy) / fy, 1)) (eps 1e-12), fx = K[0][0], fy = K[1][1], cx = K[0][2],
 *   cy = K[1][2] of intrinsics K, a device [3,3];  w = R d, R the rows c2w[i * c2w_stride + 0..2], i = 0..2, of
 *   the device camera-to-world matrix (c2w_stride 4 for a [4,4], 3 for a [3,3]),
 * then with R3DG_LIGHT_MAP r3dg_envmap_direct_light's lookup along w (the same device function, with
 * env_transform), or with R3DG_LIGHT_SH max(eval_sh(w) . env_shs + 0.5, 0) of env_shs [S, 3], S <= 25
 * (neilf_composite.py:212-213; the basis and the fused sum of r3dg_render_equation_relight's R3DG_LIGHT_SH,
 * the 0.5 added last as the reference writes it). Neither
 * matrix is read on the host. out is a valid BG_IMAGE of r3dg_display_frame and a per-pixel bg of
 * r3dg_pbr_head_forward (LAYOUT_HWC).
 * R3DG_ERR_ARG before any device work: H or W < 1, H*W > INT32_MAX, a NULL intrinsics, c2w or out, a
 * c2w_stride other than 3 or 4, a light_mode other than _SH or _MAP, _MAP without a map or with env_h or
 * env_w < 1, _SH with S outside 1..25 or a NULL env_shs. */
int r3dg_env_background(int H, int W, const float* intrinsics, const float* c2w, int c2w_stride, int light_mode,
                        const float* envmap, int env_h, int env_w, const float* env_transform,
                        const float* env_shs, int S, float* out, r3dg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* R3DG_HIP_H */
