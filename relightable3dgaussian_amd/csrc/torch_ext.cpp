// torch_ext.cpp -- pybind module `_C`: the reference operator surface over the C ABI.
//
// Mirrors r3dg_rasterization._C (reference r3dg-rasterization/ext.cu:21-35): the same 14
// function names, argument order and return tuples, so gaussian_renderer/neilf.py and
// scene/gaussian_model.py call it unchanged. Documented extensions:
//   (1) None / 0 shader-manager, texture and post-pass handles mean "defaults";
//   (2) every launch goes on the current HIP stream of means3D's device, and all buffers
//       (including the three state buffers) live on that device;
//   (3) extra entry points used by the shipped wrapper and the parity tests
//       (rasterize_gaussians_backward_ex, render_equation_forward_with_rand, rasterizer_state,
//       feature_groups, create_shader_manager, shader_manager_info).
// Errors from the C ABI surface as RuntimeError with the library's message.
#include <torch/extension.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <map>
#include <optional>
#include <string>
#include <tuple>
#include <vector>

#include "r3dg_hip.h"

namespace {

void check(int rc, const char* what) {
    if (rc != R3DG_OK) throw std::runtime_error(std::string(what) + ": " + r3dg_last_error());
}

// empty tensor (numel 0) means "absent", as the reference's data_ptr of an empty tensor
const float* opt_ptr(const torch::Tensor& t) { return t.numel() == 0 ? nullptr : t.data_ptr<float>(); }

// every entry point's inputs go to its first tensor's device, which must be a GPU: a host tensor
// is refused here, before its pointer could reach a kernel (there is no CPU path)
torch::Tensor dev_contig(const torch::Tensor& t, const torch::Device& dev) {
    TORCH_CHECK(dev.is_cuda(), "the HIP rasterizer takes tensors on a GPU device, got ", dev);
    if (t.numel() == 0) return t;
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, "expected a float32 tensor");
    return t.to(dev).contiguous();
}

struct TensorAlloc {
    torch::TensorOptions opts;
    torch::Tensor t;
};
void* tensor_alloc(void* ctx, size_t n) {
    auto* a = static_cast<TensorAlloc*>(ctx);
    a->t = torch::empty({(int64_t)std::max<size_t>(n, 256)}, a->opts);
    return a->t.data_ptr();
}

r3dg_stream_t stream_of(const torch::Device& dev) {
    return (r3dg_stream_t)c10::hip::getCurrentHIPStream(dev.index()).stream();
}

using FwdResult = std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
                             torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
                             torch::Tensor, torch::Tensor, torch::Tensor>;

// RasterizeGaussiansCUDA (rasterize_points.cu:39-181)
FwdResult rasterize_gaussians(const torch::Tensor& background, double time, double dt, const torch::Tensor& means3D,
                              const torch::Tensor& features, const torch::Tensor& colors,
                              const torch::Tensor& opacity, const torch::Tensor& scales,
                              const torch::Tensor& rotations, double scale_modifier,
                              const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                              const torch::Tensor& viewmatrix_inv, const torch::Tensor& projmatrix,
                              const torch::Tensor& projmatrix_inv, double tan_fovx, double tan_fovy, double cx,
                              double cy, int64_t image_height, int64_t image_width, const torch::Tensor& sh,
                              int64_t degree, const torch::Tensor& campos, bool prefiltered,
                              bool computer_pseudo_normal, std::optional<int64_t> d_textureManager_ptr,
                              std::optional<int64_t> h_shShaderManager_ptr,
                              std::optional<int64_t> h_splatShaderManager_ptr,
                              std::optional<std::vector<int64_t>> postProcessingPasses, bool debug) {
    if (means3D.ndimension() != 2 || means3D.size(1) != 3)
        throw std::runtime_error("means3D must have dimensions (num_points, 3)");
    TORCH_CHECK(means3D.is_cuda(), "means3D must be a GPU tensor (this build has no CPU path)");
    const torch::Device dev = means3D.device();
    const c10::OptionalDeviceGuard guard(dev);
    const int P = (int)means3D.size(0);
    const int S = features.numel() == 0 && features.dim() < 2 ? 0 : (int)features.size(1);
    const int H = (int)image_height, W = (int)image_width;
    auto fopt = means3D.options().dtype(torch::kFloat32);

    auto m3 = dev_contig(means3D, dev), ft = dev_contig(features, dev), co = dev_contig(colors, dev);
    auto op = dev_contig(opacity, dev), sc = dev_contig(scales, dev), ro = dev_contig(rotations, dev);
    auto c3 = dev_contig(cov3D_precomp, dev), shc = dev_contig(sh, dev), bg = dev_contig(background, dev);
    auto vm = dev_contig(viewmatrix, dev), vmi = dev_contig(viewmatrix_inv, dev);
    auto pm = dev_contig(projmatrix, dev), pmi = dev_contig(projmatrix_inv, dev), cp = dev_contig(campos, dev);

    torch::Tensor out_color = torch::empty({H, W, 3}, fopt);
    torch::Tensor out_opacity = torch::empty({H, W, 1}, fopt);
    torch::Tensor out_depth = torch::empty({H, W, 1}, fopt);
    torch::Tensor out_stencil = torch::empty({H, W, 1}, fopt);
    torch::Tensor out_feature = torch::empty({H, W, S}, fopt);
    torch::Tensor out_shader = torch::empty({H, W, 3}, fopt);
    torch::Tensor out_normal = torch::empty({H, W, 3}, fopt);
    torch::Tensor out_xyz = torch::empty({H, W, 3}, fopt);
    torch::Tensor radii = torch::empty({P}, means3D.options().dtype(torch::kInt32));

    auto bopt = torch::TensorOptions().dtype(torch::kUInt8).device(dev);
    TensorAlloc ga{bopt, torch::empty({0}, bopt)}, ba{bopt, torch::empty({0}, bopt)}, ia{bopt, torch::empty({0}, bopt)};

    std::vector<int64_t> passes = postProcessingPasses.value_or(std::vector<int64_t>{});
    r3dg_raster_settings s{};
    s.struct_size = sizeof(s);
    s.P = P; s.S = S; s.D = (int)degree; s.M = shc.numel() == 0 ? 0 : (int)shc.size(1);
    s.W = W; s.H = H;
    s.tan_fovx = (float)tan_fovx; s.tan_fovy = (float)tan_fovy; s.cx = (float)cx; s.cy = (float)cy;
    s.scale_modifier = (float)scale_modifier; s.time = (float)time; s.dt = (float)dt;
    s.prefiltered = prefiltered; s.compute_pseudo_normal = computer_pseudo_normal; s.debug = debug;
    s.bg = bg.data_ptr<float>();
    s.viewmatrix = vm.data_ptr<float>(); s.viewmatrix_inv = opt_ptr(vmi);
    s.projmatrix = pm.data_ptr<float>(); s.projmatrix_inv = opt_ptr(pmi);
    s.campos = cp.data_ptr<float>();
    s.sh_shader_manager = h_shShaderManager_ptr.value_or(0);
    s.splat_shader_manager = h_splatShaderManager_ptr.value_or(0);
    s.texture_manager = d_textureManager_ptr.value_or(0);
    s.post_passes = passes.data();
    s.n_post_passes = (int)passes.size();
    r3dg_gaussians g{};
    g.means3D = m3.data_ptr<float>(); g.features = opt_ptr(ft); g.colors_precomp = opt_ptr(co);
    g.opacity = opt_ptr(op); g.scales = opt_ptr(sc); g.rotations = opt_ptr(ro);
    g.cov3D_precomp = opt_ptr(c3); g.sh = opt_ptr(shc);
    r3dg_forward_outputs o{};
    o.color = out_color.data_ptr<float>(); o.opacity = out_opacity.data_ptr<float>();
    o.depth = out_depth.data_ptr<float>(); o.stencil = out_stencil.data_ptr<float>();
    o.feature = S > 0 ? out_feature.data_ptr<float>() : nullptr; o.shader_color = out_shader.data_ptr<float>();
    o.normal = out_normal.data_ptr<float>(); o.surface_xyz = out_xyz.data_ptr<float>();
    o.radii = P > 0 ? radii.data_ptr<int>() : nullptr;
    int rendered = 0;
    // the binning's tile counts: transient, returned to the caching allocator (stream-ordered) on exit
    TensorAlloc hist{bopt, torch::empty({0}, bopt)};
    check(r3dg_rasterize_gaussians_ex(&s, &g, &o, tensor_alloc, &ga, tensor_alloc, &ba, tensor_alloc, &ia, tensor_alloc,
                                      &hist, &rendered, stream_of(dev)),
          "rasterize_gaussians");
    // n_contrib is a view into the image state buffer (reference: from_blob, rasterize_points.cu:179)
    const int64_t off = (int64_t)r3dg_image_state_n_contrib_offset(H, W);
    torch::Tensor n_contrib = ia.t.narrow(0, off, (int64_t)H * W * 4).view(torch::kInt32).view({H, W, 1});
    return {rendered, n_contrib, out_color, out_opacity, out_depth, out_stencil, out_feature, out_shader,
            out_normal, out_xyz, radii, ga.t, ba.t, ia.t};
}

using BwdResult = std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
                             torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>;

BwdResult backward_impl(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& features,
                        const torch::Tensor& radii, const torch::Tensor& colors, const torch::Tensor& scales,
                        const torch::Tensor& rotations, double scale_modifier, const torch::Tensor& cov3D_precomp,
                        const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, double tan_fovx,
                        double tan_fovy, const torch::Tensor& dL_dout_color, const torch::Tensor& dL_dout_opacity,
                        const torch::Tensor& dL_dout_depth, const torch::Tensor& dL_dout_feature,
                        const torch::Tensor& sh, int64_t degree, const torch::Tensor& campos,
                        const torch::Tensor& geomBuffer, int64_t R, const torch::Tensor& binningBuffer,
                        const torch::Tensor& imageBuffer, bool backward_geometry, bool debug, int H, int W,
                        bool color_hwc, bool feature_native, int n_chunks = 1,
                        const py::object& chunk_cb = py::none(), bool packed_dense = false) {
    const torch::Device dev = means3D.device();
    const c10::OptionalDeviceGuard guard(dev);
    const int P = (int)means3D.size(0);
    const int S = features.numel() == 0 && features.dim() < 2 ? 0 : (int)features.size(1);
    const int M = sh.numel() == 0 ? 0 : (int)sh.size(1);
    auto fopt = means3D.options().dtype(torch::kFloat32);
    // packed_dense: the five dense gradients are column views of one [P, 11 + S] array (means3D 3,
    // opacity 1, scales 3, rotations 4, features S), so a Gaussian range of them is one contiguous
    // span (r3dg_backward_outputs.dense_stride; one collective per chunk in view_parallel.py)
    const int DW = 11 + S;
    torch::Tensor dense = packed_dense ? torch::empty({P, DW}, fopt) : torch::Tensor();
    torch::Tensor dL_dmeans3D = packed_dense ? dense.narrow(1, 0, 3) : torch::empty({P, 3}, fopt);
    torch::Tensor dL_dmeans2D = torch::empty({P, 3}, fopt);
    torch::Tensor dL_dfeatures = packed_dense ? dense.narrow(1, 11, S) : torch::empty({P, S}, fopt);
    torch::Tensor dL_dcolors = torch::empty({P, 3}, fopt);
    torch::Tensor dL_dopacity = packed_dense ? dense.narrow(1, 3, 1) : torch::empty({P, 1}, fopt);
    torch::Tensor dL_dcov3D = torch::empty({P, 6}, fopt);
    torch::Tensor dL_dsh = torch::empty({P, M, 3}, fopt);
    torch::Tensor dL_dscales = packed_dense ? dense.narrow(1, 4, 3) : torch::empty({P, 3}, fopt);
    torch::Tensor dL_drotations = packed_dense ? dense.narrow(1, 7, 4) : torch::empty({P, 4}, fopt);
    if (P == 0) return {dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dfeatures, dL_dcov3D, dL_dsh,
                        dL_dscales, dL_drotations};

    auto m3 = dev_contig(means3D, dev), ft = dev_contig(features, dev), co = dev_contig(colors, dev);
    auto sc = dev_contig(scales, dev), ro = dev_contig(rotations, dev), c3 = dev_contig(cov3D_precomp, dev);
    auto shc = dev_contig(sh, dev), bg = dev_contig(background, dev), vm = dev_contig(viewmatrix, dev);
    auto pm = dev_contig(projmatrix, dev), cp = dev_contig(campos, dev);
    auto gc = dev_contig(dL_dout_color, dev), go = dev_contig(dL_dout_opacity, dev);
    auto gd = dev_contig(dL_dout_depth, dev), gf = dev_contig(dL_dout_feature, dev);
    torch::Tensor rad = radii.to(dev).to(torch::kInt32).contiguous();

    r3dg_raster_settings s{};
    s.struct_size = sizeof(s);
    s.P = P; s.S = S; s.D = (int)degree; s.M = M; s.W = W; s.H = H;
    s.tan_fovx = (float)tan_fovx; s.tan_fovy = (float)tan_fovy; s.scale_modifier = (float)scale_modifier;
    s.debug = debug;
    s.bg = bg.data_ptr<float>(); s.viewmatrix = vm.data_ptr<float>(); s.projmatrix = pm.data_ptr<float>();
    s.campos = cp.data_ptr<float>();
    r3dg_gaussians g{};
    g.means3D = m3.data_ptr<float>(); g.features = opt_ptr(ft); g.colors_precomp = opt_ptr(co);
    g.scales = opt_ptr(sc); g.rotations = opt_ptr(ro); g.cov3D_precomp = opt_ptr(c3); g.sh = opt_ptr(shc);
    r3dg_backward_grads gr{};
    gr.dL_dout_color = gc.data_ptr<float>(); gr.color_hwc = color_hwc;
    gr.dL_dout_opacity = go.data_ptr<float>(); gr.dL_dout_depth = gd.data_ptr<float>();
    gr.dL_dout_feature = S > 0 ? gf.data_ptr<float>() : nullptr; gr.feature_native = feature_native;
    r3dg_backward_outputs o{};
    o.struct_size = sizeof(o);
    o.dL_dmeans2D = dL_dmeans2D.data_ptr<float>(); o.dL_dcolors = dL_dcolors.data_ptr<float>();
    o.dL_dopacity = dL_dopacity.data_ptr<float>(); o.dL_dmeans3D = dL_dmeans3D.data_ptr<float>();
    o.dL_dfeatures = S > 0 ? dL_dfeatures.data_ptr<float>() : nullptr; o.dL_dcov3D = dL_dcov3D.data_ptr<float>();
    o.dL_dsh = M > 0 ? dL_dsh.data_ptr<float>() : nullptr; o.dL_dscales = dL_dscales.data_ptr<float>();
    o.dL_drotations = dL_drotations.data_ptr<float>();
    o.dense_stride = packed_dense ? DW : 0;
    // chunked delivery: the Python callable runs (GIL held: we are inside the pybind call) after
    // each Gaussian range's kernels are enqueued; an exception is re-raised after the C call
    struct ChunkCtx {
        const py::object* cb;
        py::tuple outs;  // the 9 output tensors, handed to the callback
        bool failed = false;
        std::string what;
    } cctx{&chunk_cb, packed_dense ? py::make_tuple(dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dfeatures,
                                                    dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, dense)
                                   : py::make_tuple(dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dfeatures,
                                                    dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)};
    o.n_chunks = n_chunks;
    if (!chunk_cb.is_none()) {
        o.chunk_ctx = &cctx;
        o.chunk_done = [](void* ctx, int c, int g0, int g1) {
            auto* k = static_cast<ChunkCtx*>(ctx);
            if (k->failed) return;
            try {
                (*k->cb)(c, g0, g1, k->outs);
            } catch (const std::exception& e) {
                k->failed = true;
                k->what = e.what();
            }
        };
    }
    auto bopt = torch::TensorOptions().dtype(torch::kUInt8).device(dev);
    TensorAlloc scratch{bopt, torch::empty({0}, bopt)};
    check(r3dg_rasterize_gaussians_backward(&s, &g, rad.data_ptr<int>(), &gr, geomBuffer.data_ptr(),
                                            binningBuffer.data_ptr(), imageBuffer.data_ptr(), (int)R,
                                            backward_geometry, tensor_alloc, &scratch, &o, stream_of(dev)),
          "rasterize_gaussians_backward");
    TORCH_CHECK(!cctx.failed, "rasterize_gaussians_backward: chunk callback raised: ", cctx.what);
    return {dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dfeatures, dL_dcov3D, dL_dsh, dL_dscales,
            dL_drotations};
}

// RasterizeGaussiansBackwardCUDA (rasterize_points.cu:183-275): grads are CHW / planar.
BwdResult rasterize_gaussians_backward(const torch::Tensor& background, const torch::Tensor& means3D,
                                       const torch::Tensor& features, const torch::Tensor& radii,
                                       const torch::Tensor& colors, const torch::Tensor& scales,
                                       const torch::Tensor& rotations, double scale_modifier,
                                       const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                                       const torch::Tensor& projmatrix, double tan_fovx, double tan_fovy,
                                       const torch::Tensor& dL_dout_color, const torch::Tensor& dL_dout_opacity,
                                       const torch::Tensor& dL_dout_depth, const torch::Tensor& dL_dout_feature,
                                       const torch::Tensor& sh, int64_t degree, const torch::Tensor& campos,
                                       const torch::Tensor& geomBuffer, int64_t R, const torch::Tensor& binningBuffer,
                                       const torch::Tensor& imageBuffer, bool backward_geometry, bool debug) {
    const int H = (int)dL_dout_color.size(1), W = (int)dL_dout_color.size(2);
    return backward_impl(background, means3D, features, radii, colors, scales, rotations, scale_modifier,
                         cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_opacity,
                         dL_dout_depth, dL_dout_feature, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer,
                         backward_geometry, debug, H, W, false, false);
}

// Same, taking the forward's own output layouts (HWC colour, native feature layout): the
// shipped autograd wrapper uses this so no transposes are needed.
BwdResult rasterize_gaussians_backward_ex(const torch::Tensor& background, const torch::Tensor& means3D,
                                          const torch::Tensor& features, const torch::Tensor& radii,
                                          const torch::Tensor& colors, const torch::Tensor& scales,
                                          const torch::Tensor& rotations, double scale_modifier,
                                          const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                                          const torch::Tensor& projmatrix, double tan_fovx, double tan_fovy,
                                          const torch::Tensor& dL_dout_color, const torch::Tensor& dL_dout_opacity,
                                          const torch::Tensor& dL_dout_depth, const torch::Tensor& dL_dout_feature,
                                          const torch::Tensor& sh, int64_t degree, const torch::Tensor& campos,
                                          const torch::Tensor& geomBuffer, int64_t R,
                                          const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
                                          bool backward_geometry, bool debug, int64_t H, int64_t W) {
    return backward_impl(background, means3D, features, radii, colors, scales, rotations, scale_modifier,
                         cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_opacity,
                         dL_dout_depth, dL_dout_feature, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer,
                         backward_geometry, debug, (int)H, (int)W, true, true);
}

// rasterize_gaussians_backward_ex with chunked delivery (include/r3dg_hip.h r3dg_backward_outputs):
// chunk_cb(chunk, g_begin, g_end, outputs) is called once the gradients of Gaussians [g_begin,
// g_end) are enqueued (outputs = the 9 result tensors), e.g. to start their all-reduce on a
// communication stream (view_parallel.py).
BwdResult rasterize_gaussians_backward_chunked(
    const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& features,
    const torch::Tensor& radii, const torch::Tensor& colors, const torch::Tensor& scales,
    const torch::Tensor& rotations, double scale_modifier, const torch::Tensor& cov3D_precomp,
    const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, double tan_fovx, double tan_fovy,
    const torch::Tensor& dL_dout_color, const torch::Tensor& dL_dout_opacity, const torch::Tensor& dL_dout_depth,
    const torch::Tensor& dL_dout_feature, const torch::Tensor& sh, int64_t degree, const torch::Tensor& campos,
    const torch::Tensor& geomBuffer, int64_t R, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
    bool backward_geometry, bool debug, int64_t H, int64_t W, bool color_hwc, bool feature_native, int64_t n_chunks,
    const py::object& chunk_cb) {
    return backward_impl(background, means3D, features, radii, colors, scales, rotations, scale_modifier,
                         cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_opacity,
                         dL_dout_depth, dL_dout_feature, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer,
                         backward_geometry, debug, (int)H, (int)W, color_hwc, feature_native, (int)n_chunks, chunk_cb);
}

// rasterize_gaussians_backward_chunked with the dense gradients packed (packed_dense above): the
// callback's outputs carry a 10th tensor, the [P, 11 + S] array whose rows [g_begin, g_end) hold
// the chunk's means3D / opacity / scales / rotations / features gradients contiguously.
BwdResult rasterize_gaussians_backward_chunked_packed(
    const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& features,
    const torch::Tensor& radii, const torch::Tensor& colors, const torch::Tensor& scales,
    const torch::Tensor& rotations, double scale_modifier, const torch::Tensor& cov3D_precomp,
    const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, double tan_fovx, double tan_fovy,
    const torch::Tensor& dL_dout_color, const torch::Tensor& dL_dout_opacity, const torch::Tensor& dL_dout_depth,
    const torch::Tensor& dL_dout_feature, const torch::Tensor& sh, int64_t degree, const torch::Tensor& campos,
    const torch::Tensor& geomBuffer, int64_t R, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
    bool backward_geometry, bool debug, int64_t H, int64_t W, bool color_hwc, bool feature_native, int64_t n_chunks,
    const py::object& chunk_cb) {
    return backward_impl(background, means3D, features, radii, colors, scales, rotations, scale_modifier,
                         cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_opacity,
                         dL_dout_depth, dL_dout_feature, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer,
                         backward_geometry, debug, (int)H, (int)W, color_hwc, feature_native, (int)n_chunks, chunk_cb,
                         true);
}

// View-parallel SH-gradient exchange (include/r3dg_hip.h): this view's clamp-masked colour
// gradients of Gaussians [g0, g1) (the rank's all-gather payload) ...
torch::Tensor sh_color_grads(const torch::Tensor& geomBuffer, int64_t P, const torch::Tensor& dL_dcolors, int64_t g0,
                             int64_t g1) {
    const torch::Device dev = dL_dcolors.device();
    const c10::OptionalDeviceGuard guard(dev);
    TORCH_CHECK(dev.is_cuda() && dL_dcolors.is_contiguous() && dL_dcolors.scalar_type() == torch::kFloat32 &&
                    dL_dcolors.numel() == 3 * P && 0 <= g0 && g0 <= g1 && g1 <= P,
                "sh_color_grads: dL_dcolors must be a contiguous float32 CUDA [P,3] tensor, 0 <= g0 <= g1 <= P");
    TORCH_CHECK(geomBuffer.device() == dev && geomBuffer.is_contiguous() &&
                    (size_t)geomBuffer.nbytes() >= r3dg_geom_state_bytes((int)P, -1),
                "sh_color_grads: geomBuffer must be the forward's geometry state for these P Gaussians, on the "
                "gradients' device");
    auto out = torch::empty({g1 - g0, 3}, dL_dcolors.options());
    check(r3dg_sh_color_grads((int)P, (int)g0, (int)(g1 - g0), geomBuffer.data_ptr(), dL_dcolors.data_ptr<float>(),
                              out.data_ptr<float>(), stream_of(dev)),
          "sh_color_grads");
    return out;
}

// ... and the sum over the N views of their SH gradients, rebuilt from the gathered [N, n, 3]
// colour gradients and the views' camera centres [N, 3], into rows [g0, g0 + n) of dL_dsh.
void sh_grad_from_views(const torch::Tensor& means3D, const torch::Tensor& campos, const torch::Tensor& drgb,
                        int64_t degree, int64_t g0, torch::Tensor& dL_dsh) {
    const torch::Device dev = means3D.device();
    const c10::OptionalDeviceGuard guard(dev);
    TORCH_CHECK(drgb.dim() == 3 && drgb.size(2) == 3 && campos.dim() == 2 && campos.size(1) == 3 &&
                    campos.size(0) == drgb.size(0) && dL_dsh.dim() == 3 && dL_dsh.size(2) == 3 &&
                    dL_dsh.is_contiguous() && g0 >= 0 && g0 + drgb.size(1) <= dL_dsh.size(0),
                "sh_grad_from_views: drgb [N,n,3], campos [N,3], dL_dsh [P,M,3] contiguous");
    TORCH_CHECK(means3D.dim() == 2 && means3D.size(1) == 3 && means3D.size(0) >= g0 + drgb.size(1),
                "sh_grad_from_views: means3D must be [P,3] with P >= g0 + n");
    TORCH_CHECK(dL_dsh.device() == dev && dL_dsh.scalar_type() == torch::kFloat32 && dL_dsh.size(1) <= 16 &&
                    degree >= 0 && degree <= 3 && (degree + 1) * (degree + 1) <= dL_dsh.size(1),
                "sh_grad_from_views: dL_dsh must be a float32 [P,M,3] tensor on means3D's device, degree 0..3 with "
                "(degree+1)^2 <= M <= 16");
    auto m3 = dev_contig(means3D, dev), cp = dev_contig(campos, dev), d = dev_contig(drgb, dev);
    check(r3dg_sh_grad_from_views((int)g0, (int)drgb.size(1), (int)degree, (int)dL_dsh.size(1), (int)drgb.size(0),
                                  m3.data_ptr<float>(), cp.data_ptr<float>(), d.data_ptr<float>(),
                                  dL_dsh.data_ptr<float>(), stream_of(dev)),
          "sh_grad_from_views");
}

torch::Tensor mark_visible(torch::Tensor& means3D, torch::Tensor& viewmatrix, torch::Tensor& projmatrix) {
    const torch::Device dev = means3D.device();
    const c10::OptionalDeviceGuard guard(dev);
    const int P = (int)means3D.size(0);
    torch::Tensor present = torch::zeros({P}, means3D.options().dtype(torch::kBool));
    if (P == 0) return present;
    auto m3 = dev_contig(means3D, dev), vm = dev_contig(viewmatrix, dev), pm = dev_contig(projmatrix, dev);
    check(r3dg_mark_visible(P, m3.data_ptr<float>(), vm.data_ptr<float>(), pm.data_ptr<float>(),
                            (uint8_t*)present.data_ptr<bool>(), stream_of(dev)),
          "mark_visible");
    return present;
}

r3dg_brdf_inputs brdf_inputs(const std::vector<torch::Tensor>& t, int sample_num) {
    r3dg_brdf_inputs in{};
    in.P = (int)t[0].size(0);
    in.S_incident = (int)t[5].size(1);
    in.S_direct = (int)t[6].size(1);
    in.S_visibility = (int)t[7].size(1);
    in.sample_num = sample_num;
    in.base_color = t[0].data_ptr<float>(); in.roughness = t[1].data_ptr<float>();
    in.metallic = t[2].data_ptr<float>(); in.normals = t[3].data_ptr<float>();
    in.viewdirs = t[4].data_ptr<float>(); in.incidents_shs = t[5].data_ptr<float>();
    in.direct_shs = t[6].data_ptr<float>(); in.visibility_shs = t[7].data_ptr<float>();
    return in;
}

std::vector<torch::Tensor> prep_brdf(std::initializer_list<torch::Tensor> ts, const torch::Device& dev) {
    std::vector<torch::Tensor> r;
    for (const auto& t : ts) {
        TORCH_CHECK(t.scalar_type() == torch::kFloat32, "render_equation: expected float32 inputs");
        r.push_back(t.to(dev).contiguous());
    }
    return r;
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> render_equation_forward_impl(
    const std::vector<torch::Tensor>& t, int64_t sample_num, bool is_training, const torch::Tensor* rand_in) {
    const torch::Device dev = t[0].device();
    const int P = (int)t[0].size(0);
    auto fopt = t[0].options().dtype(torch::kFloat32);
    torch::Tensor pbr = torch::empty({P, 3}, fopt);
    torch::Tensor dirs = torch::empty({P, sample_num, 3}, fopt);
    torch::Tensor diffuse = torch::empty({P, 3}, fopt);
    // the reference always draws the per-(Gaussian, sample) rotation (render_equation.cu:708)
    torch::Tensor rnd = rand_in ? rand_in->to(dev).contiguous() : torch::rand({P, sample_num, 1}, fopt);
    r3dg_brdf_inputs in = brdf_inputs(t, (int)sample_num);
    check(r3dg_render_equation_forward(&in, is_training, rnd.numel() ? rnd.data_ptr<float>() : nullptr,
                                       pbr.data_ptr<float>(), dirs.data_ptr<float>(), diffuse.data_ptr<float>(),
                                       stream_of(dev)),
          "render_equation_forward");
    return {pbr, dirs, diffuse};
}

// RenderEquationForwardCUDA (render_equation.cu:688-726)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> render_equation_forward(
    const torch::Tensor& base_color, const torch::Tensor& roughness, const torch::Tensor& metallic,
    const torch::Tensor& normals, const torch::Tensor& viewdirs, const torch::Tensor& incidents_shs,
    const torch::Tensor& direct_shs, const torch::Tensor& visibility_shs, int64_t sample_num, bool is_training,
    bool debug) {
    (void)debug;
    const torch::Device dev = base_color.device();
    const c10::OptionalDeviceGuard guard(dev);
    auto t = prep_brdf({base_color, roughness, metallic, normals, viewdirs, incidents_shs, direct_shs, visibility_shs},
                       dev);
    return render_equation_forward_impl(t, sample_num, is_training, nullptr);
}

// test entry: explicit rotation randoms [P, sample_num(, 1)]
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> render_equation_forward_with_rand(
    const torch::Tensor& base_color, const torch::Tensor& roughness, const torch::Tensor& metallic,
    const torch::Tensor& normals, const torch::Tensor& viewdirs, const torch::Tensor& incidents_shs,
    const torch::Tensor& direct_shs, const torch::Tensor& visibility_shs, int64_t sample_num, bool is_training,
    const torch::Tensor& rand_float) {
    const torch::Device dev = base_color.device();
    const c10::OptionalDeviceGuard guard(dev);
    auto t = prep_brdf({base_color, roughness, metallic, normals, viewdirs, incidents_shs, direct_shs, visibility_shs},
                       dev);
    return render_equation_forward_impl(t, sample_num, is_training, &rand_float);
}

// RenderEquationForwardCUDA_complex (render_equation.cu:220-274)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
render_equation_forward_complex(const torch::Tensor& base_color, const torch::Tensor& roughness,
                                const torch::Tensor& metallic, const torch::Tensor& normals,
                                const torch::Tensor& viewdirs, const torch::Tensor& incidents_shs,
                                const torch::Tensor& direct_shs, const torch::Tensor& visibility_shs,
                                int64_t sample_num) {
    const torch::Device dev = base_color.device();
    const c10::OptionalDeviceGuard guard(dev);
    auto t = prep_brdf({base_color, roughness, metallic, normals, viewdirs, incidents_shs, direct_shs, visibility_shs},
                       dev);
    const int P = (int)t[0].size(0);
    const int64_t Ns = sample_num;
    auto fopt = t[0].options().dtype(torch::kFloat32);
    torch::Tensor pbr = torch::empty({P, 3}, fopt), dirs = torch::empty({P, Ns, 3}, fopt);
    torch::Tensor lights = torch::empty({P, Ns, 3}, fopt), local = torch::empty({P, Ns, 3}, fopt);
    torch::Tensor global = torch::empty({P, Ns, 3}, fopt), vis = torch::empty({P, Ns, 1}, fopt);
    torch::Tensor diffuse = torch::empty({P, 3}, fopt), local_diffuse = torch::empty({P, 3}, fopt);
    torch::Tensor accum = torch::empty({P, 1}, fopt), rgb_d = torch::empty({P, 3}, fopt);
    torch::Tensor rgb_s = torch::empty({P, 3}, fopt);
    r3dg_brdf_inputs in = brdf_inputs(t, (int)sample_num);
    r3dg_brdf_complex_outputs o{pbr.data_ptr<float>(),     dirs.data_ptr<float>(),  lights.data_ptr<float>(),
                                local.data_ptr<float>(),   global.data_ptr<float>(), vis.data_ptr<float>(),
                                diffuse.data_ptr<float>(), local_diffuse.data_ptr<float>(),
                                accum.data_ptr<float>(),   rgb_d.data_ptr<float>(), rgb_s.data_ptr<float>()};
    check(r3dg_render_equation_forward_complex(&in, &o, stream_of(dev)), "render_equation_forward_complex");
    return {pbr, dirs, lights, local, global, vis, diffuse, local_diffuse, accum, rgb_d, rgb_s};
}

// a float32 tensor on `dev` (a GPU), made contiguous; nothing is moved between devices
torch::Tensor relight_tensor(const torch::Tensor& t, const char* name, const torch::Device& dev) {
    TORCH_CHECK(t.is_cuda() && t.device() == dev, "relight: ", name, " must be on ", dev, ", got ", t.device());
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, "relight: ", name, " must be float32");
    return t.contiguous();
}

// r3dg_render_equation_relight: rendering_equation_python of the relighting script
// (neilf_composite.py:241-334) and the feature concatenation (:129-133) -> features [P, 21].
// light_mode 0 none / 1 SH (direct_shs [1, S, 3]) / 2 map (envmap [He, We, 3], env_transform [3, 3] or
// None); traced_visibility [P, Ns] or [P, Ns, 1], or None for the baked visibility_shs [P, S, 1].
torch::Tensor render_equation_relight(const torch::Tensor& base_color, const torch::Tensor& roughness,
                                      const torch::Tensor& metallic, const torch::Tensor& normals,
                                      const torch::Tensor& viewdirs, const torch::Tensor& incidents_shs,
                                      const std::optional<torch::Tensor>& direct_shs,
                                      const std::optional<torch::Tensor>& visibility_shs, int64_t sample_num,
                                      int64_t light_mode, const std::optional<torch::Tensor>& envmap,
                                      const std::optional<torch::Tensor>& env_transform,
                                      const std::optional<torch::Tensor>& traced_visibility) {
    TORCH_CHECK(base_color.is_cuda(), "relight: base_color must be a GPU tensor (this build has no CPU path)");
    const torch::Device dev = base_color.device();
    const c10::OptionalDeviceGuard guard(dev);
    TORCH_CHECK(base_color.dim() == 2 && base_color.size(1) == 3, "relight: base_color must be [P, 3]");
    const int64_t P = base_color.size(0);
    TORCH_CHECK(P <= INT32_MAX && sample_num <= INT32_MAX, "relight: P and sample_num must fit an int");
    auto per_gaussian = [&](const torch::Tensor& t, const char* name, int64_t w) {
        TORCH_CHECK(t.numel() == P * w && t.dim() >= 1 && t.size(0) == P, "relight: ", name, " must be [P, ", w, "]");
        return relight_tensor(t, name, dev);
    };
    auto sh_rows = [&](const torch::Tensor& t, const char* name, int64_t rows, int64_t ch) {
        TORCH_CHECK(t.dim() == 3 && t.size(0) == rows && t.size(2) == ch, "relight: ", name, " must be [", rows,
                    ", S, ", ch, "]");
        return relight_tensor(t, name, dev);
    };
    auto base = per_gaussian(base_color, "base_color", 3), rough = per_gaussian(roughness, "roughness", 1);
    auto metal = per_gaussian(metallic, "metallic", 1), nrm = per_gaussian(normals, "normals", 3);
    auto view = per_gaussian(viewdirs, "viewdirs", 3);
    auto inc = sh_rows(incidents_shs, "incidents_shs", P, 3);
    r3dg_relight_inputs in{};
    in.struct_size = sizeof(in);
    in.brdf.P = (int)P;
    in.brdf.sample_num = (int)sample_num;
    in.brdf.S_incident = (int)inc.size(1);
    in.brdf.base_color = base.data_ptr<float>(); in.brdf.roughness = rough.data_ptr<float>();
    in.brdf.metallic = metal.data_ptr<float>(); in.brdf.normals = nrm.data_ptr<float>();
    in.brdf.viewdirs = view.data_ptr<float>(); in.brdf.incidents_shs = inc.data_ptr<float>();
    in.light_mode = (int)light_mode;
    torch::Tensor env, vis, map, xf, traced;  // keep the contiguous copies alive over the launch
    if (light_mode == R3DG_LIGHT_SH) {
        TORCH_CHECK(direct_shs.has_value(), "relight: light_mode SH needs direct_shs");
        env = sh_rows(*direct_shs, "direct_shs", 1, 3);
        in.brdf.S_direct = (int)env.size(1);
        in.brdf.direct_shs = env.data_ptr<float>();
    } else if (light_mode == R3DG_LIGHT_MAP) {
        TORCH_CHECK(envmap.has_value(), "relight: light_mode MAP needs envmap");
        TORCH_CHECK(envmap->dim() == 3 && envmap->size(2) == 3 && envmap->size(0) >= 1 && envmap->size(1) >= 1 &&
                        envmap->size(0) <= INT32_MAX && envmap->size(1) <= INT32_MAX,
                    "relight: envmap must be [He, We, 3]");
        map = relight_tensor(*envmap, "envmap", dev);
        in.envmap = map.data_ptr<float>();
        in.env_h = (int)map.size(0);
        in.env_w = (int)map.size(1);
        if (env_transform.has_value()) {
            TORCH_CHECK(env_transform->dim() == 2 && env_transform->size(0) == 3 && env_transform->size(1) == 3,
                        "relight: env_transform must be [3, 3]");
            xf = relight_tensor(*env_transform, "env_transform", dev);
            in.env_transform = xf.data_ptr<float>();
        }
    }
    if (traced_visibility.has_value()) {
        const auto& tv = *traced_visibility;
        TORCH_CHECK((tv.dim() == 2 || (tv.dim() == 3 && tv.size(2) == 1)) && tv.size(0) == P && tv.size(1) == sample_num,
                    "relight: traced_visibility must be [P, sample_num] or [P, sample_num, 1]");
        traced = relight_tensor(tv, "traced_visibility", dev);
        // P = 0: an empty tensor's pointer may be null, which would read as "baked"
        in.traced_visibility = P > 0 ? traced.data_ptr<float>() : nullptr;
    } else {
        TORCH_CHECK(visibility_shs.has_value(), "relight: needs visibility_shs or traced_visibility");
        vis = sh_rows(*visibility_shs, "visibility_shs", P, 1);
        in.brdf.S_visibility = (int)vis.size(1);
        in.brdf.visibility_shs = vis.data_ptr<float>();
    }
    torch::Tensor features = torch::empty({P, 21}, base.options());
    check(r3dg_render_equation_relight(&in, features.data_ptr<float>(), stream_of(dev)), "render_equation_relight");
    return features;
}

// r3dg_envmap_direct_light: EnvLight.direct_light (scene/envmap.py:31-48), dirs [..., 3] -> [..., 3]
torch::Tensor envmap_direct_light(const torch::Tensor& dirs, const torch::Tensor& envmap,
                                  const std::optional<torch::Tensor>& env_transform) {
    TORCH_CHECK(dirs.is_cuda(), "envmap_direct_light: dirs must be a GPU tensor (this build has no CPU path)");
    const torch::Device dev = dirs.device();
    const c10::OptionalDeviceGuard guard(dev);
    TORCH_CHECK(dirs.dim() >= 1 && dirs.size(-1) == 3, "envmap_direct_light: dirs must be [..., 3]");
    TORCH_CHECK(envmap.dim() == 3 && envmap.size(2) == 3 && envmap.size(0) >= 1 && envmap.size(1) >= 1 &&
                    envmap.size(0) <= INT32_MAX && envmap.size(1) <= INT32_MAX,
                "envmap_direct_light: envmap must be [He, We, 3]");
    auto d = relight_tensor(dirs, "dirs", dev), map = relight_tensor(envmap, "envmap", dev);
    const int64_t n = d.numel() / 3;
    TORCH_CHECK(n <= INT32_MAX, "envmap_direct_light: too many directions");
    torch::Tensor xf;
    const float* xp = nullptr;
    if (env_transform.has_value()) {
        TORCH_CHECK(env_transform->dim() == 2 && env_transform->size(0) == 3 && env_transform->size(1) == 3,
                    "envmap_direct_light: env_transform must be [3, 3]");
        xf = relight_tensor(*env_transform, "env_transform", dev);
        xp = xf.data_ptr<float>();
    }
    torch::Tensor light = torch::empty_like(d);
    check(r3dg_envmap_direct_light((int)n, n ? d.data_ptr<float>() : nullptr, map.data_ptr<float>(), (int)map.size(0),
                                   (int)map.size(1), xp, n ? light.data_ptr<float>() : nullptr, stream_of(dev)),
          "envmap_direct_light");
    return light;
}

// RenderEquationBackwardCUDA (render_equation.cu:494-547)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor>
render_equation_backward(const torch::Tensor& base_color, const torch::Tensor& roughness,
                         const torch::Tensor& metallic, const torch::Tensor& normals, const torch::Tensor& viewdirs,
                         const torch::Tensor& incidents_shs, const torch::Tensor& direct_shs,
                         const torch::Tensor& visibility_shs, int64_t sample_num, const torch::Tensor& incident_dirs,
                         const torch::Tensor& dL_dpbr, const torch::Tensor& dL_ddiffuse_light, bool debug) {
    (void)debug;
    const torch::Device dev = base_color.device();
    const c10::OptionalDeviceGuard guard(dev);
    auto t = prep_brdf({base_color, roughness, metallic, normals, viewdirs, incidents_shs, direct_shs, visibility_shs,
                        incident_dirs, dL_dpbr, dL_ddiffuse_light},
                       dev);
    r3dg_brdf_inputs in = brdf_inputs(t, (int)sample_num);
    const int P = in.P;
    auto fopt = t[0].options().dtype(torch::kFloat32);
    torch::Tensor d_base = torch::empty({P, 3}, fopt), d_rough = torch::empty({P, 1}, fopt);
    torch::Tensor d_metal = torch::empty({P, 1}, fopt), d_n = torch::empty({P, 3}, fopt);
    torch::Tensor d_v = torch::empty({P, 3}, fopt), d_inc = torch::empty({P, in.S_incident, 3}, fopt);
    torch::Tensor d_dir = torch::empty({1, in.S_direct, 3}, fopt), d_vis = torch::empty({P, in.S_visibility, 1}, fopt);
    r3dg_brdf_grads o{d_base.data_ptr<float>(), d_rough.data_ptr<float>(), d_metal.data_ptr<float>(),
                      d_n.data_ptr<float>(),    d_v.data_ptr<float>(),     d_inc.data_ptr<float>(),
                      d_dir.data_ptr<float>(),  d_vis.data_ptr<float>()};
    auto bopt = torch::TensorOptions().dtype(torch::kUInt8).device(dev);
    TensorAlloc scratch{bopt, torch::empty({0}, bopt)};
    check(r3dg_render_equation_backward(&in, t[8].data_ptr<float>(), t[9].data_ptr<float>(), t[10].data_ptr<float>(),
                                        tensor_alloc, &scratch, &o, stream_of(dev)),
          "render_equation_backward");
    return {d_base, d_rough, d_metal, d_n, d_v, d_inc, d_dir, d_vis};
}

std::map<std::string, int64_t> shader_map(int kind) {
    std::map<std::string, int64_t> m;
    for (int i = 0; i < r3dg_shader_count(kind); ++i) m[r3dg_shader_name(kind, i)] = r3dg_shader_handle(kind, i);
    return m;
}

std::tuple<int64_t, int64_t> preprocess_model(torch::Tensor& xyz) {
    const torch::Device dev = xyz.device();
    const c10::OptionalDeviceGuard guard(dev);
    auto x = dev_contig(xyz, dev);
    int64_t a = 0, b = 0;
    check(r3dg_preprocess_model((int)xyz.size(0), x.numel() ? x.data_ptr<float>() : nullptr, &a, &b, stream_of(dev)),
          "PreprocessModel");
    return {a, b};
}

int64_t create_shader_manager(int64_t kind, const torch::Tensor& handles) {
    auto h = handles.to(torch::kCPU).to(torch::kInt64).contiguous();
    int64_t m = 0;
    check(r3dg_create_shader_manager((int)kind, (int)h.numel(), h.data_ptr<int64_t>(), &m,
                                     stream_of(torch::Device(torch::kCUDA, c10::hip::current_device()))),
          "create_shader_manager");
    return m;
}

std::tuple<std::vector<int64_t>, std::vector<int64_t>> shader_manager_info(int64_t mgr) {
    int n = 0;
    check(r3dg_shader_manager_info(mgr, &n, nullptr, nullptr), "shader_manager_info");
    std::vector<int64_t> h(n);
    std::vector<int> c(n);
    check(r3dg_shader_manager_info(mgr, &n, h.data(), c.data()), "shader_manager_info");
    return {h, std::vector<int64_t>(c.begin(), c.end())};
}

// AllocateTexture (texture.cu:86-101): the dict textureImport.py builds -- pixelData [H, W, C]
// float, height, width, encoding_mode, wrap_modes [2], normalizedCoords (CPU int32 tensors)
int64_t allocate_texture(const std::map<std::string, torch::Tensor>& d) {
    auto scalar = [&](const char* k, int i = 0) {
        auto it = d.find(k);
        if (it == d.end()) throw std::runtime_error(std::string("AllocateTexture: missing '") + k + "'");
        return it->second.to(torch::kCPU).to(torch::kInt64).contiguous().data_ptr<int64_t>()[i];
    };
    auto it = d.find("pixelData");
    if (it == d.end()) throw std::runtime_error("AllocateTexture: missing 'pixelData'");
    torch::Tensor pix = it->second.to(torch::kFloat32).contiguous();
    if (!pix.is_cuda()) pix = pix.cuda();
    const int H = (int)scalar("height"), W = (int)scalar("width"), mode = (int)scalar("encoding_mode");
    const int C = pix.numel() / std::max<int64_t>((int64_t)H * W, 1);
    if ((int64_t)C * H * W != pix.numel()) throw std::runtime_error("AllocateTexture: pixelData is not [H, W, C]");
    c10::OptionalDeviceGuard guard(pix.device());
    int64_t h = 0;
    check(r3dg_texture_create(pix.data_ptr<float>(), W, H, mode, (int)scalar("wrap_modes", 0),
                              (int)scalar("wrap_modes", 1), (int)scalar("normalizedCoords"), &h,
                              c10::hip::getCurrentHIPStream(pix.device().index()).stream()),
          "AllocateTexture");
    return h;
}
// UploadTexturesToDevice (texture.cu:237-246)
int64_t upload_textures(const std::vector<std::string>& names, const std::vector<int64_t>& textures,
                        int64_t error_texture) {
    if (names.size() != textures.size()) throw std::runtime_error("UploadTexturesToDevice: names/textures mismatch");
    std::vector<const char*> cn;
    for (const auto& n : names) cn.push_back(n.c_str());
    int64_t h = 0;
    check(r3dg_texture_manager_create((int)names.size(), cn.data(), textures.data(), error_texture, &h),
          "UploadTexturesToDevice");
    return h;
}

// parity / debug accessor: views of the sorted keys, point list, tile ranges and per-Gaussian state
std::vector<torch::Tensor> rasterizer_state(const torch::Tensor& geomBuffer, const torch::Tensor& binningBuffer,
                                            const torch::Tensor& imageBuffer, int64_t P, int64_t H, int64_t W,
                                            int64_t L) {
    r3dg_binning_view v{};
    check(r3dg_state_view((int)P, (int)H, (int)W, (int)L, geomBuffer.data_ptr(), binningBuffer.data_ptr(),
                          imageBuffer.data_ptr(), &v),
          "rasterizer_state");
    auto slice = [](const torch::Tensor& buf, const void* p, int64_t nbytes) {
        const int64_t off = (const char*)p - (const char*)buf.data_ptr();
        return buf.narrow(0, off, nbytes);
    };
    const int64_t T = ((W + 15) / 16) * ((H + 15) / 16);
    // the reference's sort key, rebuilt: tile << 32 | float bits of the instance's depth
    auto plist = slice(binningBuffer, v.point_list, 4 * L).view(torch::kInt32);
    auto dbits = slice(geomBuffer, v.depths, 4 * P).view(torch::kInt32).to(torch::kInt64).bitwise_and(0xffffffffLL);
    auto rng = slice(imageBuffer, v.ranges, 8 * T).view(torch::kInt32).view({T, 2}).to(torch::kInt64);
    auto tiles = torch::repeat_interleave(torch::arange(T, rng.options()), rng.select(1, 1) - rng.select(1, 0), 0, L);
    auto keys = tiles.bitwise_left_shift(32).bitwise_or(dbits.index_select(0, plist.to(torch::kInt64)));
    return {keys,
            plist,
            slice(imageBuffer, v.ranges, 8 * T).view(torch::kInt32).view({T, 2}),
            slice(geomBuffer, v.point_offsets, 4 * P).view(torch::kInt32),
            slice(geomBuffer, v.depths, 4 * P).view(torch::kFloat32),
            slice(geomBuffer, v.means2D, 8 * P).view(torch::kFloat32).view({P, 2}),
            slice(geomBuffer, v.conic_opacity, 16 * P).view(torch::kFloat32).view({P, 4}),
            slice(geomBuffer, v.rgb, 12 * P).view(torch::kFloat32).view({P, 3}),
            slice(geomBuffer, v.cov3D, 24 * P).view(torch::kFloat32).view({P, 6}),
            slice(geomBuffer, v.clamped, P)};
}

std::vector<int64_t> feature_groups(int64_t S) {
    int g[64];
    const int n = r3dg_feature_groups((int)S, g);
    return std::vector<int64_t>(g, g + n);
}

// ---- training step (include/r3dg_hip.h "training step on the device") ----

r3dg_param_layout make_layout(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles) {
    TORCH_CHECK(!widths.empty() && widths.size() <= R3DG_MAX_GROUPS, "param layout: 1..16 groups");
    TORCH_CHECK(roles.size() == 4, "param layout: roles = [xyz, scaling, rotation, opacity] group indices");
    r3dg_param_layout L{};
    L.P = (int)P;
    L.n_groups = (int)widths.size();
    for (size_t g = 0; g < widths.size(); ++g) L.width[g] = (int)widths[g];
    L.xyz = (int)roles[0]; L.scaling = (int)roles[1]; L.rotation = (int)roles[2]; L.opacity = (int)roles[3];
    return L;
}

float* f32_ptr(const torch::Tensor& t, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous(), what,
                ": expected a contiguous float32 device tensor");
    return t.data_ptr<float>();
}

void adam_step(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles, torch::Tensor param,
               const torch::Tensor& grad, torch::Tensor exp_avg, torch::Tensor exp_avg_sq, int64_t lo, int64_t hi,
               const std::vector<double>& lrs, double beta1, double beta2, double eps, int64_t step) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    TORCH_CHECK(lrs.size() == widths.size(), "adam_step: one learning rate per group");
    TORCH_CHECK(grad.numel() == hi - lo && exp_avg.numel() == hi - lo && exp_avg_sq.numel() == hi - lo,
                "adam_step: grad / exp_avg / exp_avg_sq must hold the shard's hi - lo floats");
    const c10::OptionalDeviceGuard guard(param.device());
    std::vector<float> lr(lrs.begin(), lrs.end());
    check(r3dg_adam_step(&L, f32_ptr(param, "param"), f32_ptr(grad, "grad"), f32_ptr(exp_avg, "exp_avg"),
                         f32_ptr(exp_avg_sq, "exp_avg_sq"), lo, hi, lr.data(), beta1, beta2, eps, (int)step,
                         stream_of(param.device())),
          "adam_step");
}

// adam_step with one step count per group; steps[g] <= 0: group g has no gradient (skipped)
void adam_step_groups(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles,
                      torch::Tensor param, const torch::Tensor& grad, torch::Tensor exp_avg, torch::Tensor exp_avg_sq,
                      int64_t lo, int64_t hi, const std::vector<double>& lrs, double beta1, double beta2, double eps,
                      const std::vector<int64_t>& steps) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    TORCH_CHECK(lrs.size() == widths.size() && steps.size() == widths.size(),
                "adam_step_groups: one learning rate and one step count per group");
    TORCH_CHECK(grad.numel() == hi - lo && exp_avg.numel() == hi - lo && exp_avg_sq.numel() == hi - lo,
                "adam_step_groups: grad / exp_avg / exp_avg_sq must hold the shard's hi - lo floats");
    const c10::OptionalDeviceGuard guard(param.device());
    std::vector<float> lr(lrs.begin(), lrs.end());
    std::vector<int> st(steps.begin(), steps.end());
    check(r3dg_adam_step_groups(&L, f32_ptr(param, "param"), f32_ptr(grad, "grad"), f32_ptr(exp_avg, "exp_avg"),
                                f32_ptr(exp_avg_sq, "exp_avg_sq"), lo, hi, lr.data(), st.data(), beta1, beta2, eps,
                                stream_of(param.device())),
          "adam_step_groups");
}

void densification_stats(const torch::Tensor& dL_dmeans2D, const torch::Tensor& normal_grad, const torch::Tensor& radii,
                         torch::Tensor xyz_accum, torch::Tensor normal_accum, torch::Tensor denom,
                         torch::Tensor max_radii2D) {
    const int P = (int)radii.size(0);
    TORCH_CHECK(radii.scalar_type() == torch::kInt32, "densification_stats: radii must be int32");
    TORCH_CHECK(dL_dmeans2D.dim() == 2 && dL_dmeans2D.size(0) == P && dL_dmeans2D.size(1) >= 2,
                "densification_stats: dL_dmeans2D must be [P, >=2]");
    TORCH_CHECK(normal_grad.numel() == 0 || normal_grad.numel() == 3 * (int64_t)P,
                "densification_stats: normal_grad must be [P, 3] or empty");
    const c10::OptionalDeviceGuard guard(radii.device());
    check(r3dg_densification_stats(P, f32_ptr(dL_dmeans2D, "dL_dmeans2D"), (int)dL_dmeans2D.size(1),
                                   normal_grad.numel() ? f32_ptr(normal_grad, "normal_grad") : nullptr,
                                   radii.data_ptr<int>(), f32_ptr(xyz_accum, "xyz_accum"),
                                   f32_ptr(normal_accum, "normal_accum"), f32_ptr(denom, "denom"),
                                   f32_ptr(max_radii2D, "max_radii2D"), stream_of(radii.device())),
          "densification_stats");
}

struct MultiAlloc {
    torch::TensorOptions opts;
    std::vector<torch::Tensor> ts;
};
void* multi_alloc(void* ctx, size_t n) {
    auto* a = static_cast<MultiAlloc*>(ctx);
    a->ts.push_back(torch::empty({(int64_t)std::max<size_t>((n + 3) / 4, 64)}, a->opts));
    return a->ts.back().data_ptr();
}
// noise source of densify_and_split: torch.randn on the device (the reference's torch.normal)
void* randn_alloc(void* ctx, size_t n) {
    auto* a = static_cast<MultiAlloc*>(ctx);
    a->ts.push_back(torch::randn({(int64_t)n}, a->opts));
    return a->ts.back().data_ptr();
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, int64_t, std::vector<int64_t>> densify_and_prune(
    int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles, const torch::Tensor& param,
    const torch::Tensor& exp_avg, const torch::Tensor& exp_avg_sq, const torch::Tensor& xyz_accum,
    const torch::Tensor& normal_accum, const torch::Tensor& denom, const torch::Tensor& max_radii2D,
    double grad_threshold, double grad_normal_threshold, double percent_dense, double extent, double min_opacity,
    double max_screen_size, int64_t N, bool prune_only, const torch::Tensor& noise) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    const c10::OptionalDeviceGuard guard(param.device());
    r3dg_densify_args d{};
    d.grad_threshold = (float)grad_threshold; d.grad_normal_threshold = (float)grad_normal_threshold;
    d.percent_dense = (float)percent_dense; d.extent = (float)extent; d.min_opacity = (float)min_opacity;
    d.max_screen_size = (float)max_screen_size; d.N = (int)N; d.prune_only = prune_only ? 1 : 0;
    MultiAlloc out{param.options(), {}}, rnd{param.options(), {}};
    // a given noise tensor (tests / replicated ranks) replaces the device generator
    auto given_noise = [](void* ctx, size_t n) -> void* {
        auto* t = static_cast<torch::Tensor*>(ctx);
        return (size_t)t->numel() >= n ? t->data_ptr() : nullptr;
    };
    torch::Tensor nz = noise;
    float *np = nullptr, *nm = nullptr, *nv = nullptr;
    int* src = nullptr;
    int Pn = 0, counts[4] = {0, 0, 0, 0};
    auto opt = [](const torch::Tensor& t, const char* w) { return t.numel() ? f32_ptr(t, w) : nullptr; };
    check(r3dg_densify_and_prune(&L, f32_ptr(param, "param"), f32_ptr(exp_avg, "exp_avg"),
                                 f32_ptr(exp_avg_sq, "exp_avg_sq"), opt(xyz_accum, "xyz_accum"),
                                 opt(normal_accum, "normal_accum"), opt(denom, "denom"),
                                 opt(max_radii2D, "max_radii2D"), &d, multi_alloc, &out,
                                 noise.numel() ? (r3dg_alloc_fn)given_noise : randn_alloc,
                                 noise.numel() ? (void*)&nz : (void*)&rnd, &np, &nm, &nv, &src, &Pn, counts,
                                 stream_of(param.device())),
          "densify_and_prune");
    auto find = [&](void* p) {
        for (auto& t : out.ts)
            if (t.data_ptr() == p) return t;
        TORCH_CHECK(false, "densify_and_prune: output not found");
        return torch::Tensor();
    };
    int64_t W = 0;
    for (auto w : widths) W += w;
    const int64_t n = (int64_t)Pn * W;
    torch::Tensor source = torch::from_blob(src, {(int64_t)Pn}, [](void*) {}, param.options().dtype(torch::kInt32));
    source = source.clone();  // own the map (the scratch allocation is released on return)
    return {find(np).narrow(0, 0, n), find(nm).narrow(0, 0, n), find(nv).narrow(0, 0, n), source, (int64_t)Pn,
            std::vector<int64_t>{counts[0], counts[1], counts[2], counts[3]}};
}

void reset_opacity(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles,
                   torch::Tensor param, const torch::Tensor& exp_avg, const torch::Tensor& exp_avg_sq) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    const c10::OptionalDeviceGuard guard(param.device());
    check(r3dg_reset_opacity(&L, f32_ptr(param, "param"), exp_avg.numel() ? f32_ptr(exp_avg, "exp_avg") : nullptr,
                             exp_avg_sq.numel() ? f32_ptr(exp_avg_sq, "exp_avg_sq") : nullptr,
                             stream_of(param.device())),
          "reset_opacity");
}

// ---- parameter activations (relightable3dgaussian_amd/activation.py; csrc/activation.hip) ----------

// role_groups: the group index of normal, f_dc, f_rest, base_color, roughness, metallic, incidents_dc,
// incidents_rest, visibility_dc, visibility_rest (-1: absent)
r3dg_activation_io make_activation_io(const r3dg_param_layout* L, const std::vector<int64_t>& role_groups,
                                      const torch::Tensor& param, const std::optional<torch::Tensor>& campos,
                                      torch::Tensor& campos_keep, const char* who) {
    TORCH_CHECK(role_groups.size() == 10, who, ": role_groups holds 10 group indices");
    TORCH_CHECK(param.is_cuda(), who, ": param must be a GPU tensor (this build has no CPU path)");
    int64_t total = 0;
    for (int g = 0; g < L->n_groups; ++g) total += (int64_t)L->P * L->width[g];
    TORCH_CHECK(L->P >= 0 && param.numel() >= total, who, ": param holds fewer than P * sum(widths) floats");
    f32_ptr(param, "param");
    r3dg_activation_io io{};
    io.struct_size = sizeof(io);
    io.layout = L;
    io.normal = (int)role_groups[0]; io.f_dc = (int)role_groups[1]; io.f_rest = (int)role_groups[2];
    io.base_color = (int)role_groups[3]; io.roughness = (int)role_groups[4]; io.metallic = (int)role_groups[5];
    io.incidents_dc = (int)role_groups[6]; io.incidents_rest = (int)role_groups[7];
    io.visibility_dc = (int)role_groups[8]; io.visibility_rest = (int)role_groups[9];
    if (campos.has_value()) {
        TORCH_CHECK(campos->is_cuda() && campos->scalar_type() == torch::kFloat32 && campos->numel() == 3 &&
                        campos->device() == param.device(),
                    who, ": campos must be 3 float32 on param's device");
        campos_keep = campos->contiguous();
        io.campos = campos_keep.data_ptr<float>();
    }
    return io;
}

// -> [scaling, rotation, normal, opacity, shs, base_color, roughness, metallic, incidents, visibility,
//     viewdirs, symm_inv]; None for the PBR outputs of a 7-group layout, viewdirs without campos, symm_inv
//     when not asked for
std::vector<std::optional<torch::Tensor>> activate_forward(int64_t P, const std::vector<int64_t>& widths,
                                                           const std::vector<int64_t>& roles,
                                                           const std::vector<int64_t>& role_groups,
                                                           const torch::Tensor& param,
                                                           const std::optional<torch::Tensor>& campos,
                                                           bool inverse_covariance) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    torch::Tensor cp;
    r3dg_activation_io io = make_activation_io(&L, role_groups, param, campos, cp, "activate_forward");
    const c10::OptionalDeviceGuard guard(param.device());
    const auto fopt = param.options();
    const bool pbr = io.base_color >= 0;
    std::vector<std::optional<torch::Tensor>> out(12);
    auto make = [&](int slot, std::vector<int64_t> shape, bool on) -> float* {
        if (!on) return nullptr;
        shape.insert(shape.begin(), P);
        out[slot] = torch::empty(shape, fopt);
        return out[slot]->data_ptr<float>();
    };
    io.out_scaling = make(0, {3}, true); io.out_rotation = make(1, {4}, true); io.out_normal = make(2, {3}, true);
    io.out_opacity = make(3, {1}, true); io.out_shs = make(4, {16, 3}, true);
    io.out_base_color = make(5, {3}, pbr); io.out_roughness = make(6, {1}, pbr); io.out_metallic = make(7, {1}, pbr);
    io.out_incidents = make(8, {16, 3}, pbr); io.out_visibility = make(9, {16, 1}, pbr);
    io.out_viewdirs = make(10, {3}, campos.has_value()); io.out_symm_inv = make(11, {6}, inverse_covariance);
    check(r3dg_activate_forward(&io, param.data_ptr<float>(), stream_of(param.device())), "activate_forward");
    return out;
}

// upstreams: [xyz, scaling, rotation, normal, opacity, shs, base_color, roughness, metallic, incidents,
// visibility, viewdirs], None = zero. An upstream whose dimensions behind the first are dense (a column block
// of a wider row-major array) is passed with its stride(0); any other layout is made contiguous first.
void activate_backward(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles,
                       const std::vector<int64_t>& role_groups, const torch::Tensor& param,
                       const std::optional<torch::Tensor>& campos,
                       const std::vector<std::optional<torch::Tensor>>& upstreams, torch::Tensor grad,
                       bool accumulate) {
    const char* who = "activate_backward";
    const r3dg_param_layout L = make_layout(P, widths, roles);
    torch::Tensor cp;
    const r3dg_activation_io io = make_activation_io(&L, role_groups, param, campos, cp, who);
    TORCH_CHECK(upstreams.size() == 12, who, ": 12 upstream slots");
    TORCH_CHECK(grad.is_cuda() && grad.device() == param.device() && grad.numel() >= param.numel(), who,
                ": grad must be a buffer of param's size on param's device");
    f32_ptr(grad, "grad");
    const c10::OptionalDeviceGuard guard(param.device());
    r3dg_activation_grads g{};
    g.struct_size = sizeof(g);
    r3dg_grad_rows* slots[12] = {&g.xyz, &g.scaling, &g.rotation, &g.normal, &g.opacity, &g.shs, &g.base_color,
                                 &g.roughness, &g.metallic, &g.incidents, &g.visibility, &g.viewdirs};
    const int64_t width[12] = {3, 3, 4, 3, 1, 48, 3, 1, 1, 48, 16, 3};
    std::vector<torch::Tensor> keep;
    for (int i = 0; i < 12; ++i) {
        if (!upstreams[i].has_value()) continue;
        torch::Tensor t = *upstreams[i];
        TORCH_CHECK(t.is_cuda() && t.device() == param.device() && t.scalar_type() == torch::kFloat32, who,
                    ": upstream ", i, " must be a float32 tensor on param's device");
        TORCH_CHECK(t.dim() >= 1 && t.size(0) == P && t.numel() == P * width[i], who, ": upstream ", i,
                    " must be [P, ...] with ", width[i], " floats per row");
        // dense behind the first dimension, rows at least a row apart
        bool dense = t.stride(0) >= width[i];
        int64_t expect = 1;
        for (int64_t d = t.dim() - 1; d >= 1; --d) {
            if (t.size(d) != 1 && t.stride(d) != expect) dense = false;
            expect *= t.size(d);
        }
        if (!dense) t = t.contiguous();
        keep.push_back(t);
        if (P > 0) *slots[i] = r3dg_grad_rows{t.data_ptr<float>(), P == 1 ? width[i] : t.stride(0)};
    }
    check(r3dg_activate_backward(&io, param.data_ptr<float>(), &g, grad.data_ptr<float>(), accumulate ? 1 : 0,
                                 stream_of(param.device())),
          who);
}

// ---- scene composition and the points capture (relightable3dgaussian_amd/compose.py; csrc/compose.hip) ----

// the 19 floats of a transform on param's device (None with flags == 0)
const float* xform_ptr(const std::optional<torch::Tensor>& xform, int64_t flags, const torch::Tensor& param,
                       const char* who) {
    if (!xform.has_value()) {
        TORCH_CHECK(flags == 0, who, ": transform flags without the 19 floats");
        return nullptr;
    }
    TORCH_CHECK(xform->is_cuda() && xform->device() == param.device() && xform->scalar_type() == torch::kFloat32 &&
                    xform->is_contiguous() &&
                    (xform->numel() == 19 || (xform->numel() == 16 && flags == R3DG_XF_TRANSFORM)),
                who, ": xform must be 19 contiguous float32 on param's device (16 do for a full transform)");
    return xform->data_ptr<float>();
}

void set_transform(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles,
                   int64_t normal_group, torch::Tensor param, const std::optional<torch::Tensor>& xform,
                   int64_t flags) {
    const char* who = "set_transform";
    const r3dg_param_layout L = make_layout(P, widths, roles);
    f32_ptr(param, "set_transform: param");
    int64_t total = 0;
    for (int g = 0; g < L.n_groups; ++g) total += (int64_t)L.P * L.width[g];
    TORCH_CHECK(L.P >= 0 && param.numel() >= total, who, ": param holds fewer than P * sum(widths) floats");
    const float* xf = xform_ptr(xform, flags, param, who);
    const c10::OptionalDeviceGuard guard(param.device());
    check(r3dg_set_transform(&L, (int)normal_group, param.data_ptr<float>(), xf, (int)flags,
                             stream_of(param.device())),
          who);
}

// outs: [xyz, scaling, rotation, normal, opacity, base_color, roughness, metallic, shs, incidents, visibility_dc,
// visibility_rest, symm_inv (None: skipped)], the composite's arrays; the object writes rows [row, row + P)
void compose_object(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles,
                    const std::vector<int64_t>& role_groups, const torch::Tensor& param,
                    const std::optional<torch::Tensor>& xform, int64_t flags,
                    const std::vector<std::optional<torch::Tensor>>& outs, int64_t row) {
    const char* who = "compose_object";
    const r3dg_param_layout L = make_layout(P, widths, roles);
    torch::Tensor cp;
    const r3dg_activation_io io = make_activation_io(&L, role_groups, param, std::nullopt, cp, who);
    const float* xf = xform_ptr(xform, flags, param, who);
    TORCH_CHECK(outs.size() == 13, who, ": 13 output slots");
    TORCH_CHECK(row >= 0, who, ": negative row offset");
    const int64_t width[13] = {3, 3, 4, 3, 1, 3, 1, 1, 48, 48, 1, 24, 6};
    float* ptr[13];
    for (int i = 0; i < 13; ++i) {
        ptr[i] = nullptr;
        if (!outs[i].has_value()) {
            TORCH_CHECK(i == 12, who, ": only symm_inv may be None");
            continue;
        }
        const torch::Tensor& t = *outs[i];
        TORCH_CHECK(t.is_cuda() && t.device() == param.device() && t.scalar_type() == torch::kFloat32 &&
                        t.is_contiguous(),
                    who, ": output ", i, " must be a contiguous float32 tensor on param's device");
        TORCH_CHECK(t.numel() >= (row + P) * width[i], who, ": output ", i, " holds fewer than row + P rows");
        ptr[i] = t.data_ptr<float>();
    }
    r3dg_compose_out o{};
    o.struct_size = sizeof(o);
    o.xyz = ptr[0]; o.scaling = ptr[1]; o.rotation = ptr[2]; o.normal = ptr[3]; o.opacity = ptr[4];
    o.base_color = ptr[5]; o.roughness = ptr[6]; o.metallic = ptr[7]; o.shs = ptr[8]; o.incidents = ptr[9];
    o.visibility_dc = ptr[10]; o.visibility_rest = ptr[11]; o.symm_inv = ptr[12];
    const c10::OptionalDeviceGuard guard(param.device());
    check(r3dg_compose_object(&io, param.data_ptr<float>(), xf, (int)flags, &o, row, stream_of(param.device())), who);
}

// bg: 3 floats on the device, or None with the 3 host numbers bg_value (passed to the kernel by value)
// -> (rgb [3,H,W], depth [H,W] or None)
std::tuple<torch::Tensor, std::optional<torch::Tensor>> render_points(const torch::Tensor& xyz,
                                                                      const torch::Tensor& color,
                                                                      const torch::Tensor& world_view,
                                                                      const torch::Tensor& intrinsics, int64_t H,
                                                                      int64_t W,
                                                                      const std::optional<torch::Tensor>& bg,
                                                                      const std::vector<double>& bg_value,
                                                                      bool return_depth) {
    const char* who = "render_points";
    const torch::Device dev = xyz.device();
    auto dev_f32 = [&](const torch::Tensor& t, int64_t n, const char* name) {
        TORCH_CHECK(t.is_cuda() && t.device() == dev && t.scalar_type() == torch::kFloat32, who, ": ", name,
                    " must be a float32 tensor on xyz's GPU device (this build has no CPU path)");
        TORCH_CHECK(n < 0 || t.numel() == n, who, ": ", name, " must hold ", n, " floats");
        return t.contiguous();
    };
    TORCH_CHECK(xyz.dim() == 2 && xyz.size(1) == 3 && color.dim() == 2 && color.size(1) == 3 &&
                    color.size(0) == xyz.size(0),
                who, ": xyz and color must be [P, 3]");
    TORCH_CHECK(H > 0 && W > 0 && H * W <= 0x7fffffffLL, who, ": bad H or W");
    TORCH_CHECK(xyz.size(0) <= 0x7fffffffLL, who, ": more than 2^31 - 1 points (a pixel's key holds a 32-bit index)");
    const auto x = dev_f32(xyz, -1, "xyz"), c = dev_f32(color, -1, "color");
    const auto v = dev_f32(world_view, 16, "world_view_transform"), k = dev_f32(intrinsics, 9, "intrinsics");
    torch::Tensor b;
    float bgv[3] = {0.0f, 0.0f, 0.0f};
    if (bg.has_value()) {
        b = dev_f32(*bg, 3, "bg");
    } else {
        TORCH_CHECK(bg_value.size() == 3, who, ": bg_value must hold 3 numbers");
        for (int i = 0; i < 3; ++i) bgv[i] = (float)bg_value[i];
    }
    const c10::OptionalDeviceGuard guard(dev);
    torch::Tensor rgb = torch::empty({3, H, W}, xyz.options());
    std::optional<torch::Tensor> depth;
    if (return_depth) depth = torch::empty({H, W}, xyz.options());
    const int64_t P = xyz.size(0);
    auto bopt = torch::TensorOptions().dtype(torch::kUInt8).device(dev);
    TensorAlloc scratch{bopt, torch::empty({0}, bopt)};
    check(r3dg_render_points((int)P, P ? x.data_ptr<float>() : nullptr, P ? c.data_ptr<float>() : nullptr,
                             v.data_ptr<float>(), k.data_ptr<float>(), (int)H, (int)W,
                             bg.has_value() ? b.data_ptr<float>() : nullptr, bgv, rgb.data_ptr<float>(), depth ? depth->data_ptr<float>() : nullptr, tensor_alloc, &scratch,
                             stream_of(dev)),
          who);
    return {rgb, depth};
}

// ---- BVH visibility tracer: the reference's bvh_tracing._C (bvh/src/bindings.cpp:9-11) ----------

torch::Tensor cuda_f32(const torch::Tensor& t, const char* what) {
    TORCH_CHECK(t.is_cuda(), what, ": expected a GPU tensor (this build has no CPU path)");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, what, ": expected float32");
    return t.contiguous();
}

// RayTracer.__init__ leaf boxes (bvh/__init__.py:29-59) in one launch -> [P, 6]
torch::Tensor bvh_leaf_aabbs(const torch::Tensor& means3D, const torch::Tensor& scales,
                             const torch::Tensor& rotations) {
    const auto m = cuda_f32(means3D, "bvh_leaf_aabbs"), s = cuda_f32(scales, "bvh_leaf_aabbs"),
               r = cuda_f32(rotations, "bvh_leaf_aabbs");
    const int64_t P = m.size(0);
    TORCH_CHECK(m.numel() == 3 * P && s.numel() == 3 * P && r.numel() == 4 * P,
                "bvh_leaf_aabbs: means3D [P,3], scales [P,3], rotations [P,4] expected");
    const c10::OptionalDeviceGuard guard(m.device());
    auto out = torch::empty({P, 6}, m.options());
    check(r3dg_bvh_leaf_aabbs((int)P, m.data_ptr<float>(), s.data_ptr<float>(), r.data_ptr<float>(),
                              out.data_ptr<float>(), stream_of(m.device())),
          "bvh_leaf_aabbs");
    return out;
}

// create_bvh (bvh/src/bvh.cu:8-26): fills nodes / aabbs in place (their leaf boxes are the input)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> create_bvh(const torch::Tensor& means3D,
                                                                   const torch::Tensor& scales,
                                                                   const torch::Tensor& rotations,
                                                                   torch::Tensor nodes, torch::Tensor aabbs) {
    (void)scales;
    (void)rotations;  // the reference takes them and does not read them (construct.cu:148-155)
    const int64_t P = means3D.size(0);
    TORCH_CHECK(nodes.is_cuda() && aabbs.is_cuda(), "create_bvh: expected GPU tensors");
    TORCH_CHECK(nodes.scalar_type() == torch::kInt32 && aabbs.scalar_type() == torch::kFloat32,
                "create_bvh: nodes int32, aabbs float32 expected");
    TORCH_CHECK(nodes.is_contiguous() && aabbs.is_contiguous(), "create_bvh: nodes / aabbs must be contiguous");
    TORCH_CHECK(P >= 1 && nodes.numel() == 5 * (2 * P - 1) && aabbs.numel() == 6 * (2 * P - 1),
                "create_bvh: nodes [2P-1,5] and aabbs [2P-1,6] expected");
    const c10::OptionalDeviceGuard guard(aabbs.device());
    auto morton = torch::empty({P}, aabbs.options().dtype(torch::kInt64));
    TensorAlloc scratch{aabbs.options().dtype(torch::kUInt8), {}};
    check(r3dg_bvh_build((int)P, nodes.data_ptr<int32_t>(), aabbs.data_ptr<float>(),
                         reinterpret_cast<uint64_t*>(morton.data_ptr<int64_t>()), tensor_alloc, &scratch,
                         stream_of(aabbs.device())),
          "create_bvh");
    return {nodes, aabbs, morton};
}

// distCUDA2 (submodules/simple-knn/spatial.cu:15-26): [P,3] f32 points -> [P] mean squared distance to
// the three nearest other points, on the current stream
torch::Tensor dist_cuda2(const torch::Tensor& points) {
    TORCH_CHECK(points.scalar_type() == torch::kFloat32, "distCUDA2: expected float32");
    TORCH_CHECK(points.dim() == 2 && points.size(1) == 3, "distCUDA2: points [P,3] expected");
    TORCH_CHECK(points.is_cuda(), "distCUDA2: expected a GPU tensor (this build has no CPU path)");
    TORCH_CHECK(points.size(0) < (int64_t(1) << 30), "distCUDA2: too many points");
    const auto p = points.contiguous();
    const int64_t P = p.size(0);
    const c10::OptionalDeviceGuard guard(p.device());
    auto out = torch::empty({P}, p.options());
    TensorAlloc scratch{p.options().dtype(torch::kUInt8), {}};
    check(r3dg_knn_mean_dist2((int)P, P ? p.data_ptr<float>() : nullptr, P ? out.data_ptr<float>() : nullptr,
                              tensor_alloc, &scratch, stream_of(p.device())),
          "distCUDA2");
    return out;
}

// ---- image loss (utils/loss_utils.py:31-62 ssim, neilf.py:216-222) --------------------------------

// img: [..., H, W] planes (hwc false) or the rasterizer's [H, W, C] (hwc true); gt always [..., H, W]
// with as many planes. The checked, contiguous pair and the geometry the C ABI wants.
struct LossImages {
    torch::Tensor img, gt;
    int64_t planes, H, W, img_stride[3];
};
LossImages loss_images(const torch::Tensor& img, const torch::Tensor& gt, bool hwc, const char* what) {
    TORCH_CHECK(img.scalar_type() == torch::kFloat32 && gt.scalar_type() == torch::kFloat32, what,
                ": expected float32");
    TORCH_CHECK(gt.dim() >= 2, what, ": gt [..., H, W] expected");
    LossImages r;
    r.H = gt.size(-2);
    r.W = gt.size(-1);
    r.planes = r.H * r.W ? gt.numel() / (r.H * r.W) : 0;
    if (hwc) {
        TORCH_CHECK(img.dim() == 3 && gt.dim() == 3 && img.size(0) == r.H && img.size(1) == r.W &&
                        img.size(2) == gt.size(0),
                    what, ": shape mismatch: img [H,W,C] against gt [C,H,W] expected");
        r.img_stride[0] = 1, r.img_stride[1] = r.W * r.planes, r.img_stride[2] = r.planes;
    } else {
        TORCH_CHECK(img.sizes() == gt.sizes(), what, ": shape mismatch between img and gt");
        r.img_stride[0] = r.H * r.W, r.img_stride[1] = r.W, r.img_stride[2] = 1;
    }
    TORCH_CHECK(gt.numel() <= (int64_t)INT32_MAX, what, ": planes * H * W exceeds int32");
    TORCH_CHECK(img.is_cuda() && gt.is_cuda(), what, ": expected GPU tensors (this build has no CPU path)");
    TORCH_CHECK(img.device() == gt.device(), what, ": img and gt on different devices");
    r.img = img.contiguous();
    r.gt = gt.contiguous();
    return r;
}

// -> (sums [planes, 3]: per plane the sums of ssim_map, |img - gt|, (img - gt)^2; dmaps [3, planes, H, W]
// for image_loss_backward, or an empty tensor when need_grad is false)
std::tuple<torch::Tensor, torch::Tensor> image_loss_forward(const torch::Tensor& img, const torch::Tensor& gt,
                                                            bool hwc, bool need_grad) {
    const auto a = loss_images(img, gt, hwc, "image_loss_forward");
    const c10::OptionalDeviceGuard guard(a.img.device());
    auto sums = a.gt.numel() ? torch::empty({a.planes, 3}, a.img.options()) : torch::zeros({a.planes, 3}, a.img.options());
    auto dmaps = need_grad ? torch::empty({3, a.planes, a.H, a.W}, a.img.options()) : torch::empty({0}, a.img.options());
    TensorAlloc scratch{a.img.options().dtype(torch::kUInt8), {}};
    check(r3dg_image_loss_forward((int)a.planes, (int)a.H, (int)a.W, a.img.data_ptr<float>(), a.img_stride[0],
                                  a.img_stride[1], a.img_stride[2], a.gt.data_ptr<float>(), a.H * a.W, a.W, 1,
                                  sums.data_ptr<float>(), need_grad && dmaps.numel() ? dmaps.data_ptr<float>() : nullptr,
                                  tensor_alloc, &scratch, stream_of(a.img.device())),
          "image_loss_forward");
    return {sums, dmaps};
}

// -> dL/dimg, shaped and laid out like img: scale * (w_ssim * d(sum ssim_map)/dimg + w_abs * sign(img - gt))
// per plane, the weights read on the device (an absent scale is 1)
torch::Tensor image_loss_backward(const torch::Tensor& img, const torch::Tensor& gt, bool hwc,
                                  const torch::Tensor& dmaps, const torch::Tensor& w_ssim, const torch::Tensor& w_abs,
                                  const std::optional<torch::Tensor>& scale) {
    const auto a = loss_images(img, gt, hwc, "image_loss_backward");
    auto weight = [&](const torch::Tensor& t, const char* name) {
        TORCH_CHECK(t.is_cuda() && t.device() == a.img.device() && t.scalar_type() == torch::kFloat32 &&
                        t.numel() == a.planes,
                    "image_loss_backward: ", name, " float32 [planes] on the images' device expected");
        return t.contiguous();
    };
    TORCH_CHECK(dmaps.is_cuda() && dmaps.device() == a.img.device() && dmaps.scalar_type() == torch::kFloat32 &&
                    dmaps.numel() == 3 * a.gt.numel(),
                "image_loss_backward: dmaps float32 [3,planes,H,W] from image_loss_forward(need_grad=True) expected");
    const auto d = dmaps.contiguous(), ws = weight(w_ssim, "w_ssim"), wa = weight(w_abs, "w_abs");
    const auto sc = scale ? weight(*scale, "scale") : torch::Tensor();
    const c10::OptionalDeviceGuard guard(a.img.device());
    auto out = torch::empty_like(a.img);
    check(r3dg_image_loss_backward((int)a.planes, (int)a.H, (int)a.W, a.img.data_ptr<float>(), a.img_stride[0],
                                   a.img_stride[1], a.img_stride[2], a.gt.data_ptr<float>(), a.H * a.W, a.W, 1,
                                   d.data_ptr<float>(), ws.data_ptr<float>(), wa.data_ptr<float>(),
                                   scale ? sc.data_ptr<float>() : nullptr, out.data_ptr<float>(),
                                   stream_of(a.img.device())),
          "image_loss_backward");
    return out;
}

// ---- image-space regularisers (neilf.py:233-321; csrc/reg_loss.hip) -------------------------------

// The eleven maps in the order of r3dg_reg_loss_inputs: opacity, depth, normal, pseudo_normal, base_color,
// roughness, metallic (rendered: [n,H,W], or the rasterizer's [H,W,n] with hwc), then gt_image, gt_depth,
// image_mask, mvs_normal (always [n,H,W]). None is absent. The checked, contiguous tensors and the struct.
struct RegInputs {
    std::vector<torch::Tensor> keep;
    r3dg_reg_loss_inputs in;
    torch::Device dev{torch::kCPU};
};
constexpr int kRegMaps = 11, kRegRendered = 7;
const int kRegPlanes[kRegMaps] = {1, 1, 3, 3, 3, 1, 1, 3, 1, 1, 3};
const char* const kRegNames[kRegMaps] = {"opacity", "depth", "normal", "pseudo_normal", "base_color", "roughness",
                                         "metallic", "gt_image", "gt_depth", "image_mask", "mvs_normal"};
RegInputs reg_inputs(const std::vector<std::optional<torch::Tensor>>& maps, int64_t H, int64_t W, int64_t terms,
                     bool hwc, const char* what) {
    TORCH_CHECK((int64_t)maps.size() == kRegMaps, what, ": ", kRegMaps, " maps (or None) expected");
    TORCH_CHECK(H >= 0 && W >= 0 && H * W <= (int64_t)INT32_MAX, what, ": H, W >= 0 and H * W within int32 expected");
    TORCH_CHECK(terms >= 0 && terms < (1 << R3DG_REG_TERMS), what, ": unknown bits in terms");
    RegInputs r;
    r.keep.resize(kRegMaps);
    r.in = r3dg_reg_loss_inputs{};
    r.in.struct_size = sizeof(r3dg_reg_loss_inputs);
    r.in.H = (int)H, r.in.W = (int)W, r.in.terms = (unsigned)terms;
    r3dg_map* dst[kRegMaps] = {&r.in.opacity, &r.in.depth, &r.in.normal, &r.in.pseudo_normal, &r.in.base_color,
                               &r.in.roughness, &r.in.metallic, &r.in.gt_image, &r.in.gt_depth, &r.in.image_mask,
                               &r.in.mvs_normal};
    bool have = false;
    for (int i = 0; i < kRegMaps; ++i) {
        if (!maps[i]) continue;
        const torch::Tensor& t = *maps[i];
        const int64_t n = kRegPlanes[i];
        TORCH_CHECK(t.scalar_type() == torch::kFloat32, what, ": ", kRegNames[i], ": expected float32");
        const bool pixel_major = hwc && i < kRegRendered;
        if (pixel_major) {
            TORCH_CHECK(t.dim() == 3 && t.size(0) == H && t.size(1) == W && t.size(2) == n, what, ": shape mismatch: ",
                        kRegNames[i], " [H,W,", n, "] expected, got ", t.sizes());
        } else {
            TORCH_CHECK(t.dim() == 3 && t.size(0) == n && t.size(1) == H && t.size(2) == W, what, ": shape mismatch: ",
                        kRegNames[i], " [", n, ",H,W] expected, got ", t.sizes());
        }
        TORCH_CHECK(t.is_cuda(), what, ": ", kRegNames[i], ": expected a GPU tensor (this build has no CPU path)");
        if (!have) r.dev = t.device(), have = true;
        TORCH_CHECK(t.device() == r.dev, what, ": ", kRegNames[i], ": maps on different devices");
        r.keep[i] = t.contiguous();
        if (t.numel() == 0) continue;
        *dst[i] = pixel_major ? r3dg_map{r.keep[i].data_ptr<float>(), 1, W * n, n}
                              : r3dg_map{r.keep[i].data_ptr<float>(), H * W, W, 1};
    }
    TORCH_CHECK(have, what, ": no map given");
    return r;
}

// -> (values f32 [8]: each enabled term's value under its R3DG_REG_* index, 0 for a disabled one;
//     depth_count int32 [1]: the pixels the depth term selected)
std::tuple<torch::Tensor, torch::Tensor> reg_loss_forward(const std::vector<std::optional<torch::Tensor>>& maps,
                                                          int64_t H, int64_t W, int64_t terms, bool hwc) {
    auto a = reg_inputs(maps, H, W, terms, hwc, "reg_loss_forward");
    const c10::OptionalDeviceGuard guard(a.dev);
    const auto fopt = torch::TensorOptions().dtype(torch::kFloat32).device(a.dev);
    // with work to do the finishing kernel writes every slot (0 for a disabled term)
    const bool work = H * W != 0 && terms != 0;
    auto values = work ? torch::empty({R3DG_REG_TERMS}, fopt) : torch::zeros({R3DG_REG_TERMS}, fopt);
    auto count = work ? torch::empty({1}, fopt.dtype(torch::kInt32)) : torch::zeros({1}, fopt.dtype(torch::kInt32));
    TensorAlloc scratch{fopt.dtype(torch::kUInt8), {}};
    check(r3dg_reg_loss_forward(&a.in, values.data_ptr<float>(), count.data_ptr<int32_t>(), tensor_alloc, &scratch,
                                stream_of(a.dev)),
          "reg_loss_forward");
    return {values, count};
}

// -> the gradients of opacity, depth, normal, base_color, roughness, metallic, each laid out like its map, or
// None where `want` (a bit per map, in this order) is clear or no enabled term reaches the map
std::vector<std::optional<torch::Tensor>> reg_loss_backward(const std::vector<std::optional<torch::Tensor>>& maps,
                                                            int64_t H, int64_t W, int64_t terms, bool hwc,
                                                            const torch::Tensor& depth_count,
                                                            const torch::Tensor& weights,
                                                            const std::optional<torch::Tensor>& scale, int64_t want) {
    auto a = reg_inputs(maps, H, W, terms, hwc, "reg_loss_backward");
    TORCH_CHECK(depth_count.is_cuda() && depth_count.device() == a.dev && depth_count.scalar_type() == torch::kInt32 &&
                    depth_count.numel() == 1,
                "reg_loss_backward: depth_count int32 [1] from reg_loss_forward expected");
    TORCH_CHECK(weights.is_cuda() && weights.device() == a.dev && weights.scalar_type() == torch::kFloat32 &&
                    weights.numel() == R3DG_REG_TERMS,
                "reg_loss_backward: weights float32 [8] on the maps' device expected");
    TORCH_CHECK(!scale || (scale->is_cuda() && scale->device() == a.dev && scale->scalar_type() == torch::kFloat32 &&
                           scale->numel() == 1),
                "reg_loss_backward: scale float32 [1] on the maps' device expected");
    const auto w = weights.contiguous(), cnt = depth_count.contiguous();
    const auto sc = scale ? scale->contiguous() : torch::Tensor();
    const c10::OptionalDeviceGuard guard(a.dev);
    const unsigned t = (unsigned)terms;
    auto bit = [&](int k) { return (t >> k & 1u) != 0; };
    // the map (index into maps) and whether an enabled term reaches it, in the order of the result
    const int src[6] = {0, 1, 2, 4, 5, 6};
    const bool reached[6] = {bit(R3DG_REG_MASK_ENTROPY),
                             bit(R3DG_REG_DEPTH),
                             bit(R3DG_REG_NORMAL_RENDER_DEPTH) || bit(R3DG_REG_NORMAL_MVS_DEPTH),
                             bit(R3DG_REG_BASE_COLOR) || bit(R3DG_REG_BASE_COLOR_SMOOTH),
                             bit(R3DG_REG_ROUGHNESS_SMOOTH),
                             bit(R3DG_REG_METALLIC_SMOOTH)};
    std::vector<std::optional<torch::Tensor>> out(6);
    r3dg_reg_loss_grads g{};
    g.struct_size = sizeof(r3dg_reg_loss_grads);
    float** dst[6] = {&g.opacity, &g.depth, &g.normal, &g.base_color, &g.roughness, &g.metallic};
    for (int i = 0; i < 6; ++i) {
        if (!(want >> i & 1) || !reached[i] || !a.keep[src[i]].defined()) continue;
        out[i] = torch::empty_like(a.keep[src[i]]);
        if (out[i]->numel()) *dst[i] = out[i]->data_ptr<float>();
    }
    check(r3dg_reg_loss_backward(&a.in, cnt.data_ptr<int32_t>(), w.data_ptr<float>(),
                                 scale ? sc.data_ptr<float>() : nullptr, &g, stream_of(a.dev)),
          "reg_loss_backward");
    return out;
}

// trace_bvh_opacity (bvh/src/bvh.cu:87-117): outputs shaped like rays_o without its last axis
std::tuple<torch::Tensor, torch::Tensor> trace_bvh_opacity(const torch::Tensor& nodes, const torch::Tensor& aabbs,
                                                           const torch::Tensor& rays_o, const torch::Tensor& rays_d,
                                                           const torch::Tensor& means3D, const torch::Tensor& covs3D,
                                                           const torch::Tensor& opacities,
                                                           const torch::Tensor& normals) {
    TORCH_CHECK(nodes.is_cuda() && nodes.scalar_type() == torch::kInt32, "trace_bvh_opacity: nodes int32 on GPU");
    const auto o = cuda_f32(rays_o, "rays_o"), d = cuda_f32(rays_d, "rays_d");
    TORCH_CHECK(o.dim() >= 1 && o.size(-1) == 3 && d.numel() == o.numel(), "trace_bvh_opacity: rays [..., 3]");
    const int64_t R = o.numel() / 3;
    const c10::OptionalDeviceGuard guard(o.device());
    auto shape = o.sizes().slice(0, o.dim() - 1);
    auto contrib = torch::zeros(shape, o.options().dtype(torch::kInt32));
    auto vis = torch::ones(shape, o.options());
    const auto nd = nodes.contiguous(), bx = cuda_f32(aabbs, "aabbs"), m = cuda_f32(means3D, "means3D"),
               c = cuda_f32(covs3D, "covs3D"), op = cuda_f32(opacities, "opacities"), n = cuda_f32(normals, "normals");
    const int64_t P = m.numel() / 3;
    TORCH_CHECK(P >= 1 && nd.numel() == 5 * (2 * P - 1) && bx.numel() == 6 * (2 * P - 1) && c.numel() == 6 * P &&
                    op.numel() == P && n.numel() == 3 * P,
                "trace_bvh_opacity: tree / Gaussian shapes disagree");
    TensorAlloc scratch{o.options().dtype(torch::kUInt8), {}};
    check(r3dg_bvh_trace_opacity((int)R, (int)P, nd.data_ptr<int32_t>(), bx.data_ptr<float>(), o.data_ptr<float>(),
                                 d.data_ptr<float>(), m.data_ptr<float>(), c.data_ptr<float>(), op.data_ptr<float>(),
                                 n.data_ptr<float>(), contrib.data_ptr<int32_t>(), vis.data_ptr<float>(),
                                 tensor_alloc, &scratch, stream_of(o.device())),
          "trace_bvh_opacity");
    return {contrib, vis};
}

// ---- visibility baking (relightable3dgaussian_amd/visibility.py) -----------------------------------

// index [G] of any integer type on the rays' device -> contiguous int32
torch::Tensor index_i32(const torch::Tensor& index, const torch::Device& dev, const char* what) {
    TORCH_CHECK(index.is_cuda() && index.device() == dev, what, ": index must be on ", dev);
    TORCH_CHECK(index.dim() == 1 && (index.scalar_type() == torch::kInt32 || index.scalar_type() == torch::kInt64),
                what, ": index must be a 1-D int32 or int64 tensor");
    return index.to(torch::kInt32).contiguous();
}

// r3dg_bvh_trace_opacity_centres: rays from the centres of the Gaussians index names (all, without index).
// rays_d [G, Ns, 3] / [G * Ns, 3] given directions, or None for sample_num Fibonacci directions per entry.
// -> (contribute or None, visibility), shaped like rays_d without its last axis, [G, Ns] for Fibonacci rays
std::tuple<std::optional<torch::Tensor>, torch::Tensor> trace_bvh_opacity_centres(
    const torch::Tensor& nodes, const torch::Tensor& aabbs, const std::optional<torch::Tensor>& rays_d,
    const torch::Tensor& means3D, const torch::Tensor& covs3D, const torch::Tensor& opacities,
    const torch::Tensor& normals, const std::optional<torch::Tensor>& index, bool flip, int64_t sample_num,
    bool want_contribute) {
    const char* who = "trace_bvh_opacity_centres";
    TORCH_CHECK(nodes.is_cuda() && nodes.scalar_type() == torch::kInt32, who, ": nodes int32 on GPU");
    const auto nd = nodes.contiguous(), bx = cuda_f32(aabbs, "aabbs"), m = cuda_f32(means3D, "means3D"),
               c = cuda_f32(covs3D, "covs3D"), op = cuda_f32(opacities, "opacities"), n = cuda_f32(normals, "normals");
    const auto dev = m.device();
    const int64_t P = m.numel() / 3;
    TORCH_CHECK(P >= 1 && m.numel() == 3 * P && nd.numel() == 5 * (2 * P - 1) && bx.numel() == 6 * (2 * P - 1) &&
                    c.numel() == 6 * P && op.numel() == P && n.numel() == 3 * P,
                who, ": tree / Gaussian shapes disagree");
    for (const auto* t : {&nd, &bx, &c, &op, &n})
        TORCH_CHECK(t->device() == dev, who, ": every tensor must be on ", dev);
    TORCH_CHECK(sample_num >= 1, who, ": sample_num must be at least 1");
    torch::Tensor idx, d;
    int64_t G = P;
    if (index.has_value()) {
        idx = index_i32(*index, dev, who);
        G = idx.numel();
    }
    std::vector<int64_t> shape{G, sample_num};
    if (rays_d.has_value()) {
        d = cuda_f32(*rays_d, "rays_d");
        TORCH_CHECK(d.device() == dev && d.dim() >= 1 && d.size(-1) == 3, who, ": rays_d [..., 3] on ", dev);
        TORCH_CHECK(d.numel() == 3 * G * sample_num, who, ": rays_d must hold sample_num (", sample_num,
                    ") directions for each of the ", G, " ray origins");
        shape = d.sizes().slice(0, d.dim() - 1).vec();
    }
    const int64_t R = G * sample_num;
    TORCH_CHECK(R <= INT32_MAX, who, ": too many rays");
    const c10::OptionalDeviceGuard guard(dev);
    auto vis = torch::empty(shape, m.options());
    std::optional<torch::Tensor> contrib;
    if (want_contribute) contrib = torch::empty(shape, m.options().dtype(torch::kInt32));
    r3dg_centre_rays rays{};
    rays.struct_size = sizeof(rays);
    rays.num_rays = (int)R;
    rays.sample_num = (int)sample_num;
    rays.dirs = d.defined() ? d.data_ptr<float>() : nullptr;
    rays.index = idx.defined() ? idx.data_ptr<int32_t>() : nullptr;
    rays.flip = flip ? 1 : 0;
    TensorAlloc scratch{m.options().dtype(torch::kUInt8), {}};
    check(r3dg_bvh_trace_opacity_centres(&rays, (int)P, nd.data_ptr<int32_t>(), bx.data_ptr<float>(),
                                         m.data_ptr<float>(), c.data_ptr<float>(), op.data_ptr<float>(),
                                         n.data_ptr<float>(), contrib ? contrib->data_ptr<int32_t>() : nullptr,
                                         vis.data_ptr<float>(), tensor_alloc, &scratch, stream_of(dev)),
          who);
    return {contrib, vis};
}

// r3dg_fibonacci_dirs: normals [P, 3] -> [P, sample_num, 3]
torch::Tensor fibonacci_dirs(const torch::Tensor& normals, int64_t sample_num) {
    const auto n = cuda_f32(normals, "fibonacci_dirs");
    TORCH_CHECK(n.dim() == 2 && n.size(1) == 3, "fibonacci_dirs: normals [P, 3] expected");
    TORCH_CHECK(sample_num >= 1 && n.size(0) * sample_num <= INT32_MAX, "fibonacci_dirs: sample_num out of range");
    const c10::OptionalDeviceGuard guard(n.device());
    auto out = torch::empty({n.size(0), sample_num, 3}, n.options());
    check(r3dg_fibonacci_dirs((int)n.size(0), (int)sample_num, n.data_ptr<float>(), out.data_ptr<float>(),
                              stream_of(n.device())),
          "fibonacci_dirs");
    return out;
}

// the checked inputs of the visibility-SH loss; the tensors keep the made-contiguous copies alive
struct VisInputs {
    torch::Tensor dc, rest, dirs, traced, normals, index;
    r3dg_visibility_sh_inputs in;
};

VisInputs vis_inputs(const torch::Tensor& dc, const torch::Tensor& rest, const torch::Tensor& rays_d,
                     const torch::Tensor& traced, const std::optional<torch::Tensor>& normals,
                     const std::optional<torch::Tensor>& index, const char* who, bool in_place) {
    VisInputs v{};
    TORCH_CHECK(dc.is_cuda(), who, ": visibility_dc must be a GPU tensor (this build has no CPU path)");
    const auto dev = dc.device();
    auto f32 = [&](const torch::Tensor& t, const char* name) {
        TORCH_CHECK(t.is_cuda() && t.device() == dev, who, ": ", name, " must be on ", dev, ", got ", t.device());
        TORCH_CHECK(t.scalar_type() == torch::kFloat32, who, ": ", name, " must be float32");
        TORCH_CHECK(!in_place || t.is_contiguous(), who, ": ", name, " is updated in place and must be contiguous");
        return t.contiguous();
    };
    v.dc = f32(dc, "visibility_dc");
    v.rest = f32(rest, "visibility_rest");
    const int64_t P = v.dc.numel();
    TORCH_CHECK(P >= 1 && v.dc.dim() >= 1 && v.dc.size(0) == P, who, ": visibility_dc must be [P, 1, 1]");
    TORCH_CHECK(v.rest.dim() >= 1 && v.rest.size(0) == P && v.rest.numel() % P == 0, who,
                ": visibility_rest must be [P, K - 1, 1] with visibility_dc's P");
    const int64_t K = 1 + v.rest.numel() / P;
    in_place = false;
    v.dirs = f32(rays_d, "rays_d");
    v.traced = f32(traced, "traced");
    TORCH_CHECK(v.dirs.dim() >= 1 && v.dirs.size(-1) == 3, who, ": rays_d must be [R, 3]");
    const int64_t R = v.dirs.numel() / 3;
    TORCH_CHECK(v.traced.numel() == R, who, ": traced must hold one value per ray (", R, ")");
    if (normals.has_value()) {
        v.normals = f32(*normals, "normals");
        TORCH_CHECK(v.normals.numel() == 3 * P, who, ": normals must be [P, 3]");
    }
    if (index.has_value()) {
        v.index = index_i32(*index, dev, who);
        TORCH_CHECK(v.index.numel() == R, who, ": index must name one Gaussian per ray (", R, ")");
    } else {
        TORCH_CHECK(R == P, who, ": without index, rays_d must hold one ray per Gaussian (P = ", P, ", R = ", R, ")");
    }
    TORCH_CHECK(P <= INT32_MAX && R <= INT32_MAX && K <= INT32_MAX, who, ": sizes must fit an int");
    v.in = r3dg_visibility_sh_inputs{};
    v.in.struct_size = sizeof(v.in);
    v.in.P = (int)P; v.in.K = (int)K; v.in.R = (int)R;
    v.in.sh_dc = v.dc.data_ptr<float>();
    v.in.sh_rest = K > 1 ? v.rest.data_ptr<float>() : nullptr;
    v.in.dirs = R ? v.dirs.data_ptr<float>() : nullptr;
    v.in.traced = R ? v.traced.data_ptr<float>() : nullptr;
    v.in.normals = v.normals.defined() ? v.normals.data_ptr<float>() : nullptr;
    v.in.index = v.index.defined() && R ? v.index.data_ptr<int32_t>() : nullptr;
    return v;
}

// mean over the rays of |traced - clamp(eval_sh(sh[g], d) + 0.5, 0, 1)| -> 0-dim tensor
torch::Tensor visibility_sh_loss_forward(const torch::Tensor& dc, const torch::Tensor& rest,
                                         const torch::Tensor& rays_d, const torch::Tensor& traced,
                                         const std::optional<torch::Tensor>& normals,
                                         const std::optional<torch::Tensor>& index) {
    const auto v = vis_inputs(dc, rest, rays_d, traced, normals, index, "visibility_sh_loss_forward", false);
    const c10::OptionalDeviceGuard guard(v.dc.device());
    auto loss = torch::empty({}, v.dc.options());
    TensorAlloc scratch{v.dc.options().dtype(torch::kUInt8), {}};
    check(r3dg_visibility_sh_loss_forward(&v.in, loss.data_ptr<float>(), tensor_alloc, &scratch,
                                          stream_of(v.dc.device())),
          "visibility_sh_loss_forward");
    return loss;
}

// -> (grad visibility_dc, grad visibility_rest), dense; upstream is a device scalar (no host read)
std::tuple<torch::Tensor, torch::Tensor> visibility_sh_loss_backward(
    const torch::Tensor& dc, const torch::Tensor& rest, const torch::Tensor& rays_d, const torch::Tensor& traced,
    const std::optional<torch::Tensor>& normals, const std::optional<torch::Tensor>& index,
    const torch::Tensor& upstream) {
    const auto v = vis_inputs(dc, rest, rays_d, traced, normals, index, "visibility_sh_loss_backward", false);
    TORCH_CHECK(upstream.is_cuda() && upstream.device() == v.dc.device() && upstream.numel() == 1 &&
                    upstream.scalar_type() == torch::kFloat32,
                "visibility_sh_loss_backward: upstream must be one float32 on the inputs' device");
    const c10::OptionalDeviceGuard guard(v.dc.device());
    auto gdc = torch::empty_like(v.dc), grest = torch::empty_like(v.rest);
    check(r3dg_visibility_sh_loss_backward(&v.in, upstream.data_ptr<float>(), gdc.data_ptr<float>(),
                                           v.in.K > 1 ? grest.data_ptr<float>() : nullptr, stream_of(v.dc.device())),
          "visibility_sh_loss_backward");
    return {gdc, grest};
}

// one fused fit step (gradient + Adam, in place) over one ray per Gaussian; the mean L1 before the step goes
// to losses[slot]
void visibility_sh_fit_step(torch::Tensor dc, torch::Tensor rest, const torch::Tensor& rays_d,
                            const torch::Tensor& traced, const std::optional<torch::Tensor>& normals,
                            torch::Tensor exp_avg_dc, torch::Tensor exp_avg_rest, torch::Tensor exp_avg_sq_dc,
                            torch::Tensor exp_avg_sq_rest, int64_t step, double lr, double beta1, double beta2,
                            double eps, torch::Tensor losses, int64_t slot) {
    const char* who = "visibility_sh_fit_step";
    const auto v = vis_inputs(dc, rest, rays_d, traced, normals, std::nullopt, who, true);
    auto state = [&](const torch::Tensor& t, const torch::Tensor& like, const char* name) {
        TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == torch::kFloat32 &&
                        t.is_contiguous() && t.numel() == like.numel(),
                    who, ": ", name, " must be a contiguous float32 tensor of its parameter's size and device");
        return t.data_ptr<float>();
    };
    TORCH_CHECK(losses.is_cuda() && losses.device() == v.dc.device() && losses.scalar_type() == torch::kFloat32 &&
                    losses.is_contiguous() && slot >= 0 && slot < losses.numel(),
                who, ": losses must be a contiguous float32 tensor on the inputs' device holding slot ", slot);
    TORCH_CHECK(step >= 1 && step <= INT32_MAX, who, ": step must be >= 1");
    r3dg_visibility_fit fit{};
    fit.struct_size = sizeof(fit);
    fit.exp_avg_dc = state(exp_avg_dc, v.dc, "exp_avg_dc");
    fit.exp_avg_sq_dc = state(exp_avg_sq_dc, v.dc, "exp_avg_sq_dc");
    fit.exp_avg_rest = v.in.K > 1 ? state(exp_avg_rest, v.rest, "exp_avg_rest") : nullptr;
    fit.exp_avg_sq_rest = v.in.K > 1 ? state(exp_avg_sq_rest, v.rest, "exp_avg_sq_rest") : nullptr;
    fit.step = (int)step;
    fit.lr = (float)lr;
    fit.beta1 = beta1; fit.beta2 = beta2; fit.eps = eps;
    const c10::OptionalDeviceGuard guard(v.dc.device());
    TensorAlloc scratch{v.dc.options().dtype(torch::kUInt8), {}};
    check(r3dg_visibility_sh_fit_step(&v.in, &fit, losses.data_ptr<float>() + slot, tensor_alloc, &scratch,
                                      stream_of(v.dc.device())),
          who);
}

struct MultiAllocBvh {
    torch::TensorOptions opts;
    std::vector<torch::Tensor> ts;
};
void* multi_alloc_bvh(void* ctx, size_t n) {
    auto* a = static_cast<MultiAllocBvh*>(ctx);
    a->ts.push_back(torch::empty({(int64_t)std::max<size_t>(n, 256)}, a->opts));
    return a->ts.back().data_ptr();
}

// trace_bvh (bvh/src/bvh.cu:28-85)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> trace_bvh(
    const torch::Tensor& nodes, const torch::Tensor& aabbs, const torch::Tensor& rays_o, const torch::Tensor& rays_d,
    const torch::Tensor& means3D, const torch::Tensor& covs3D, const torch::Tensor& opacities) {
    (void)covs3D;
    (void)opacities;  // unused by the reference's arithmetic (trace.cu:123-124 commented out)
    TORCH_CHECK(nodes.is_cuda() && nodes.scalar_type() == torch::kInt32, "trace_bvh: nodes int32 on GPU");
    const auto o = cuda_f32(rays_o, "rays_o"), d = cuda_f32(rays_d, "rays_d");
    const int64_t R = o.size(0);
    TORCH_CHECK(o.numel() == 3 * R && d.numel() == 3 * R, "trace_bvh: rays [R, 3]");
    const c10::OptionalDeviceGuard guard(o.device());
    const auto iopt = o.options().dtype(torch::kInt32);
    auto contrib = torch::zeros({R, 1}, iopt);
    const auto nd = nodes.contiguous(), bx = cuda_f32(aabbs, "aabbs"), m = cuda_f32(means3D, "means3D");
    const int64_t P = m.numel() / 3;
    TORCH_CHECK(P >= 1 && nd.numel() == 5 * (2 * P - 1) && bx.numel() == 6 * (2 * P - 1),
                "trace_bvh: tree shapes disagree");
    MultiAllocBvh al{o.options().dtype(torch::kUInt8), {}};
    int L = 0;
    int32_t *pt = nullptr, *rid = nullptr;
    float* pos = nullptr;
    check(r3dg_bvh_trace((int)R, (int)P, nd.data_ptr<int32_t>(), bx.data_ptr<float>(), o.data_ptr<float>(), d.data_ptr<float>(),
                         m.data_ptr<float>(), contrib.data_ptr<int32_t>(), multi_alloc_bvh, &al, &L, &pt, &pos, &rid,
                         stream_of(o.device())),
          "trace_bvh");
    if (L == 0)  // the reference's empty shapes (bvh.cu:48-53), ray_id_list float [0, 3] included
        return {contrib, torch::zeros({0, 1}, iopt), torch::zeros({0, 3}, o.options()), torch::zeros({0, 3}, o.options())};
    auto view = [&](void* p, std::vector<int64_t> shape, torch::ScalarType t) {
        for (auto& b : al.ts)
            if (b.data_ptr() == p) return b.narrow(0, 0, L * (t == torch::kFloat32 ? 12 : 4)).view(t).view(shape);
        TORCH_CHECK(false, "trace_bvh: output not found");
        return torch::Tensor();
    };
    return {contrib, view(pt, {L, 1}, torch::kInt32), view(pos, {L, 3}, torch::kFloat32),
            view(rid, {L, 1}, torch::kInt32)};
}

}  // namespace


// r3dg_get_options / r3dg_set_options (include/r3dg_hip.h) as a dict of the option fields
#define R3DG_OPTION_FIELDS(X)                                                                         \
    X(bwd_reduce) X(prof_sort_markers) X(test_bwd_dpp) X(test_bwd_wterms) X(test_no_cull)              \
    X(test_bin_atomic) X(test_bin_blocks) X(test_tile_order_spatial) X(test_bwd_srs) X(test_bvh_lanes) \
    X(test_bvh_sort) X(test_bvh_split) X(test_bin_one_pass)
std::map<std::string, int64_t> get_options() {
    r3dg_options o{};
    o.struct_size = sizeof(o);
    check(r3dg_get_options(&o), "get_options");
    std::map<std::string, int64_t> d;
#define X(f) d[#f] = o.f;
    R3DG_OPTION_FIELDS(X)
#undef X
    return d;
}
// sets the given fields (the others keep their values); returns the previous options
std::map<std::string, int64_t> set_options(const std::map<std::string, int64_t>& kv) {
    r3dg_options o{};
    o.struct_size = sizeof(o);
    check(r3dg_get_options(&o), "set_options");
    const std::map<std::string, int64_t> prev = get_options();
    for (const auto& it : kv) {
        bool known = false;
#define X(f) if (it.first == #f) { o.f = (int)it.second; known = true; }
        R3DG_OPTION_FIELDS(X)
#undef X
        TORCH_CHECK(known, "set_options: unknown option ", it.first);
    }
    check(r3dg_set_options(&o), "set_options");
    return prev;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "MI355X-native relightable Gaussian-splat rasterizer (drop-in for r3dg_rasterization._C)";
    // the reference surface (ext.cu:21-35)
    m.def("rasterize_gaussians", &rasterize_gaussians);
    m.def("rasterize_gaussians_backward", &rasterize_gaussians_backward);
    m.def("render_equation_forward", &render_equation_forward);
    m.def("render_equation_forward_complex", &render_equation_forward_complex);
    m.def("render_equation_backward", &render_equation_backward);
    m.def("mark_visible", &mark_visible);
    m.def("GetSplatShaderAddressMap", []() { return shader_map(R3DG_SHADER_SPLAT); });
    m.def("GetShShaderAddressMap", []() { return shader_map(R3DG_SHADER_SH); });
    m.def("GetPostProcessShaderAddressMap", []() { return shader_map(R3DG_SHADER_POST); });
    m.def("PreprocessModel", &preprocess_model);
    m.def("EncodeTextureMode", [](const std::string& s) { return r3dg_encode_texture_mode(s.c_str()); });
    m.def("EncodeWrapMode", [](const std::string& s) { return r3dg_encode_wrap_mode(s.c_str()); });
    m.def("AllocateTexture", &allocate_texture);
    m.def("UploadTexturesToDevice", &upload_textures);
    // extensions
    m.def("rasterize_gaussians_backward_ex", &rasterize_gaussians_backward_ex);
    m.def("rasterize_gaussians_backward_chunked", &rasterize_gaussians_backward_chunked);
    m.def("rasterize_gaussians_backward_chunked_packed", &rasterize_gaussians_backward_chunked_packed);
    m.def("render_equation_forward_with_rand", &render_equation_forward_with_rand);
    // the relighting script's render equation and environment light (neilf_composite.py, envmap.py)
    m.def("render_equation_relight", &render_equation_relight);
    m.def("envmap_direct_light", &envmap_direct_light);
    m.def("rasterizer_state", &rasterizer_state);
    m.def("sh_color_grads", &sh_color_grads);
    m.def("sh_grad_from_views", &sh_grad_from_views);
    m.def("feature_groups", &feature_groups);
    m.def("create_shader_manager", &create_shader_manager);
    m.def("shader_manager_info", &shader_manager_info);
    m.def("abi_version", []() { return r3dg_abi_version(); });
    m.def("get_options", &get_options);
    m.def("set_options", &set_options);
    // training step on the device (§8f rank 3)
    m.def("adam_step", &adam_step);
    m.def("adam_step_groups", &adam_step_groups);
    m.def("densification_stats", &densification_stats);
    m.def("densify_and_prune", &densify_and_prune);
    m.def("reset_opacity", &reset_opacity);
    // parameter activations (relightable3dgaussian_amd/activation.py)
    m.def("activate_forward", &activate_forward, py::arg("P"), py::arg("widths"), py::arg("roles"),
          py::arg("role_groups"), py::arg("param"), py::arg("campos") = py::none(),
          py::arg("inverse_covariance") = false);
    m.def("activate_backward", &activate_backward, py::arg("P"), py::arg("widths"), py::arg("roles"),
          py::arg("role_groups"), py::arg("param"), py::arg("campos"), py::arg("upstreams"), py::arg("grad"),
          py::arg("accumulate") = false);
    // scene composition and the points capture (relightable3dgaussian_amd/compose.py, relight.render_points)
    m.def("set_transform", &set_transform);
    m.def("compose_object", &compose_object);
    m.def("render_points", &render_points);
    // BVH visibility tracer (§8f rank 4): the reference's bvh_tracing._C names + the leaf boxes
    m.def("create_bvh", &create_bvh);
    m.def("trace_bvh", &trace_bvh);
    m.def("trace_bvh_opacity", &trace_bvh_opacity);
    m.def("bvh_leaf_aabbs", &bvh_leaf_aabbs);
    // visibility baking (relightable3dgaussian_amd/visibility.py): rays from Gaussian centres, the
    // visibility-SH loss and the fused fit step
    m.def("trace_bvh_opacity_centres", &trace_bvh_opacity_centres, py::arg("nodes"), py::arg("aabbs"),
          py::arg("rays_d"), py::arg("means3D"), py::arg("covs3D"), py::arg("opacities"), py::arg("normals"),
          py::arg("index") = py::none(), py::arg("flip") = true, py::arg("sample_num") = 1,
          py::arg("want_contribute") = true);
    m.def("fibonacci_dirs", &fibonacci_dirs);
    m.def("visibility_sh_loss_forward", &visibility_sh_loss_forward);
    m.def("visibility_sh_loss_backward", &visibility_sh_loss_backward);
    m.def("visibility_sh_fit_step", &visibility_sh_fit_step);
    // nearest-neighbour distances: the reference's simple_knn._C (submodules/simple-knn/ext.cpp)
    m.def("distCUDA2", &dist_cuda2);
    // the fused L1 + SSIM image loss (relightable3dgaussian_amd/loss.py)
    m.def("image_loss_forward", &image_loss_forward, py::arg("img"), py::arg("gt"), py::arg("hwc"),
          py::arg("need_grad"));
    m.def("image_loss_backward", &image_loss_backward, py::arg("img"), py::arg("gt"), py::arg("hwc"),
          py::arg("dmaps"), py::arg("w_ssim"), py::arg("w_abs"), py::arg("scale") = py::none());
    // the fused depth / mask / normal / base-colour / smoothness terms (relightable3dgaussian_amd/loss.py)
    m.def("reg_loss_forward", &reg_loss_forward, py::arg("maps"), py::arg("H"), py::arg("W"), py::arg("terms"),
          py::arg("hwc"));
    m.def("reg_loss_backward", &reg_loss_backward, py::arg("maps"), py::arg("H"), py::arg("W"), py::arg("terms"),
          py::arg("hwc"), py::arg("depth_count"), py::arg("weights"), py::arg("scale") = py::none(),
          py::arg("want") = 63);
    m.def("image_loss_window", []() {
        const float* w = r3dg_image_loss_window();
        return std::vector<float>(w, w + 11);
    });
    m.def("profile_enable", [](int64_t n) { check(r3dg_profile_enable((int)n), "profile_enable"); });
    m.def("profile_read", [](int64_t kernel) {
        int c = 0;
        float ms = 0.f;
        check(r3dg_profile_read((int)kernel, &c, &ms), "profile_read");
        return std::make_tuple((int64_t)c, (double)ms);
    });
}
