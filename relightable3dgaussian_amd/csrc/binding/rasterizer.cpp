// rasterizer.cpp -- the rasterizer's forward and backward, the state accessor, the view-parallel SH
// exchange, mark_visible, shader managers, textures, options and profiling.
#include "binding.h"

using namespace binding;

namespace {

using FwdResult = std::tuple<int, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor,
                             Tensor, Tensor>;

// RasterizeGaussiansCUDA (rasterize_points.cu:39-181)
FwdResult rasterize_gaussians(const Tensor& background, double time, double dt, const Tensor& means3D,
                              const Tensor& features, const Tensor& colors, const Tensor& opacity, const Tensor& scales,
                              const Tensor& rotations, double scale_modifier, const Tensor& cov3D_precomp,
                              const Tensor& viewmatrix, const Tensor& viewmatrix_inv, const Tensor& projmatrix,
                              const Tensor& projmatrix_inv, double tan_fovx, double tan_fovy, double cx, double cy,
                              int64_t image_height, int64_t image_width, const Tensor& sh, int64_t degree,
                              const Tensor& campos, bool prefiltered, bool computer_pseudo_normal,
                              std::optional<int64_t> d_textureManager_ptr, std::optional<int64_t> h_shShaderManager_ptr,
                              std::optional<int64_t> h_splatShaderManager_ptr,
                              std::optional<std::vector<int64_t>> postProcessingPasses, bool debug) {
    if (means3D.ndimension() != 2 || means3D.size(1) != 3)
        throw std::runtime_error("means3D must have dimensions (num_points, 3)");
    const Call call("rasterize_gaussians", means3D, "means3D");
    const int P = (int)means3D.size(0);
    const int S = features.numel() == 0 && features.dim() < 2 ? 0 : (int)features.size(1);
    const int H = (int)image_height, W = (int)image_width;
    const auto fopt = call.options();

    auto m3 = call.moved(means3D, "means3D"), ft = call.moved(features, "features"), co = call.moved(colors, "colors");
    auto op = call.moved(opacity, "opacity"), sc = call.moved(scales, "scales"), ro = call.moved(rotations, "rotations");
    auto c3 = call.moved(cov3D_precomp, "cov3D_precomp"), shc = call.moved(sh, "sh");
    auto bg = call.moved(background, "background"), vm = call.moved(viewmatrix, "viewmatrix");
    auto vmi = call.moved(viewmatrix_inv, "viewmatrix_inv"), pm = call.moved(projmatrix, "projmatrix");
    auto pmi = call.moved(projmatrix_inv, "projmatrix_inv"), cp = call.moved(campos, "campos");

    Tensor out_color = torch::empty({H, W, 3}, fopt);
    Tensor out_opacity = torch::empty({H, W, 1}, fopt);
    Tensor out_depth = torch::empty({H, W, 1}, fopt);
    Tensor out_stencil = torch::empty({H, W, 1}, fopt);
    Tensor out_feature = torch::empty({H, W, S}, fopt);
    Tensor out_shader = torch::empty({H, W, 3}, fopt);
    Tensor out_normal = torch::empty({H, W, 3}, fopt);
    Tensor out_xyz = torch::empty({H, W, 3}, fopt);
    Tensor radii = torch::empty({P}, call.options(torch::kInt32));

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
    // the three state buffers are one allocation each and go to the caller; the binning's tile counts
    // (hist) are transient
    Scratch geom(call), binning(call), image(call), hist(call);
    check(r3dg_rasterize_gaussians_ex(&s, &g, &o, Scratch::alloc, &geom, Scratch::alloc, &binning, Scratch::alloc, &image,
                                      Scratch::alloc, &hist, &rendered, call.stream()),
          call.who);
    // n_contrib is a view into the image state buffer (reference: from_blob, rasterize_points.cu:179)
    const int64_t off = (int64_t)r3dg_image_state_n_contrib_offset(H, W);
    const Tensor img = image.buffer();
    Tensor n_contrib = img.narrow(0, off, (int64_t)H * W * 4).view(torch::kInt32).view({H, W, 1});
    return {rendered, n_contrib, out_color, out_opacity, out_depth, out_stencil, out_feature, out_shader,
            out_normal, out_xyz, radii, geom.buffer(), binning.buffer(), img};
}

using BwdResult = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;

// What the four bound backward names differ in, read from what follows `debug` in the Python call.
struct BwdVariant {
    int64_t H, W;                   // image size
    bool color_hwc, feature_native; // the upstream gradients are in the forward's own output layouts
    int64_t n_chunks = 1;           // chunked delivery (include/r3dg_hip.h r3dg_backward_outputs)
    py::object chunk_cb = py::none();
    bool packed_dense = false;
};
using BwdVariantFn = BwdVariant (*)(const Tensor& dL_dout_color, const py::args& extra);

// RasterizeGaussiansBackwardCUDA (rasterize_points.cu:183-275): grads are CHW / planar, H and W theirs.
BwdVariant variant_reference(const Tensor& dL_dout_color, const py::args& extra) {
    TORCH_CHECK(extra.size() == 0, "rasterize_gaussians_backward: takes 26 arguments");
    return {dL_dout_color.size(1), dL_dout_color.size(2), false, false};
}
// Same, taking the forward's own output layouts (HWC colour, native feature layout): the shipped
// autograd wrapper uses this so no transposes are needed. (..., H, W)
BwdVariant variant_ex(const Tensor&, const py::args& extra) {
    TORCH_CHECK(extra.size() == 2, "rasterize_gaussians_backward_ex: takes H, W after debug");
    return {extra[0].cast<int64_t>(), extra[1].cast<int64_t>(), true, true};
}
// With chunked delivery: chunk_cb(chunk, g_begin, g_end, outputs) is called once the gradients of
// Gaussians [g_begin, g_end) are enqueued (outputs = the 9 result tensors), e.g. to start their
// all-reduce on a communication stream (view_parallel.py).
// (..., H, W, color_hwc, feature_native, n_chunks, chunk_cb)
BwdVariant variant_chunked(const Tensor&, const py::args& extra) {
    TORCH_CHECK(extra.size() == 6, "rasterize_gaussians_backward_chunked: takes H, W, color_hwc, feature_native, "
                                   "n_chunks, chunk_cb after debug");
    return {extra[0].cast<int64_t>(), extra[1].cast<int64_t>(), extra[2].cast<bool>(), extra[3].cast<bool>(),
            extra[4].cast<int64_t>(), extra[5].cast<py::object>()};
}
// Chunked with the dense gradients packed (packed_dense below): the callback's outputs carry a 10th
// tensor, the [P, 11 + S] array whose rows [g_begin, g_end) hold the chunk's means3D / opacity / scales /
// rotations / features gradients contiguously.
BwdVariant variant_chunked_packed(const Tensor& dL_dout_color, const py::args& extra) {
    BwdVariant v = variant_chunked(dL_dout_color, extra);
    v.packed_dense = true;
    return v;
}

// The backward under one of its four names: the 26 parameters they share, then the variant's own.
auto backward(BwdVariantFn variant) {
    return [variant](const Tensor& background, const Tensor& means3D, const Tensor& features, const Tensor& radii,
                     const Tensor& colors, const Tensor& scales, const Tensor& rotations, double scale_modifier,
                     const Tensor& cov3D_precomp, const Tensor& viewmatrix, const Tensor& projmatrix, double tan_fovx,
                     double tan_fovy, const Tensor& dL_dout_color, const Tensor& dL_dout_opacity,
                     const Tensor& dL_dout_depth, const Tensor& dL_dout_feature, const Tensor& sh, int64_t degree,
                     const Tensor& campos, const Tensor& geomBuffer, int64_t R, const Tensor& binningBuffer,
                     const Tensor& imageBuffer, bool backward_geometry, bool debug, const py::args& extra) -> BwdResult {
        const BwdVariant v = variant(dL_dout_color, extra);
        const Call call("rasterize_gaussians_backward", means3D, "means3D");
        const int P = (int)means3D.size(0);
        const int S = features.numel() == 0 && features.dim() < 2 ? 0 : (int)features.size(1);
        const int M = sh.numel() == 0 ? 0 : (int)sh.size(1);
        const auto fopt = call.options();
        // packed_dense: the five dense gradients are column views of one [P, 11 + S] array (means3D 3,
        // opacity 1, scales 3, rotations 4, features S), so a Gaussian range of them is one contiguous
        // span (r3dg_backward_outputs.dense_stride; one collective per chunk in view_parallel.py)
        const int DW = 11 + S;
        Tensor dense = v.packed_dense ? torch::empty({P, DW}, fopt) : Tensor();
        Tensor dL_dmeans3D = v.packed_dense ? dense.narrow(1, 0, 3) : torch::empty({P, 3}, fopt);
        Tensor dL_dmeans2D = torch::empty({P, 3}, fopt);
        Tensor dL_dfeatures = v.packed_dense ? dense.narrow(1, 11, S) : torch::empty({P, S}, fopt);
        Tensor dL_dcolors = torch::empty({P, 3}, fopt);
        Tensor dL_dopacity = v.packed_dense ? dense.narrow(1, 3, 1) : torch::empty({P, 1}, fopt);
        Tensor dL_dcov3D = torch::empty({P, 6}, fopt);
        Tensor dL_dsh = torch::empty({P, M, 3}, fopt);
        Tensor dL_dscales = v.packed_dense ? dense.narrow(1, 4, 3) : torch::empty({P, 3}, fopt);
        Tensor dL_drotations = v.packed_dense ? dense.narrow(1, 7, 4) : torch::empty({P, 4}, fopt);
        const BwdResult result{dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D,  dL_dfeatures,
                               dL_dcov3D,   dL_dsh,     dL_dscales,  dL_drotations};
        if (P == 0) return result;

        auto m3 = call.moved(means3D, "means3D"), ft = call.moved(features, "features"), co = call.moved(colors, "colors");
        auto sc = call.moved(scales, "scales"), ro = call.moved(rotations, "rotations");
        auto c3 = call.moved(cov3D_precomp, "cov3D_precomp"), shc = call.moved(sh, "sh");
        auto bg = call.moved(background, "background"), vm = call.moved(viewmatrix, "viewmatrix");
        auto pm = call.moved(projmatrix, "projmatrix"), cp = call.moved(campos, "campos");
        auto gc = call.moved(dL_dout_color, "dL_dout_color"), go = call.moved(dL_dout_opacity, "dL_dout_opacity");
        auto gd = call.moved(dL_dout_depth, "dL_dout_depth"), gf = call.moved(dL_dout_feature, "dL_dout_feature");
        auto rad = call.moved(radii, "radii", torch::kInt32);
        // the forward's state buffers, as it returned them
        void* geom = call.in_place<uint8_t>(geomBuffer, "geomBuffer");
        void* binning = call.in_place<uint8_t>(binningBuffer, "binningBuffer");
        void* image = call.in_place<uint8_t>(imageBuffer, "imageBuffer");

        r3dg_raster_settings s{};
        s.struct_size = sizeof(s);
        s.P = P; s.S = S; s.D = (int)degree; s.M = M; s.W = (int)v.W; s.H = (int)v.H;
        s.tan_fovx = (float)tan_fovx; s.tan_fovy = (float)tan_fovy; s.scale_modifier = (float)scale_modifier;
        s.debug = debug;
        s.bg = bg.data_ptr<float>(); s.viewmatrix = vm.data_ptr<float>(); s.projmatrix = pm.data_ptr<float>();
        s.campos = cp.data_ptr<float>();
        r3dg_gaussians g{};
        g.means3D = m3.data_ptr<float>(); g.features = opt_ptr(ft); g.colors_precomp = opt_ptr(co);
        g.scales = opt_ptr(sc); g.rotations = opt_ptr(ro); g.cov3D_precomp = opt_ptr(c3); g.sh = opt_ptr(shc);
        r3dg_backward_grads gr{};
        gr.dL_dout_color = gc.data_ptr<float>(); gr.color_hwc = v.color_hwc;
        gr.dL_dout_opacity = go.data_ptr<float>(); gr.dL_dout_depth = gd.data_ptr<float>();
        gr.dL_dout_feature = S > 0 ? gf.data_ptr<float>() : nullptr; gr.feature_native = v.feature_native;
        r3dg_backward_outputs o{};
        o.struct_size = sizeof(o);
        o.dL_dmeans2D = dL_dmeans2D.data_ptr<float>(); o.dL_dcolors = dL_dcolors.data_ptr<float>();
        o.dL_dopacity = dL_dopacity.data_ptr<float>(); o.dL_dmeans3D = dL_dmeans3D.data_ptr<float>();
        o.dL_dfeatures = S > 0 ? dL_dfeatures.data_ptr<float>() : nullptr; o.dL_dcov3D = dL_dcov3D.data_ptr<float>();
        o.dL_dsh = M > 0 ? dL_dsh.data_ptr<float>() : nullptr; o.dL_dscales = dL_dscales.data_ptr<float>();
        o.dL_drotations = dL_drotations.data_ptr<float>();
        o.dense_stride = v.packed_dense ? DW : 0;
        // chunked delivery: the Python callable runs (GIL held: we are inside the pybind call) after
        // each Gaussian range's kernels are enqueued; an exception is re-raised after the C call
        struct ChunkCtx {
            const py::object* cb;
            py::tuple outs;  // the 9 output tensors (and the packed array), handed to the callback
            bool failed = false;
            std::string what;
        } cctx{&v.chunk_cb, py::tuple()};
        o.n_chunks = (int)v.n_chunks;
        if (!v.chunk_cb.is_none()) {
            cctx.outs = v.packed_dense ? py::tuple(py::cast(std::tuple_cat(result, std::make_tuple(dense))))
                                       : py::tuple(py::cast(result));
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
        Scratch scratch(call);
        check(r3dg_rasterize_gaussians_backward(&s, &g, rad.data_ptr<int>(), &gr, geom, binning, image, (int)R,
                                                backward_geometry, Scratch::alloc, &scratch, &o, call.stream()),
              call.who);
        TORCH_CHECK(!cctx.failed, call.who, ": chunk callback raised: ", cctx.what);
        return result;
    };
}

// View-parallel SH-gradient exchange (include/r3dg_hip.h): this view's clamp-masked colour
// gradients of Gaussians [g0, g1) (the rank's all-gather payload) ...
Tensor sh_color_grads(const Tensor& geomBuffer, int64_t P, const Tensor& dL_dcolors, int64_t g0, int64_t g1) {
    const Call call("sh_color_grads", dL_dcolors, "dL_dcolors");
    const float* grads = call.in_place(dL_dcolors, "dL_dcolors");
    TORCH_CHECK(dL_dcolors.numel() == 3 * P && 0 <= g0 && g0 <= g1 && g1 <= P,
                "sh_color_grads: dL_dcolors must be a [P,3] tensor, 0 <= g0 <= g1 <= P");
    void* geom = call.in_place<uint8_t>(geomBuffer, "geomBuffer");
    TORCH_CHECK((size_t)geomBuffer.nbytes() >= r3dg_geom_state_bytes((int)P, -1),
                "sh_color_grads: geomBuffer must be the forward's geometry state for these P Gaussians");
    auto out = torch::empty({g1 - g0, 3}, dL_dcolors.options());
    check(r3dg_sh_color_grads((int)P, (int)g0, (int)(g1 - g0), geom, grads, out.data_ptr<float>(), call.stream()),
          call.who);
    return out;
}

// ... and the sum over the N views of their SH gradients, rebuilt from the gathered [N, n, 3]
// colour gradients and the views' camera centres [N, 3], into rows [g0, g0 + n) of dL_dsh.
void sh_grad_from_views(const Tensor& means3D, const Tensor& campos, const Tensor& drgb, int64_t degree, int64_t g0,
                        Tensor& dL_dsh) {
    const Call call("sh_grad_from_views", means3D, "means3D");
    TORCH_CHECK(drgb.dim() == 3 && drgb.size(2) == 3 && campos.dim() == 2 && campos.size(1) == 3 &&
                    campos.size(0) == drgb.size(0) && dL_dsh.dim() == 3 && dL_dsh.size(2) == 3 && g0 >= 0 &&
                    g0 + drgb.size(1) <= dL_dsh.size(0),
                "sh_grad_from_views: drgb [N,n,3], campos [N,3], dL_dsh [P,M,3]");
    TORCH_CHECK(means3D.dim() == 2 && means3D.size(1) == 3 && means3D.size(0) >= g0 + drgb.size(1),
                "sh_grad_from_views: means3D must be [P,3] with P >= g0 + n");
    TORCH_CHECK(dL_dsh.size(1) <= 16 && degree >= 0 && degree <= 3 && (degree + 1) * (degree + 1) <= dL_dsh.size(1),
                "sh_grad_from_views: degree 0..3 with (degree+1)^2 <= M <= 16");
    float* out = call.in_place(dL_dsh, "dL_dsh");
    auto m3 = call.moved(means3D, "means3D"), cp = call.moved(campos, "campos"), d = call.moved(drgb, "drgb");
    check(r3dg_sh_grad_from_views((int)g0, (int)drgb.size(1), (int)degree, (int)dL_dsh.size(1), (int)drgb.size(0),
                                  m3.data_ptr<float>(), cp.data_ptr<float>(), d.data_ptr<float>(), out, call.stream()),
          call.who);
}

Tensor mark_visible(Tensor& means3D, Tensor& viewmatrix, Tensor& projmatrix) {
    const Call call("mark_visible", means3D, "means3D");
    const int P = (int)means3D.size(0);
    Tensor present = torch::zeros({P}, call.options(torch::kBool));
    if (P == 0) return present;
    auto m3 = call.moved(means3D, "means3D"), vm = call.moved(viewmatrix, "viewmatrix");
    auto pm = call.moved(projmatrix, "projmatrix");
    check(r3dg_mark_visible(P, m3.data_ptr<float>(), vm.data_ptr<float>(), pm.data_ptr<float>(),
                            (uint8_t*)present.data_ptr<bool>(), call.stream()),
          call.who);
    return present;
}

std::map<std::string, int64_t> shader_map(int kind) {
    std::map<std::string, int64_t> m;
    for (int i = 0; i < r3dg_shader_count(kind); ++i) m[r3dg_shader_name(kind, i)] = r3dg_shader_handle(kind, i);
    return m;
}

std::tuple<int64_t, int64_t> preprocess_model(Tensor& xyz) {
    const Call call("PreprocessModel", xyz, "xyz");
    auto x = call.moved(xyz, "xyz");
    int64_t a = 0, b = 0;
    check(r3dg_preprocess_model((int)xyz.size(0), opt_ptr(x), &a, &b, call.stream()), call.who);
    return {a, b};
}

// handles: host data by design (any device, any integer type), read here; the manager is built on the
// current device
int64_t create_shader_manager(int64_t kind, const Tensor& handles) {
    auto h = handles.to(torch::kCPU).to(torch::kInt64).contiguous();
    int64_t m = 0;
    check(r3dg_create_shader_manager((int)kind, (int)h.numel(), h.data_ptr<int64_t>(), &m,
                                     (r3dg_stream_t)c10::hip::getCurrentHIPStream().stream()),
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
// float, height, width, encoding_mode, wrap_modes [2], normalizedCoords (CPU int32 tensors). Host
// data by design: the pixels are converted and uploaded here.
int64_t allocate_texture(const std::map<std::string, Tensor>& d) {
    auto scalar = [&](const char* k, int i = 0) {
        auto it = d.find(k);
        if (it == d.end()) throw std::runtime_error(std::string("AllocateTexture: missing '") + k + "'");
        return it->second.to(torch::kCPU).to(torch::kInt64).contiguous().data_ptr<int64_t>()[i];
    };
    auto it = d.find("pixelData");
    if (it == d.end()) throw std::runtime_error("AllocateTexture: missing 'pixelData'");
    Tensor pix = it->second.to(torch::kFloat32).contiguous();
    if (!pix.is_cuda()) pix = pix.cuda();
    const int H = (int)scalar("height"), W = (int)scalar("width"), mode = (int)scalar("encoding_mode");
    const int C = pix.numel() / std::max<int64_t>((int64_t)H * W, 1);
    if ((int64_t)C * H * W != pix.numel()) throw std::runtime_error("AllocateTexture: pixelData is not [H, W, C]");
    const Call call("AllocateTexture", pix, "pixelData");
    int64_t h = 0;
    check(r3dg_texture_create(pix.data_ptr<float>(), W, H, mode, (int)scalar("wrap_modes", 0),
                              (int)scalar("wrap_modes", 1), (int)scalar("normalizedCoords"), &h, call.stream()),
          call.who);
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
std::vector<Tensor> rasterizer_state(const Tensor& geomBuffer, const Tensor& binningBuffer, const Tensor& imageBuffer,
                                     int64_t P, int64_t H, int64_t W, int64_t L) {
    const Call call("rasterizer_state", geomBuffer, "geomBuffer");
    r3dg_binning_view v{};
    check(r3dg_state_view((int)P, (int)H, (int)W, (int)L, call.in_place<uint8_t>(geomBuffer, "geomBuffer"),
                          call.in_place<uint8_t>(binningBuffer, "binningBuffer"),
                          call.in_place<uint8_t>(imageBuffer, "imageBuffer"), &v),
          call.who);
    auto slice = [](const Tensor& buf, const void* p, int64_t nbytes) {
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

}  // namespace

void bind_rasterizer(py::module_& m) {
    // the reference surface (ext.cu:21-35)
    m.def("rasterize_gaussians", &rasterize_gaussians);
    m.def("rasterize_gaussians_backward", backward(variant_reference));
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
    m.def("rasterize_gaussians_backward_ex", backward(variant_ex));
    m.def("rasterize_gaussians_backward_chunked", backward(variant_chunked));
    m.def("rasterize_gaussians_backward_chunked_packed", backward(variant_chunked_packed));
    m.def("rasterizer_state", &rasterizer_state);
    m.def("sh_color_grads", &sh_color_grads);
    m.def("sh_grad_from_views", &sh_grad_from_views);
    m.def("feature_groups", &feature_groups);
    m.def("create_shader_manager", &create_shader_manager);
    m.def("shader_manager_info", &shader_manager_info);
    m.def("abi_version", []() { return r3dg_abi_version(); });
    m.def("get_options", &get_options);
    m.def("set_options", &set_options);
    m.def("profile_enable", [](int64_t n) { check(r3dg_profile_enable((int)n), "profile_enable"); });
    m.def("profile_read", [](int64_t kernel) {
        int c = 0;
        float ms = 0.f;
        check(r3dg_profile_read((int)kernel, &c, &ms), "profile_read");
        return std::make_tuple((int64_t)c, (double)ms);
    });
}
