// losses.cpp -- the training losses: the fused L1 + SSIM image loss, the image-space regularisers, and
// the visibility-SH loss with its fused fit step.
#include "binding.h"

using namespace binding;

namespace {

// ---- image loss (utils/loss_utils.py:31-62 ssim, neilf.py:216-222) --------------------------------

// img: [..., H, W] planes (hwc false) or the rasterizer's [H, W, C] (hwc true); gt always [..., H, W]
// with as many planes. The checked, contiguous pair, the geometry the C ABI wants, and the call on img's
// device (built once type and shape are known good: a mistyped or misshapen pair is reported as such
// wherever it lives).
struct LossImages {
    std::optional<Call> call;
    Tensor img, gt;
    int64_t planes, H, W, img_stride[3];

    LossImages(const Tensor& img_in, const Tensor& gt_in, bool hwc, const char* what) {
        TORCH_CHECK(img_in.scalar_type() == torch::kFloat32 && gt_in.scalar_type() == torch::kFloat32, what,
                    ": expected float32");
        TORCH_CHECK(gt_in.dim() >= 2, what, ": gt [..., H, W] expected");
        H = gt_in.size(-2);
        W = gt_in.size(-1);
        planes = H * W ? gt_in.numel() / (H * W) : 0;
        if (hwc) {
            TORCH_CHECK(img_in.dim() == 3 && gt_in.dim() == 3 && img_in.size(0) == H && img_in.size(1) == W &&
                            img_in.size(2) == gt_in.size(0),
                        what, ": shape mismatch: img [H,W,C] against gt [C,H,W] expected");
            img_stride[0] = 1, img_stride[1] = W * planes, img_stride[2] = planes;
        } else {
            TORCH_CHECK(img_in.sizes() == gt_in.sizes(), what, ": shape mismatch between img and gt");
            img_stride[0] = H * W, img_stride[1] = W, img_stride[2] = 1;
        }
        TORCH_CHECK(gt_in.numel() <= (int64_t)INT32_MAX, what, ": planes * H * W exceeds int32");
        call.emplace(what, img_in, "img");
        img = call->on_device(img_in, "img");
        gt = call->on_device(gt_in, "gt");
    }
};

// -> (sums [planes, 3]: per plane the sums of ssim_map, |img - gt|, (img - gt)^2; dmaps [3, planes, H, W]
// for image_loss_backward, or an empty tensor when need_grad is false)
std::tuple<Tensor, Tensor> image_loss_forward(const Tensor& img, const Tensor& gt, bool hwc, bool need_grad) {
    const LossImages a(img, gt, hwc, "image_loss_forward");
    const Call& call = *a.call;
    const auto fopt = call.options();
    auto sums = a.gt.numel() ? torch::empty({a.planes, 3}, fopt) : torch::zeros({a.planes, 3}, fopt);
    auto dmaps = need_grad ? torch::empty({3, a.planes, a.H, a.W}, fopt) : torch::empty({0}, fopt);
    Scratch scratch(call);
    check(r3dg_image_loss_forward((int)a.planes, (int)a.H, (int)a.W, a.img.data_ptr<float>(), a.img_stride[0],
                                  a.img_stride[1], a.img_stride[2], a.gt.data_ptr<float>(), a.H * a.W, a.W, 1,
                                  sums.data_ptr<float>(), need_grad && dmaps.numel() ? dmaps.data_ptr<float>() : nullptr,
                                  Scratch::alloc, &scratch, call.stream()),
          call.who);
    return {sums, dmaps};
}

// -> dL/dimg, shaped and laid out like img: scale * (w_ssim * d(sum ssim_map)/dimg + w_abs * sign(img - gt))
// per plane, the weights read on the device (an absent scale is 1)
Tensor image_loss_backward(const Tensor& img, const Tensor& gt, bool hwc, const Tensor& dmaps, const Tensor& w_ssim,
                           const Tensor& w_abs, const std::optional<Tensor>& scale) {
    const LossImages a(img, gt, hwc, "image_loss_backward");
    const Call& call = *a.call;
    auto weight = [&](const Tensor& t, const char* name) {
        auto w = call.on_device(t, name);
        TORCH_CHECK(w.numel() == a.planes, call.who, ": ", name, " float32 [planes] expected");
        return w;
    };
    const auto d = call.on_device(dmaps, "dmaps");
    TORCH_CHECK(d.numel() == 3 * a.gt.numel(), call.who,
                ": dmaps float32 [3,planes,H,W] from image_loss_forward(need_grad=True) expected");
    const auto ws = weight(w_ssim, "w_ssim"), wa = weight(w_abs, "w_abs");
    const auto sc = scale ? weight(*scale, "scale") : Tensor();
    auto out = torch::empty_like(a.img);
    check(r3dg_image_loss_backward((int)a.planes, (int)a.H, (int)a.W, a.img.data_ptr<float>(), a.img_stride[0],
                                   a.img_stride[1], a.img_stride[2], a.gt.data_ptr<float>(), a.H * a.W, a.W, 1,
                                   d.data_ptr<float>(), ws.data_ptr<float>(), wa.data_ptr<float>(),
                                   scale ? sc.data_ptr<float>() : nullptr, out.data_ptr<float>(), call.stream()),
          call.who);
    return out;
}

// ---- image-space regularisers (neilf.py:233-321; csrc/reg_loss.hip) -------------------------------

// The eleven maps in the order of r3dg_reg_loss_inputs: opacity, depth, normal, pseudo_normal, base_color,
// roughness, metallic (rendered: [n,H,W], or the rasterizer's [H,W,n] with hwc), then gt_image, gt_depth,
// image_mask, mvs_normal (always [n,H,W]). None is absent. The checked, contiguous tensors, the struct, and
// the call on the first given map's device (type and shape are reported first, as for the image loss).
constexpr int kRegMaps = 11, kRegRendered = 7;
const int kRegPlanes[kRegMaps] = {1, 1, 3, 3, 3, 1, 1, 3, 1, 1, 3};
const char* const kRegNames[kRegMaps] = {"opacity", "depth", "normal", "pseudo_normal", "base_color", "roughness",
                                         "metallic", "gt_image", "gt_depth", "image_mask", "mvs_normal"};
struct RegInputs {
    std::optional<Call> call;
    std::vector<Tensor> keep;
    r3dg_reg_loss_inputs in{};

    RegInputs(const std::vector<std::optional<Tensor>>& maps, int64_t H, int64_t W, int64_t terms, bool hwc,
              const char* what) {
        TORCH_CHECK((int64_t)maps.size() == kRegMaps, what, ": ", kRegMaps, " maps (or None) expected");
        TORCH_CHECK(H >= 0 && W >= 0 && H * W <= (int64_t)INT32_MAX, what, ": H, W >= 0 and H * W within int32 expected");
        TORCH_CHECK(terms >= 0 && terms < (1 << R3DG_REG_TERMS), what, ": unknown bits in terms");
        keep.resize(kRegMaps);
        in.struct_size = sizeof(r3dg_reg_loss_inputs);
        in.H = (int)H, in.W = (int)W, in.terms = (unsigned)terms;
        r3dg_map* dst[kRegMaps] = {&in.opacity,   &in.depth,    &in.normal,   &in.pseudo_normal, &in.base_color, &in.roughness,
                                   &in.metallic,  &in.gt_image, &in.gt_depth, &in.image_mask,    &in.mvs_normal};
        for (int i = 0; i < kRegMaps; ++i) {
            if (!maps[i]) continue;
            const Tensor& t = *maps[i];
            const int64_t n = kRegPlanes[i];
            TORCH_CHECK(t.scalar_type() == torch::kFloat32, what, ": ", kRegNames[i], ": expected float32");
            const bool pixel_major = hwc && i < kRegRendered;
            if (pixel_major) {
                TORCH_CHECK(t.dim() == 3 && t.size(0) == H && t.size(1) == W && t.size(2) == n, what,
                            ": shape mismatch: ", kRegNames[i], " [H,W,", n, "] expected, got ", t.sizes());
            } else {
                TORCH_CHECK(t.dim() == 3 && t.size(0) == n && t.size(1) == H && t.size(2) == W, what,
                            ": shape mismatch: ", kRegNames[i], " [", n, ",H,W] expected, got ", t.sizes());
            }
            if (!call) call.emplace(what, t, kRegNames[i]);
            keep[i] = call->on_device(t, kRegNames[i]);
            if (t.numel() == 0) continue;
            *dst[i] = pixel_major ? r3dg_map{keep[i].data_ptr<float>(), 1, W * n, n}
                                  : r3dg_map{keep[i].data_ptr<float>(), H * W, W, 1};
        }
        TORCH_CHECK(call.has_value(), what, ": no map given");
    }
};

// -> (values f32 [8]: each enabled term's value under its R3DG_REG_* index, 0 for a disabled one;
//     depth_count int32 [1]: the pixels the depth term selected)
std::tuple<Tensor, Tensor> reg_loss_forward(const std::vector<std::optional<Tensor>>& maps, int64_t H, int64_t W,
                                            int64_t terms, bool hwc) {
    const RegInputs a(maps, H, W, terms, hwc, "reg_loss_forward");
    const Call& call = *a.call;
    // with work to do the finishing kernel writes every slot (0 for a disabled term)
    const bool work = H * W != 0 && terms != 0;
    auto values = work ? torch::empty({R3DG_REG_TERMS}, call.options()) : torch::zeros({R3DG_REG_TERMS}, call.options());
    auto count = work ? torch::empty({1}, call.options(torch::kInt32)) : torch::zeros({1}, call.options(torch::kInt32));
    Scratch scratch(call);
    check(r3dg_reg_loss_forward(&a.in, values.data_ptr<float>(), count.data_ptr<int32_t>(), Scratch::alloc, &scratch,
                                call.stream()),
          call.who);
    return {values, count};
}

// -> the gradients of opacity, depth, normal, base_color, roughness, metallic, each laid out like its map, or
// None where `want` (a bit per map, in this order) is clear or no enabled term reaches the map
std::vector<std::optional<Tensor>> reg_loss_backward(const std::vector<std::optional<Tensor>>& maps, int64_t H,
                                                     int64_t W, int64_t terms, bool hwc, const Tensor& depth_count,
                                                     const Tensor& weights, const std::optional<Tensor>& scale,
                                                     int64_t want) {
    const RegInputs a(maps, H, W, terms, hwc, "reg_loss_backward");
    const Call& call = *a.call;
    const auto cnt = call.on_device(depth_count, "depth_count", torch::kInt32), w = call.on_device(weights, "weights");
    const auto sc = scale ? call.on_device(*scale, "scale") : Tensor();
    TORCH_CHECK(cnt.numel() == 1, call.who, ": depth_count int32 [1] from reg_loss_forward expected");
    TORCH_CHECK(w.numel() == R3DG_REG_TERMS, call.who, ": weights float32 [8] expected");
    TORCH_CHECK(!scale || sc.numel() == 1, call.who, ": scale float32 [1] expected");
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
    std::vector<std::optional<Tensor>> out(6);
    r3dg_reg_loss_grads g{};
    g.struct_size = sizeof(r3dg_reg_loss_grads);
    float** dst[6] = {&g.opacity, &g.depth, &g.normal, &g.base_color, &g.roughness, &g.metallic};
    for (int i = 0; i < 6; ++i) {
        if (!(want >> i & 1) || !reached[i] || !a.keep[src[i]].defined()) continue;
        out[i] = torch::empty_like(a.keep[src[i]]);
        if (out[i]->numel()) *dst[i] = out[i]->data_ptr<float>();
    }
    check(r3dg_reg_loss_backward(&a.in, cnt.data_ptr<int32_t>(), w.data_ptr<float>(),
                                 scale ? sc.data_ptr<float>() : nullptr, &g, call.stream()),
          call.who);
    return out;
}

// ---- the visibility-SH loss and its fit step (relightable3dgaussian_amd/visibility.py) ---------------

// The checked inputs of the visibility-SH loss, on visibility_dc's device; the tensors keep the
// made-contiguous copies alive. `update`: the fit step writes visibility_dc and visibility_rest, so those two
// are taken in place; the rays, the traced values, the normals and the index are only read.
struct VisInputs {
    const Call call;
    Tensor dc, rest, dirs, traced, normals, index;
    r3dg_visibility_sh_inputs in{};

    VisInputs(const Tensor& dc_in, const Tensor& rest_in, const Tensor& rays_d, const Tensor& traced_in,
              const std::optional<Tensor>& normals_in, const std::optional<Tensor>& index_in, const char* who,
              bool update)
        : call(who, dc_in, "visibility_dc") {
        auto sh = [&](const Tensor& t, const char* name) {
            if (!update) return call.on_device(t, name);
            call.in_place(t, name);
            return t;
        };
        dc = sh(dc_in, "visibility_dc");
        rest = sh(rest_in, "visibility_rest");
        const int64_t P = dc.numel();
        TORCH_CHECK(P >= 1 && dc.dim() >= 1 && dc.size(0) == P, who, ": visibility_dc must be [P, 1, 1]");
        TORCH_CHECK(rest.dim() >= 1 && rest.size(0) == P && rest.numel() % P == 0, who,
                    ": visibility_rest must be [P, K - 1, 1] with visibility_dc's P");
        const int64_t K = 1 + rest.numel() / P;
        dirs = call.on_device(rays_d, "rays_d");
        traced = call.on_device(traced_in, "traced");
        TORCH_CHECK(dirs.dim() >= 1 && dirs.size(-1) == 3, who, ": rays_d must be [R, 3]");
        const int64_t R = dirs.numel() / 3;
        TORCH_CHECK(traced.numel() == R, who, ": traced must hold one value per ray (", R, ")");
        if (normals_in.has_value()) {
            normals = call.on_device(*normals_in, "normals");
            TORCH_CHECK(normals.numel() == 3 * P, who, ": normals must be [P, 3]");
        }
        if (index_in.has_value()) {
            index = call.index(*index_in, "index");
            TORCH_CHECK(index.numel() == R, who, ": index must name one Gaussian per ray (", R, ")");
        } else {
            TORCH_CHECK(R == P, who, ": without index, rays_d must hold one ray per Gaussian (P = ", P, ", R = ", R, ")");
        }
        TORCH_CHECK(P <= INT32_MAX && R <= INT32_MAX && K <= INT32_MAX, who, ": sizes must fit an int");
        in.struct_size = sizeof(in);
        in.P = (int)P; in.K = (int)K; in.R = (int)R;
        in.sh_dc = dc.data_ptr<float>();
        in.sh_rest = K > 1 ? rest.data_ptr<float>() : nullptr;
        in.dirs = R ? dirs.data_ptr<float>() : nullptr;
        in.traced = R ? traced.data_ptr<float>() : nullptr;
        in.normals = normals.defined() ? normals.data_ptr<float>() : nullptr;
        in.index = index.defined() && R ? index.data_ptr<int32_t>() : nullptr;
    }
};

// mean over the rays of |traced - clamp(eval_sh(sh[g], d) + 0.5, 0, 1)| -> 0-dim tensor
Tensor visibility_sh_loss_forward(const Tensor& dc, const Tensor& rest, const Tensor& rays_d, const Tensor& traced,
                                  const std::optional<Tensor>& normals, const std::optional<Tensor>& index) {
    const VisInputs v(dc, rest, rays_d, traced, normals, index, "visibility_sh_loss_forward", false);
    auto loss = torch::empty({}, v.dc.options());
    Scratch scratch(v.call);
    check(r3dg_visibility_sh_loss_forward(&v.in, loss.data_ptr<float>(), Scratch::alloc, &scratch, v.call.stream()),
          v.call.who);
    return loss;
}

// -> (grad visibility_dc, grad visibility_rest), dense; upstream is a device scalar (no host read)
std::tuple<Tensor, Tensor> visibility_sh_loss_backward(const Tensor& dc, const Tensor& rest, const Tensor& rays_d,
                                                       const Tensor& traced, const std::optional<Tensor>& normals,
                                                       const std::optional<Tensor>& index, const Tensor& upstream) {
    const VisInputs v(dc, rest, rays_d, traced, normals, index, "visibility_sh_loss_backward", false);
    const auto up = v.call.on_device(upstream, "upstream");
    TORCH_CHECK(up.numel() == 1, v.call.who, ": upstream must be one float32");
    auto gdc = torch::empty_like(v.dc), grest = torch::empty_like(v.rest);
    check(r3dg_visibility_sh_loss_backward(&v.in, up.data_ptr<float>(), gdc.data_ptr<float>(),
                                           v.in.K > 1 ? grest.data_ptr<float>() : nullptr, v.call.stream()),
          v.call.who);
    return {gdc, grest};
}

// one fused fit step (gradient + Adam, in place) over one ray per Gaussian; the mean L1 before the step goes
// to losses[slot]
void visibility_sh_fit_step(Tensor dc, Tensor rest, const Tensor& rays_d, const Tensor& traced,
                            const std::optional<Tensor>& normals, Tensor exp_avg_dc, Tensor exp_avg_rest,
                            Tensor exp_avg_sq_dc, Tensor exp_avg_sq_rest, int64_t step, double lr, double beta1,
                            double beta2, double eps, Tensor losses, int64_t slot) {
    const VisInputs v(dc, rest, rays_d, traced, normals, std::nullopt, "visibility_sh_fit_step", true);
    const Call& call = v.call;
    auto state = [&](const Tensor& t, const Tensor& like, const char* name) {
        float* p = call.in_place(t, name);
        TORCH_CHECK(t.numel() == like.numel(), call.who, ": ", name, " must have its parameter's size");
        return p;
    };
    float* loss = call.in_place(losses, "losses");
    TORCH_CHECK(slot >= 0 && slot < losses.numel(), call.who, ": losses must hold slot ", slot);
    TORCH_CHECK(step >= 1 && step <= INT32_MAX, call.who, ": step must be >= 1");
    r3dg_visibility_fit fit{};
    fit.struct_size = sizeof(fit);
    fit.exp_avg_dc = state(exp_avg_dc, v.dc, "exp_avg_dc");
    fit.exp_avg_sq_dc = state(exp_avg_sq_dc, v.dc, "exp_avg_sq_dc");
    fit.exp_avg_rest = v.in.K > 1 ? state(exp_avg_rest, v.rest, "exp_avg_rest") : nullptr;
    fit.exp_avg_sq_rest = v.in.K > 1 ? state(exp_avg_sq_rest, v.rest, "exp_avg_sq_rest") : nullptr;
    fit.step = (int)step;
    fit.lr = (float)lr;
    fit.beta1 = beta1; fit.beta2 = beta2; fit.eps = eps;
    Scratch scratch(call);
    check(r3dg_visibility_sh_fit_step(&v.in, &fit, loss + slot, Scratch::alloc, &scratch, call.stream()), call.who);
}

}  // namespace

void bind_losses(py::module_& m) {
    // the fused L1 + SSIM image loss (relightable3dgaussian_amd/loss.py)
    m.def("image_loss_forward", &image_loss_forward, py::arg("img"), py::arg("gt"), py::arg("hwc"),
          py::arg("need_grad"));
    m.def("image_loss_backward", &image_loss_backward, py::arg("img"), py::arg("gt"), py::arg("hwc"),
          py::arg("dmaps"), py::arg("w_ssim"), py::arg("w_abs"), py::arg("scale") = py::none());
    m.def("image_loss_window", []() {
        const float* w = r3dg_image_loss_window();
        return std::vector<float>(w, w + 11);
    });
    // the fused depth / mask / normal / base-colour / smoothness terms (relightable3dgaussian_amd/loss.py)
    m.def("reg_loss_forward", &reg_loss_forward, py::arg("maps"), py::arg("H"), py::arg("W"), py::arg("terms"),
          py::arg("hwc"));
    m.def("reg_loss_backward", &reg_loss_backward, py::arg("maps"), py::arg("H"), py::arg("W"), py::arg("terms"),
          py::arg("hwc"), py::arg("depth_count"), py::arg("weights"), py::arg("scale") = py::none(),
          py::arg("want") = 63);
    // the visibility-SH loss and the fused fit step (relightable3dgaussian_amd/visibility.py)
    m.def("visibility_sh_loss_forward", &visibility_sh_loss_forward);
    m.def("visibility_sh_loss_backward", &visibility_sh_loss_backward);
    m.def("visibility_sh_fit_step", &visibility_sh_fit_step);
}
