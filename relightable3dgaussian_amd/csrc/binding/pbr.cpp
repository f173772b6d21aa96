// pbr.cpp -- the PBR image head (composite over the background, tone step) and the light regulariser
// (csrc/pbr_head.hip; relightable3dgaussian_amd/pbr.py), bound on the submodule `_C.pbr`.
#include "binding.h"

using namespace binding;

namespace {

// pbr [H,W,3] and opacity [H,W,1] (hwc: the rasterizer's blocks as they are) or [3,H,W] and [1,H,W]; bg [3]
// or an image shaped like pbr; gamma [1] with tone gamma. The checked, contiguous tensors on pbr's device
// (type and shape are reported first, wherever the tensors live).
struct HeadInputs {
    std::optional<Call> call;
    Tensor pbr, opacity, bg, gamma;
    int64_t H, W;
    bool bg_image;

    HeadInputs(const Tensor& pbr_in, const Tensor& opacity_in, const Tensor& bg_in,
               const std::optional<Tensor>& gamma_in, int64_t tone, bool hwc, bool backward, const char* what) {
        TORCH_CHECK(pbr_in.scalar_type() == torch::kFloat32 && opacity_in.scalar_type() == torch::kFloat32 &&
                        bg_in.scalar_type() == torch::kFloat32,
                    what, ": expected float32");
        TORCH_CHECK(pbr_in.dim() == 3 && pbr_in.size(hwc ? 2 : 0) == 3, what, ": shape mismatch: pbr ",
                    hwc ? "[H,W,3]" : "[3,H,W]", " expected, got ", pbr_in.sizes());
        H = pbr_in.size(hwc ? 0 : 1);
        W = pbr_in.size(hwc ? 1 : 2);
        TORCH_CHECK(H >= 1 && W >= 1 && H * W <= (int64_t)INT32_MAX, what, ": H, W >= 1 and H * W within int32 expected");
        TORCH_CHECK(opacity_in.dim() == 3 && opacity_in.size(hwc ? 2 : 0) == 1 && opacity_in.numel() == H * W &&
                        opacity_in.size(hwc ? 0 : 1) == H,
                    what, ": shape mismatch: opacity ", hwc ? "[H,W,1]" : "[1,H,W]", " expected, got ",
                    opacity_in.sizes());
        bg_image = bg_in.dim() == 3;
        TORCH_CHECK(bg_image ? bg_in.sizes() == pbr_in.sizes() : (bg_in.dim() == 1 && bg_in.numel() == 3), what,
                    ": shape mismatch: bg [3] or an image shaped like pbr expected, got ", bg_in.sizes());
        TORCH_CHECK(tone >= R3DG_PBR_TONE_NONE && tone <= R3DG_PBR_TONE_CLAMP, what, ": unknown tone ", tone);
        TORCH_CHECK(!backward || tone == R3DG_PBR_TONE_NONE || tone == R3DG_PBR_TONE_GAMMA, what,
                    ": tone aces and clamp are forward only");
        TORCH_CHECK((tone == R3DG_PBR_TONE_GAMMA) == gamma_in.has_value(), what,
                    ": gamma is given with tone gamma and with no other");
        call.emplace(what, pbr_in, "pbr");
        pbr = call->on_device(pbr_in, "pbr");
        opacity = call->on_device(opacity_in, "opacity");
        bg = call->on_device(bg_in, "bg");
        if (gamma_in) {
            gamma = call->on_device(*gamma_in, "gamma");
            TORCH_CHECK(gamma.numel() == 1, what, ": gamma float32 [1] expected");
        }
    }
    const float* gamma_ptr() const { return gamma.defined() ? gamma.data_ptr<float>() : nullptr; }
};

// -> image, shaped and laid out like pbr, a fresh tensor
Tensor head_forward(const Tensor& pbr, const Tensor& opacity, const Tensor& bg, const std::optional<Tensor>& gamma,
                    int64_t tone, bool hwc) {
    const HeadInputs a(pbr, opacity, bg, gamma, tone, hwc, false, "pbr_head_forward");
    const Call& call = *a.call;
    auto image = torch::empty(a.pbr.sizes(), call.options());
    check(r3dg_pbr_head_forward((int)a.H, (int)a.W, hwc ? R3DG_PBR_LAYOUT_HWC : R3DG_PBR_LAYOUT_CHW, (int)tone,
                                a.pbr.data_ptr<float>(), a.opacity.data_ptr<float>(), a.bg.data_ptr<float>(),
                                a.bg_image, a.gamma_ptr(), image.data_ptr<float>(), call.stream()),
          call.who);
    return image;
}

// -> (dL/dpbr like pbr, dL/dopacity like opacity, dL/dgamma [1]), None where `want` (bit 0, 1, 2) is clear
std::tuple<std::optional<Tensor>, std::optional<Tensor>, std::optional<Tensor>> head_backward(
    const Tensor& pbr, const Tensor& opacity, const Tensor& bg, const std::optional<Tensor>& gamma, int64_t tone,
    bool hwc, const Tensor& grad_image, int64_t want) {
    const HeadInputs a(pbr, opacity, bg, gamma, tone, hwc, true, "pbr_head_backward");
    const Call& call = *a.call;
    TORCH_CHECK(want >= 0 && want < 8 && (!(want & 4) || tone == R3DG_PBR_TONE_GAMMA), call.who,
                ": want: bit 0 pbr, 1 opacity, 2 gamma (with tone gamma)");
    TORCH_CHECK(grad_image.sizes() == a.pbr.sizes(), call.who, ": shape mismatch: grad_image shaped like pbr expected");
    const auto g = call.on_device(grad_image, "grad_image");
    std::optional<Tensor> dpbr, dopacity, dgamma;
    if (want & 1) dpbr = torch::empty(a.pbr.sizes(), call.options());
    if (want & 2) dopacity = torch::empty(a.opacity.sizes(), call.options());
    if (want & 4) dgamma = torch::empty({1}, call.options());
    Scratch scratch(call);
    check(r3dg_pbr_head_backward((int)a.H, (int)a.W, hwc ? R3DG_PBR_LAYOUT_HWC : R3DG_PBR_LAYOUT_CHW, (int)tone,
                                 a.pbr.data_ptr<float>(), a.opacity.data_ptr<float>(), a.bg.data_ptr<float>(),
                                 a.bg_image, a.gamma_ptr(), g.data_ptr<float>(),
                                 dpbr ? dpbr->data_ptr<float>() : nullptr,
                                 dopacity ? dopacity->data_ptr<float>() : nullptr,
                                 dgamma ? dgamma->data_ptr<float>() : nullptr, Scratch::alloc, &scratch,
                                 call.stream()),
          call.who);
    return {dpbr, dopacity, dgamma};
}

struct LightInputs {
    std::optional<Call> call;
    Tensor d;
    int64_t P;

    LightInputs(const Tensor& d_in, const char* what) {
        TORCH_CHECK(d_in.scalar_type() == torch::kFloat32, what, ": expected float32");
        TORCH_CHECK(d_in.dim() == 2 && d_in.size(1) == 3 && d_in.size(0) <= (int64_t)INT32_MAX, what,
                    ": shape mismatch: diffuse_light [P,3] expected, got ", d_in.sizes());
        P = d_in.size(0);
        call.emplace(what, d_in, "diffuse_light");
        d = call->on_device(d_in, "diffuse_light");
    }
};

// -> the 0-dim mean of |d_c - mean_c d|; 0 for P = 0 (nothing launched)
Tensor light_loss_forward(const Tensor& diffuse_light) {
    const LightInputs a(diffuse_light, "light_loss_forward");
    const Call& call = *a.call;
    if (a.P == 0) return torch::zeros({}, call.options());
    auto loss = torch::empty({}, call.options());
    Scratch scratch(call);
    check(r3dg_light_loss_forward((int)a.P, a.d.data_ptr<float>(), loss.data_ptr<float>(), Scratch::alloc, &scratch,
                                  call.stream()),
          call.who);
    return loss;
}

// -> dL/ddiffuse_light, contiguous [P,3]; upstream is a device scalar (no host read)
Tensor light_loss_backward(const Tensor& diffuse_light, const Tensor& upstream) {
    const LightInputs a(diffuse_light, "light_loss_backward");
    const Call& call = *a.call;
    const auto up = call.on_device(upstream, "upstream");
    TORCH_CHECK(up.numel() == 1, call.who, ": upstream must be one float32");
    auto grad = torch::empty({a.P, 3}, call.options());
    if (a.P == 0) return grad;
    check(r3dg_light_loss_backward((int)a.P, a.d.data_ptr<float>(), up.data_ptr<float>(), grad.data_ptr<float>(),
                                   call.stream()),
          call.who);
    return grad;
}

}  // namespace

// On a submodule: `_C` itself is the reference's operator surface plus the table tests/test_abi.py holds it to
void bind_pbr(py::module_& m) {
    auto pbr = m.def_submodule("pbr", "the PBR image head and the light regulariser (relightable3dgaussian_amd/pbr.py)");
    pbr.attr("TONES") = py::dict(py::arg("none") = (int)R3DG_PBR_TONE_NONE, py::arg("gamma") = (int)R3DG_PBR_TONE_GAMMA,
                                 py::arg("aces") = (int)R3DG_PBR_TONE_ACES, py::arg("clamp") = (int)R3DG_PBR_TONE_CLAMP);
    pbr.def("head_forward", &head_forward, py::arg("pbr"), py::arg("opacity"), py::arg("bg"), py::arg("gamma"),
            py::arg("tone"), py::arg("hwc"));
    pbr.def("head_backward", &head_backward, py::arg("pbr"), py::arg("opacity"), py::arg("bg"), py::arg("gamma"),
            py::arg("tone"), py::arg("hwc"), py::arg("grad_image"), py::arg("want") = 3);
    pbr.def("light_loss_forward", &light_loss_forward, py::arg("diffuse_light"));
    pbr.def("light_loss_backward", &light_loss_backward, py::arg("diffuse_light"), py::arg("upstream"));
}
