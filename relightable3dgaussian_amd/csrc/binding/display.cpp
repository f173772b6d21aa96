// display.cpp -- the display and capture head (csrc/display.hip; relightable3dgaussian_amd/display.py) and the
// environment background (csrc/relight.hip `r3dg_env_background`; relight.py), bound on the submodule `_C.display`.
#include "binding.h"

using namespace binding;

namespace {

// sources[k] float32 [H,W,1|3], with chw[k] [1|3,H,W], int32 [H,W,1] with mode count; opacity [H,W,1]; bg [3] or
// [H,W,3] on the device, or bg_value (3 host numbers, passed by value); -> [K,H,W,3] uint8 or float32, fresh
Tensor frame(const std::vector<Tensor>& sources, const std::vector<int64_t>& modes, const std::vector<int64_t>& tones,
             const std::vector<bool>& chw, const std::optional<Tensor>& opacity, const std::optional<Tensor>& bg,
             const std::vector<double>& bg_value, int64_t encoding) {
    const char* who = "display_frame";
    const size_t K = sources.size();
    TORCH_CHECK(K >= 1 && K <= R3DG_DISPLAY_MAX_SPECS, who, ": 1 to ", R3DG_DISPLAY_MAX_SPECS, " specs expected, got ", K);
    TORCH_CHECK(modes.size() == K && tones.size() == K && chw.size() == K, who,
                ": sources, modes, tones and chw must have one entry per spec");
    TORCH_CHECK(encoding == R3DG_DISPLAY_ENC_F32 || encoding == R3DG_DISPLAY_ENC_U8, who, ": unknown encoding ", encoding);
    TORCH_CHECK(!bg.has_value() || bg_value.empty(), who, ": bg and bg_value exclude each other");
    TORCH_CHECK(bg_value.empty() || bg_value.size() == 3, who, ": bg_value must be 3 numbers");
    int64_t H = 0, W = 0;
    for (size_t k = 0; k < K; ++k) {
        const Tensor& s = sources[k];
        const int c = chw[k] ? 0 : 2;
        TORCH_CHECK(modes[k] >= R3DG_DISPLAY_MODE_PLAIN && modes[k] <= R3DG_DISPLAY_MODE_COUNT, who, ": spec ", k,
                    ": unknown mode ", modes[k]);
        TORCH_CHECK(tones[k] >= R3DG_DISPLAY_TONE_NONE && tones[k] <= R3DG_DISPLAY_TONE_ACES, who, ": spec ", k,
                    ": unknown tone ", tones[k]);
        const bool count = modes[k] == R3DG_DISPLAY_MODE_COUNT;
        TORCH_CHECK(s.scalar_type() == (count ? torch::kInt32 : torch::kFloat32), who, ": spec ", k, ": expected ",
                    count ? "int32 (mode count)" : "float32");
        TORCH_CHECK(s.dim() == 3 && (s.size(c) == 3 || s.size(c) == 1) && (!count || s.size(c) == 1), who, ": spec ", k,
                    ": shape mismatch: ", chw[k] ? "[1|3,H,W]" : "[H,W,1|3]", " expected, got ", s.sizes());
        const int64_t h = s.size(chw[k] ? 1 : 0), w = s.size(chw[k] ? 2 : 1);
        if (k == 0) {
            H = h, W = w;
            TORCH_CHECK(H >= 1 && W >= 1 && H * W <= (int64_t)INT32_MAX, who, ": H, W >= 1 and H * W within int32 expected");
        }
        TORCH_CHECK(h == H && w == W, who, ": spec ", k, ": shape mismatch: every source must be ", H, " x ", W, ", got ",
                    s.sizes());
    }
    if (opacity)
        TORCH_CHECK(opacity->scalar_type() == torch::kFloat32 && opacity->dim() == 3 && opacity->size(0) == H &&
                        opacity->size(1) == W && opacity->size(2) == 1,
                    who, ": shape mismatch: opacity float32 [H,W,1] expected, got ", opacity->sizes());
    bool bg_image = false;
    if (bg) {
        bg_image = bg->dim() == 3;
        TORCH_CHECK(bg->scalar_type() == torch::kFloat32 &&
                        (bg_image ? (bg->size(0) == H && bg->size(1) == W && bg->size(2) == 3)
                                  : (bg->dim() == 1 && bg->numel() == 3)),
                    who, ": shape mismatch: bg float32 [3] or [H,W,3] expected, got ", bg->sizes());
    }
    const Call call(who, sources[0], "source");
    std::vector<Tensor> keep(K);
    r3dg_display_spec specs[R3DG_DISPLAY_MAX_SPECS];
    for (size_t k = 0; k < K; ++k) {
        const bool count = modes[k] == R3DG_DISPLAY_MODE_COUNT;
        keep[k] = call.on_device(sources[k], "source", count ? torch::kInt32 : torch::kFloat32);
        specs[k] = r3dg_display_spec{keep[k].data_ptr(), (int)sources[k].size(chw[k] ? 0 : 2),
                                     chw[k] ? R3DG_PBR_LAYOUT_CHW : R3DG_PBR_LAYOUT_HWC, (int)modes[k], (int)tones[k]};
    }
    Tensor o, b;
    if (opacity) o = call.on_device(*opacity, "opacity");
    if (bg) b = call.on_device(*bg, "bg");
    const float host_bg[3] = {bg_value.empty() ? 0.f : (float)bg_value[0], bg_value.empty() ? 0.f : (float)bg_value[1],
                              bg_value.empty() ? 0.f : (float)bg_value[2]};
    const int bg_kind = bg ? (bg_image ? R3DG_DISPLAY_BG_IMAGE : R3DG_DISPLAY_BG_VECTOR)
                           : (bg_value.empty() ? R3DG_DISPLAY_BG_NONE : R3DG_DISPLAY_BG_HOST);
    const float* bg_ptr = bg ? b.data_ptr<float>() : (bg_value.empty() ? nullptr : host_bg);
    const bool u8 = encoding == R3DG_DISPLAY_ENC_U8;
    auto out = torch::empty({(int64_t)K, H, W, 3}, call.options(u8 ? torch::kUInt8 : torch::kFloat32));
    Scratch scratch(call);
    check(r3dg_display_frame((int)H, (int)W, (int)K, specs, opacity ? o.data_ptr<float>() : nullptr, bg_ptr, bg_kind,
                             (int)encoding, out.data_ptr(), Scratch::alloc, &scratch, call.stream()),
          call.who);
    return out;
}

// -> the environment behind the object [H,W,3]: the map lookup with envmap [He,We,3] (and its optional
// [3,3] transform), else max(eval_sh + 0.5, 0) of shs [1,M,3] or [M,3]
Tensor env_background(const Tensor& intrinsics, const Tensor& c2w, int64_t H, int64_t W,
                      const std::optional<Tensor>& envmap, const std::optional<Tensor>& env_transform,
                      const std::optional<Tensor>& shs) {
    const char* who = "env_background";
    TORCH_CHECK(H >= 1 && W >= 1 && H * W <= (int64_t)INT32_MAX, who, ": H, W >= 1 and H * W within int32 expected");
    TORCH_CHECK(intrinsics.dim() == 2 && intrinsics.size(0) == 3 && intrinsics.size(1) == 3, who,
                ": shape mismatch: intrinsics [3,3] expected, got ", intrinsics.sizes());
    TORCH_CHECK(c2w.dim() == 2 && c2w.size(0) == c2w.size(1) && (c2w.size(0) == 3 || c2w.size(0) == 4), who,
                ": shape mismatch: c2w [4,4] or [3,3] expected, got ", c2w.sizes());
    TORCH_CHECK(envmap.has_value() != shs.has_value(), who, ": one of envmap and shs expected");
    if (envmap) {
        TORCH_CHECK(envmap->dim() == 3 && envmap->size(2) == 3 && envmap->size(0) >= 1 && envmap->size(1) >= 1 &&
                        envmap->size(0) <= INT32_MAX && envmap->size(1) <= INT32_MAX,
                    who, ": shape mismatch: envmap [He,We,3] expected, got ", envmap->sizes());
        TORCH_CHECK(!env_transform || (env_transform->dim() == 2 && env_transform->size(0) == 3 && env_transform->size(1) == 3),
                    who, ": shape mismatch: env_transform [3,3] expected, got ", env_transform->sizes());
    } else {
        TORCH_CHECK((shs->dim() == 3 ? shs->size(0) == 1 : shs->dim() == 2) && shs->size(-1) == 3 && shs->size(-2) >= 1 &&
                        shs->size(-2) <= 25,
                    who, ": shape mismatch: shs [1,M,3] with M <= 25 (degree 4) expected, got ", shs->sizes());
    }
    const Call call(who, intrinsics, "intrinsics");
    const auto Kt = call.on_device(intrinsics, "intrinsics"), R = call.on_device(c2w, "c2w");
    Tensor map, xf, sh;
    int64_t S = 0;
    if (envmap) {
        map = call.on_device(*envmap, "envmap");
        if (env_transform) xf = call.on_device(*env_transform, "env_transform");
    } else {
        sh = call.on_device(*shs, "shs");
        S = shs->size(-2);
    }
    auto out = torch::empty({H, W, 3}, call.options());
    check(r3dg_env_background((int)H, (int)W, Kt.data_ptr<float>(), R.data_ptr<float>(), (int)c2w.size(0),
                              envmap ? R3DG_LIGHT_MAP : R3DG_LIGHT_SH, envmap ? map.data_ptr<float>() : nullptr,
                              envmap ? (int)map.size(0) : 0, envmap ? (int)map.size(1) : 0,
                              xf.defined() ? xf.data_ptr<float>() : nullptr, envmap ? nullptr : sh.data_ptr<float>(),
                              (int)S, out.data_ptr<float>(), call.stream()),
          call.who);
    return out;
}

}  // namespace

// On a submodule: `_C` itself is the reference's operator surface plus the table tests/test_abi.py holds it to
void bind_display(py::module_& m) {
    auto d = m.def_submodule("display", "the display and capture head and the environment background "
                                        "(relightable3dgaussian_amd/display.py, relight.py)");
    d.attr("MODES") = py::dict(py::arg("plain") = (int)R3DG_DISPLAY_MODE_PLAIN, py::arg("over") = (int)R3DG_DISPLAY_MODE_OVER,
                               py::arg("normal_over") = (int)R3DG_DISPLAY_MODE_NORMAL_OVER,
                               py::arg("normal_mask") = (int)R3DG_DISPLAY_MODE_NORMAL_MASK,
                               py::arg("range") = (int)R3DG_DISPLAY_MODE_RANGE, py::arg("count") = (int)R3DG_DISPLAY_MODE_COUNT);
    d.attr("TONES") = py::dict(py::arg("none") = (int)R3DG_DISPLAY_TONE_NONE, py::arg("clamp") = (int)R3DG_DISPLAY_TONE_CLAMP,
                               py::arg("aces") = (int)R3DG_DISPLAY_TONE_ACES);
    d.attr("ENCODINGS") = py::dict(py::arg("f32") = (int)R3DG_DISPLAY_ENC_F32, py::arg("u8") = (int)R3DG_DISPLAY_ENC_U8);
    d.attr("MAX_SPECS") = (int)R3DG_DISPLAY_MAX_SPECS;
    d.def("frame", &frame, py::arg("sources"), py::arg("modes"), py::arg("tones"), py::arg("chw"), py::arg("opacity"),
          py::arg("bg"), py::arg("bg_value"), py::arg("encoding"));
    d.def("env_background", &env_background, py::arg("intrinsics"), py::arg("c2w"), py::arg("H"), py::arg("W"),
          py::arg("envmap"), py::arg("env_transform"), py::arg("shs"));
}
