// render_equation.cpp -- the render equation: the reference's three forwards and its backward, the
// relighting script's variant, and the environment-map light.
#include "binding.h"

using namespace binding;

namespace {

// What every reference render_equation_* entry starts with: the call on base_color's device, the eight
// BRDF tensors moved there (base_color, roughness, metallic, normals, viewdirs, incidents_shs,
// direct_shs, visibility_shs, in this order) and the struct the C ABI reads them through.
struct Brdf {
    const Call call;
    std::vector<Tensor> t;
    r3dg_brdf_inputs in{};

    Brdf(const char* who, std::initializer_list<Tensor> src, int64_t sample_num) : call(who, *src.begin(), "base_color") {
        static const char* const names[8] = {"base_color", "roughness",     "metallic",   "normals",
                                             "viewdirs",   "incidents_shs", "direct_shs", "visibility_shs"};
        for (const auto& s : src) t.push_back(call.moved(s, names[t.size()]));
        in.P = (int)t[0].size(0);
        in.S_incident = (int)t[5].size(1);
        in.S_direct = (int)t[6].size(1);
        in.S_visibility = (int)t[7].size(1);
        in.sample_num = (int)sample_num;
        in.base_color = opt_ptr(t[0]); in.roughness = opt_ptr(t[1]); in.metallic = opt_ptr(t[2]);
        in.normals = opt_ptr(t[3]); in.viewdirs = opt_ptr(t[4]); in.incidents_shs = opt_ptr(t[5]);
        in.direct_shs = opt_ptr(t[6]); in.visibility_shs = opt_ptr(t[7]);
    }
};

std::tuple<Tensor, Tensor, Tensor> render_equation_forward_impl(const Brdf& b, bool is_training, const Tensor* rand_in) {
    const int64_t P = b.in.P, Ns = b.in.sample_num;
    const auto fopt = b.call.options();
    Tensor pbr = torch::empty({P, 3}, fopt), dirs = torch::empty({P, Ns, 3}, fopt), diffuse = torch::empty({P, 3}, fopt);
    // the reference always draws the per-(Gaussian, sample) rotation (render_equation.cu:708)
    Tensor rnd = rand_in ? b.call.moved(*rand_in, "rand_float") : torch::rand({P, Ns, 1}, fopt);
    check(r3dg_render_equation_forward(&b.in, is_training, opt_ptr(rnd), pbr.data_ptr<float>(), dirs.data_ptr<float>(),
                                       diffuse.data_ptr<float>(), b.call.stream()),
          "render_equation_forward");
    return {pbr, dirs, diffuse};
}

// RenderEquationForwardCUDA (render_equation.cu:688-726)
std::tuple<Tensor, Tensor, Tensor> render_equation_forward(const Tensor& base_color, const Tensor& roughness,
                                                           const Tensor& metallic, const Tensor& normals,
                                                           const Tensor& viewdirs, const Tensor& incidents_shs,
                                                           const Tensor& direct_shs, const Tensor& visibility_shs,
                                                           int64_t sample_num, bool is_training, bool debug) {
    (void)debug;
    const Brdf b("render_equation_forward",
                 {base_color, roughness, metallic, normals, viewdirs, incidents_shs, direct_shs, visibility_shs}, sample_num);
    return render_equation_forward_impl(b, is_training, nullptr);
}

// test entry: explicit rotation randoms [P, sample_num(, 1)]
std::tuple<Tensor, Tensor, Tensor> render_equation_forward_with_rand(
    const Tensor& base_color, const Tensor& roughness, const Tensor& metallic, const Tensor& normals,
    const Tensor& viewdirs, const Tensor& incidents_shs, const Tensor& direct_shs, const Tensor& visibility_shs,
    int64_t sample_num, bool is_training, const Tensor& rand_float) {
    const Brdf b("render_equation_forward_with_rand",
                 {base_color, roughness, metallic, normals, viewdirs, incidents_shs, direct_shs, visibility_shs}, sample_num);
    return render_equation_forward_impl(b, is_training, &rand_float);
}

// RenderEquationForwardCUDA_complex (render_equation.cu:220-274)
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>
render_equation_forward_complex(const Tensor& base_color, const Tensor& roughness, const Tensor& metallic,
                                const Tensor& normals, const Tensor& viewdirs, const Tensor& incidents_shs,
                                const Tensor& direct_shs, const Tensor& visibility_shs, int64_t sample_num) {
    const Brdf b("render_equation_forward_complex",
                 {base_color, roughness, metallic, normals, viewdirs, incidents_shs, direct_shs, visibility_shs}, sample_num);
    const int64_t P = b.in.P, Ns = sample_num;
    const auto fopt = b.call.options();
    Tensor pbr = torch::empty({P, 3}, fopt), dirs = torch::empty({P, Ns, 3}, fopt);
    Tensor lights = torch::empty({P, Ns, 3}, fopt), local = torch::empty({P, Ns, 3}, fopt);
    Tensor global = torch::empty({P, Ns, 3}, fopt), vis = torch::empty({P, Ns, 1}, fopt);
    Tensor diffuse = torch::empty({P, 3}, fopt), local_diffuse = torch::empty({P, 3}, fopt);
    Tensor accum = torch::empty({P, 1}, fopt), rgb_d = torch::empty({P, 3}, fopt);
    Tensor rgb_s = torch::empty({P, 3}, fopt);
    r3dg_brdf_complex_outputs o{pbr.data_ptr<float>(),     dirs.data_ptr<float>(),  lights.data_ptr<float>(),
                                local.data_ptr<float>(),   global.data_ptr<float>(), vis.data_ptr<float>(),
                                diffuse.data_ptr<float>(), local_diffuse.data_ptr<float>(),
                                accum.data_ptr<float>(),   rgb_d.data_ptr<float>(), rgb_s.data_ptr<float>()};
    check(r3dg_render_equation_forward_complex(&b.in, &o, b.call.stream()), b.call.who);
    return {pbr, dirs, lights, local, global, vis, diffuse, local_diffuse, accum, rgb_d, rgb_s};
}

// RenderEquationBackwardCUDA (render_equation.cu:494-547)
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> render_equation_backward(
    const Tensor& base_color, const Tensor& roughness, const Tensor& metallic, const Tensor& normals,
    const Tensor& viewdirs, const Tensor& incidents_shs, const Tensor& direct_shs, const Tensor& visibility_shs,
    int64_t sample_num, const Tensor& incident_dirs, const Tensor& dL_dpbr, const Tensor& dL_ddiffuse_light, bool debug) {
    (void)debug;
    const Brdf b("render_equation_backward",
                 {base_color, roughness, metallic, normals, viewdirs, incidents_shs, direct_shs, visibility_shs}, sample_num);
    const auto dirs = b.call.moved(incident_dirs, "incident_dirs"), g_pbr = b.call.moved(dL_dpbr, "dL_dpbr");
    const auto g_diffuse = b.call.moved(dL_ddiffuse_light, "dL_ddiffuse_light");
    const r3dg_brdf_inputs& in = b.in;
    const int P = in.P;
    const auto fopt = b.call.options();
    Tensor d_base = torch::empty({P, 3}, fopt), d_rough = torch::empty({P, 1}, fopt);
    Tensor d_metal = torch::empty({P, 1}, fopt), d_n = torch::empty({P, 3}, fopt);
    Tensor d_v = torch::empty({P, 3}, fopt), d_inc = torch::empty({P, in.S_incident, 3}, fopt);
    Tensor d_dir = torch::empty({1, in.S_direct, 3}, fopt), d_vis = torch::empty({P, in.S_visibility, 1}, fopt);
    r3dg_brdf_grads o{d_base.data_ptr<float>(), d_rough.data_ptr<float>(), d_metal.data_ptr<float>(),
                      d_n.data_ptr<float>(),    d_v.data_ptr<float>(),     d_inc.data_ptr<float>(),
                      d_dir.data_ptr<float>(),  d_vis.data_ptr<float>()};
    Scratch scratch(b.call);
    check(r3dg_render_equation_backward(&in, opt_ptr(dirs), opt_ptr(g_pbr), opt_ptr(g_diffuse), Scratch::alloc, &scratch,
                                        &o, b.call.stream()),
          b.call.who);
    return {d_base, d_rough, d_metal, d_n, d_v, d_inc, d_dir, d_vis};
}

// r3dg_render_equation_relight: rendering_equation_python of the relighting script
// (neilf_composite.py:241-334) and the feature concatenation (:129-133) -> features [P, 21].
// light_mode 0 none / 1 SH (direct_shs [1, S, 3]) / 2 map (envmap [He, We, 3], env_transform [3, 3] or
// None); traced_visibility [P, Ns] or [P, Ns, 1], or None for the baked visibility_shs [P, S, 1].
// Nothing is moved between devices here: every tensor must be on base_color's.
Tensor render_equation_relight(const Tensor& base_color, const Tensor& roughness, const Tensor& metallic,
                               const Tensor& normals, const Tensor& viewdirs, const Tensor& incidents_shs,
                               const std::optional<Tensor>& direct_shs, const std::optional<Tensor>& visibility_shs,
                               int64_t sample_num, int64_t light_mode, const std::optional<Tensor>& envmap,
                               const std::optional<Tensor>& env_transform,
                               const std::optional<Tensor>& traced_visibility) {
    const Call call("render_equation_relight", base_color, "base_color");
    TORCH_CHECK(base_color.dim() == 2 && base_color.size(1) == 3, "relight: base_color must be [P, 3]");
    const int64_t P = base_color.size(0);
    TORCH_CHECK(P <= INT32_MAX && sample_num <= INT32_MAX, "relight: P and sample_num must fit an int");
    auto per_gaussian = [&](const Tensor& t, const char* name, int64_t w) {
        TORCH_CHECK(t.numel() == P * w && t.dim() >= 1 && t.size(0) == P, "relight: ", name, " must be [P, ", w, "]");
        return call.on_device(t, name);
    };
    auto sh_rows = [&](const Tensor& t, const char* name, int64_t rows, int64_t ch) {
        TORCH_CHECK(t.dim() == 3 && t.size(0) == rows && t.size(2) == ch, "relight: ", name, " must be [", rows,
                    ", S, ", ch, "]");
        return call.on_device(t, name);
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
    Tensor env, vis, map, xf, traced;  // keep the contiguous copies alive over the launch
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
        map = call.on_device(*envmap, "envmap");
        in.envmap = map.data_ptr<float>();
        in.env_h = (int)map.size(0);
        in.env_w = (int)map.size(1);
        if (env_transform.has_value()) {
            TORCH_CHECK(env_transform->dim() == 2 && env_transform->size(0) == 3 && env_transform->size(1) == 3,
                        "relight: env_transform must be [3, 3]");
            xf = call.on_device(*env_transform, "env_transform");
            in.env_transform = xf.data_ptr<float>();
        }
    }
    if (traced_visibility.has_value()) {
        const auto& tv = *traced_visibility;
        TORCH_CHECK((tv.dim() == 2 || (tv.dim() == 3 && tv.size(2) == 1)) && tv.size(0) == P && tv.size(1) == sample_num,
                    "relight: traced_visibility must be [P, sample_num] or [P, sample_num, 1]");
        traced = call.on_device(tv, "traced_visibility");
        // P = 0: an empty tensor's pointer may be null, which would read as "baked"
        in.traced_visibility = P > 0 ? traced.data_ptr<float>() : nullptr;
    } else {
        TORCH_CHECK(visibility_shs.has_value(), "relight: needs visibility_shs or traced_visibility");
        vis = sh_rows(*visibility_shs, "visibility_shs", P, 1);
        in.brdf.S_visibility = (int)vis.size(1);
        in.brdf.visibility_shs = vis.data_ptr<float>();
    }
    Tensor features = torch::empty({P, 21}, base.options());
    check(r3dg_render_equation_relight(&in, features.data_ptr<float>(), call.stream()), call.who);
    return features;
}

// r3dg_envmap_direct_light: EnvLight.direct_light (scene/envmap.py:31-48), dirs [..., 3] -> [..., 3]
Tensor envmap_direct_light(const Tensor& dirs, const Tensor& envmap, const std::optional<Tensor>& env_transform) {
    const Call call("envmap_direct_light", dirs, "dirs");
    TORCH_CHECK(dirs.dim() >= 1 && dirs.size(-1) == 3, "envmap_direct_light: dirs must be [..., 3]");
    TORCH_CHECK(envmap.dim() == 3 && envmap.size(2) == 3 && envmap.size(0) >= 1 && envmap.size(1) >= 1 &&
                    envmap.size(0) <= INT32_MAX && envmap.size(1) <= INT32_MAX,
                "envmap_direct_light: envmap must be [He, We, 3]");
    auto d = call.on_device(dirs, "dirs"), map = call.on_device(envmap, "envmap");
    const int64_t n = d.numel() / 3;
    TORCH_CHECK(n <= INT32_MAX, "envmap_direct_light: too many directions");
    Tensor xf;
    const float* xp = nullptr;
    if (env_transform.has_value()) {
        TORCH_CHECK(env_transform->dim() == 2 && env_transform->size(0) == 3 && env_transform->size(1) == 3,
                    "envmap_direct_light: env_transform must be [3, 3]");
        xf = call.on_device(*env_transform, "env_transform");
        xp = xf.data_ptr<float>();
    }
    Tensor light = torch::empty_like(d);
    check(r3dg_envmap_direct_light((int)n, n ? d.data_ptr<float>() : nullptr, map.data_ptr<float>(), (int)map.size(0),
                                   (int)map.size(1), xp, n ? light.data_ptr<float>() : nullptr, call.stream()),
          call.who);
    return light;
}

}  // namespace

void bind_render_equation(py::module_& m) {
    // the reference surface (ext.cu:21-35)
    m.def("render_equation_forward", &render_equation_forward);
    m.def("render_equation_forward_complex", &render_equation_forward_complex);
    m.def("render_equation_backward", &render_equation_backward);
    // extension: the forward with given randoms
    m.def("render_equation_forward_with_rand", &render_equation_forward_with_rand);
    // the relighting script's render equation and environment light (neilf_composite.py, envmap.py)
    m.def("render_equation_relight", &render_equation_relight);
    m.def("envmap_direct_light", &envmap_direct_light);
}
