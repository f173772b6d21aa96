// training.cpp -- the training step on the device: optimiser, densification, the parameter activations,
// scene composition and the points capture (include/r3dg_hip.h "training step on the device").
#include "binding.h"

using namespace binding;

namespace {

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

// the flat parameter buffer, which must hold the layout's P * sum(widths) floats
float* param_ptr(const Call& call, const r3dg_param_layout& L, const Tensor& param) {
    float* p = call.in_place(param, "param");
    int64_t total = 0;
    for (int g = 0; g < L.n_groups; ++g) total += (int64_t)L.P * L.width[g];
    TORCH_CHECK(L.P >= 0 && param.numel() >= total, call.who, ": param holds fewer than P * sum(widths) floats");
    return p;
}

// an in-place tensor that may be absent (numel 0)
float* opt_in_place(const Call& call, const Tensor& t, const char* name) {
    return t.numel() ? call.in_place(t, name) : nullptr;
}

void adam_step(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles, Tensor param,
               const Tensor& grad, Tensor exp_avg, Tensor exp_avg_sq, int64_t lo, int64_t hi,
               const std::vector<double>& lrs, double beta1, double beta2, double eps, int64_t step) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    TORCH_CHECK(lrs.size() == widths.size(), "adam_step: one learning rate per group");
    TORCH_CHECK(grad.numel() == hi - lo && exp_avg.numel() == hi - lo && exp_avg_sq.numel() == hi - lo,
                "adam_step: grad / exp_avg / exp_avg_sq must hold the shard's hi - lo floats");
    const Call call("adam_step", param, "param");
    float *p = call.in_place(param, "param"), *m = call.in_place(exp_avg, "exp_avg");
    float* v = call.in_place(exp_avg_sq, "exp_avg_sq");
    const float* g = call.in_place(grad, "grad");
    std::vector<float> lr(lrs.begin(), lrs.end());
    check(r3dg_adam_step(&L, p, g, m, v, lo, hi, lr.data(), beta1, beta2, eps, (int)step, call.stream()), call.who);
}

// adam_step with one step count per group; steps[g] <= 0: group g has no gradient (skipped)
void adam_step_groups(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles, Tensor param,
                      const Tensor& grad, Tensor exp_avg, Tensor exp_avg_sq, int64_t lo, int64_t hi,
                      const std::vector<double>& lrs, double beta1, double beta2, double eps,
                      const std::vector<int64_t>& steps) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    TORCH_CHECK(lrs.size() == widths.size() && steps.size() == widths.size(),
                "adam_step_groups: one learning rate and one step count per group");
    TORCH_CHECK(grad.numel() == hi - lo && exp_avg.numel() == hi - lo && exp_avg_sq.numel() == hi - lo,
                "adam_step_groups: grad / exp_avg / exp_avg_sq must hold the shard's hi - lo floats");
    const Call call("adam_step_groups", param, "param");
    float *p = call.in_place(param, "param"), *m = call.in_place(exp_avg, "exp_avg");
    float* v = call.in_place(exp_avg_sq, "exp_avg_sq");
    const float* g = call.in_place(grad, "grad");
    std::vector<float> lr(lrs.begin(), lrs.end());
    std::vector<int> st(steps.begin(), steps.end());
    check(r3dg_adam_step_groups(&L, p, g, m, v, lo, hi, lr.data(), st.data(), beta1, beta2, eps, call.stream()),
          call.who);
}

void densification_stats(const Tensor& dL_dmeans2D, const Tensor& normal_grad, const Tensor& radii, Tensor xyz_accum,
                         Tensor normal_accum, Tensor denom, Tensor max_radii2D) {
    const int P = (int)radii.size(0);
    TORCH_CHECK(dL_dmeans2D.dim() == 2 && dL_dmeans2D.size(0) == P && dL_dmeans2D.size(1) >= 2,
                "densification_stats: dL_dmeans2D must be [P, >=2]");
    TORCH_CHECK(normal_grad.numel() == 0 || normal_grad.numel() == 3 * (int64_t)P,
                "densification_stats: normal_grad must be [P, 3] or empty");
    const Call call("densification_stats", dL_dmeans2D, "dL_dmeans2D");
    const float *g2d = call.in_place(dL_dmeans2D, "dL_dmeans2D"), *gn = opt_in_place(call, normal_grad, "normal_grad");
    const int* rad = call.in_place<int>(radii, "radii");
    float *xa = call.in_place(xyz_accum, "xyz_accum"), *na = call.in_place(normal_accum, "normal_accum");
    float *dn = call.in_place(denom, "denom"), *mr = call.in_place(max_radii2D, "max_radii2D");
    check(r3dg_densification_stats(P, g2d, (int)dL_dmeans2D.size(1), gn, rad, xa, na, dn, mr, call.stream()), call.who);
}

std::tuple<Tensor, Tensor, Tensor, Tensor, int64_t, std::vector<int64_t>> densify_and_prune(
    int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles, const Tensor& param,
    const Tensor& exp_avg, const Tensor& exp_avg_sq, const Tensor& xyz_accum, const Tensor& normal_accum,
    const Tensor& denom, const Tensor& max_radii2D, double grad_threshold, double grad_normal_threshold,
    double percent_dense, double extent, double min_opacity, double max_screen_size, int64_t N, bool prune_only,
    const Tensor& noise) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    const Call call("densify_and_prune", param, "param");
    r3dg_densify_args d{};
    d.grad_threshold = (float)grad_threshold; d.grad_normal_threshold = (float)grad_normal_threshold;
    d.percent_dense = (float)percent_dense; d.extent = (float)extent; d.min_opacity = (float)min_opacity;
    d.max_screen_size = (float)max_screen_size; d.N = (int)N; d.prune_only = prune_only ? 1 : 0;
    const float *p = call.in_place(param, "param"), *m = call.in_place(exp_avg, "exp_avg");
    const float *v = call.in_place(exp_avg_sq, "exp_avg_sq"), *xa = opt_in_place(call, xyz_accum, "xyz_accum");
    const float *na = opt_in_place(call, normal_accum, "normal_accum"), *dn = opt_in_place(call, denom, "denom");
    const float* mr = opt_in_place(call, max_radii2D, "max_radii2D");
    // a given noise tensor (tests / replicated ranks) replaces the device generator
    Tensor nz = noise.numel() ? call.on_device(noise, "noise") : Tensor();
    auto given_noise = [](void* ctx, size_t n) -> void* {
        auto* t = static_cast<Tensor*>(ctx);
        return (size_t)t->numel() >= n ? t->data_ptr() : nullptr;
    };
    // the new parameter and moment buffers come out of `out`'s blocks and go to the caller
    Scratch out(call);
    float *np = nullptr, *nm = nullptr, *nv = nullptr;
    int* src = nullptr;
    int Pn = 0, counts[4] = {0, 0, 0, 0};
    check(r3dg_densify_and_prune(&L, p, m, v, xa, na, dn, mr, &d, Scratch::alloc, &out,
                                 nz.defined() ? (r3dg_alloc_fn)given_noise : Scratch::randn,
                                 nz.defined() ? (void*)&nz : (void*)&out, &np, &nm, &nv, &src, &Pn, counts,
                                 call.stream()),
          call.who);
    int64_t W = 0;
    for (auto w : widths) W += w;
    const int64_t n = (int64_t)Pn * W;
    auto floats = [&](const void* ptr) { return out.holder(ptr, call.who).narrow(0, 0, 4 * n).view(torch::kFloat32); };
    // the source map gets a block of its own size (the library's block may be larger)
    Tensor source = out.holder(src, call.who).narrow(0, 0, 4 * (int64_t)Pn).view(torch::kInt32).clone();
    return {floats(np), floats(nm), floats(nv), source, (int64_t)Pn,
            std::vector<int64_t>{counts[0], counts[1], counts[2], counts[3]}};
}

void reset_opacity(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles, Tensor param,
                   const Tensor& exp_avg, const Tensor& exp_avg_sq) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    const Call call("reset_opacity", param, "param");
    float *p = call.in_place(param, "param"), *m = opt_in_place(call, exp_avg, "exp_avg");
    float* v = opt_in_place(call, exp_avg_sq, "exp_avg_sq");
    check(r3dg_reset_opacity(&L, p, m, v, call.stream()), call.who);
}

// ---- parameter activations (relightable3dgaussian_amd/activation.py; csrc/activation.hip) ----------

// role_groups: the group index of normal, f_dc, f_rest, base_color, roughness, metallic, incidents_dc,
// incidents_rest, visibility_dc, visibility_rest (-1: absent)
r3dg_activation_io make_activation_io(const Call& call, const r3dg_param_layout* L,
                                      const std::vector<int64_t>& role_groups, const std::optional<Tensor>& campos,
                                      Tensor& campos_keep) {
    TORCH_CHECK(role_groups.size() == 10, call.who, ": role_groups holds 10 group indices");
    r3dg_activation_io io{};
    io.struct_size = sizeof(io);
    io.layout = L;
    io.normal = (int)role_groups[0]; io.f_dc = (int)role_groups[1]; io.f_rest = (int)role_groups[2];
    io.base_color = (int)role_groups[3]; io.roughness = (int)role_groups[4]; io.metallic = (int)role_groups[5];
    io.incidents_dc = (int)role_groups[6]; io.incidents_rest = (int)role_groups[7];
    io.visibility_dc = (int)role_groups[8]; io.visibility_rest = (int)role_groups[9];
    if (campos.has_value()) {
        TORCH_CHECK(campos->numel() == 3, call.who, ": campos must be 3 float32 on param's device");
        campos_keep = call.on_device(*campos, "campos");
        io.campos = campos_keep.data_ptr<float>();
    }
    return io;
}

// -> [scaling, rotation, normal, opacity, shs, base_color, roughness, metallic, incidents, visibility,
//     viewdirs, symm_inv]; None for the PBR outputs of a 7-group layout, viewdirs without campos, symm_inv
//     when not asked for
std::vector<std::optional<Tensor>> activate_forward(int64_t P, const std::vector<int64_t>& widths,
                                                    const std::vector<int64_t>& roles,
                                                    const std::vector<int64_t>& role_groups, const Tensor& param,
                                                    const std::optional<Tensor>& campos, bool inverse_covariance) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    const Call call("activate_forward", param, "param");
    const float* p = param_ptr(call, L, param);
    Tensor cp;
    r3dg_activation_io io = make_activation_io(call, &L, role_groups, campos, cp);
    const auto fopt = param.options();
    const bool pbr = io.base_color >= 0;
    std::vector<std::optional<Tensor>> out(12);
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
    check(r3dg_activate_forward(&io, p, call.stream()), call.who);
    return out;
}

// upstreams: [xyz, scaling, rotation, normal, opacity, shs, base_color, roughness, metallic, incidents,
// visibility, viewdirs], None = zero. An upstream whose dimensions behind the first are dense (a column block
// of a wider row-major array) is passed with its stride(0); any other layout is made contiguous first.
void activate_backward(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles,
                       const std::vector<int64_t>& role_groups, const Tensor& param,
                       const std::optional<Tensor>& campos, const std::vector<std::optional<Tensor>>& upstreams,
                       Tensor grad, bool accumulate) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    const Call call("activate_backward", param, "param");
    const float* p = param_ptr(call, L, param);
    Tensor cp;
    const r3dg_activation_io io = make_activation_io(call, &L, role_groups, campos, cp);
    TORCH_CHECK(upstreams.size() == 12, call.who, ": 12 upstream slots");
    float* out = call.in_place(grad, "grad");
    TORCH_CHECK(grad.numel() >= param.numel(), call.who, ": grad must be a buffer of param's size");
    r3dg_activation_grads g{};
    g.struct_size = sizeof(g);
    r3dg_grad_rows* slots[12] = {&g.xyz, &g.scaling, &g.rotation, &g.normal, &g.opacity, &g.shs, &g.base_color,
                                 &g.roughness, &g.metallic, &g.incidents, &g.visibility, &g.viewdirs};
    const int64_t width[12] = {3, 3, 4, 3, 1, 48, 3, 1, 1, 48, 16, 3};
    std::vector<Tensor> keep;
    for (int i = 0; i < 12; ++i) {
        if (!upstreams[i].has_value()) continue;
        Tensor t = *upstreams[i];
        const std::string name = "upstream " + std::to_string(i);
        TORCH_CHECK(t.dim() >= 1 && t.size(0) == P && t.numel() == P * width[i], call.who, ": ", name,
                    " must be [P, ...] with ", width[i], " floats per row");
        // dense behind the first dimension, rows at least a row apart
        bool dense = t.stride(0) >= width[i];
        int64_t expect = 1;
        for (int64_t d = t.dim() - 1; d >= 1; --d) {
            if (t.size(d) != 1 && t.stride(d) != expect) dense = false;
            expect *= t.size(d);
        }
        call.require(t, name.c_str());
        if (!dense) t = t.contiguous();
        keep.push_back(t);
        if (P > 0) *slots[i] = r3dg_grad_rows{t.data_ptr<float>(), P == 1 ? width[i] : t.stride(0)};
    }
    check(r3dg_activate_backward(&io, p, &g, out, accumulate ? 1 : 0, call.stream()), call.who);
}

// ---- scene composition and the points capture (relightable3dgaussian_amd/compose.py; csrc/compose.hip) ----

// the 19 floats of a transform on param's device (None with flags == 0)
const float* xform_ptr(const Call& call, const std::optional<Tensor>& xform, int64_t flags) {
    if (!xform.has_value()) {
        TORCH_CHECK(flags == 0, call.who, ": transform flags without the 19 floats");
        return nullptr;
    }
    TORCH_CHECK(xform->numel() == 19 || (xform->numel() == 16 && flags == R3DG_XF_TRANSFORM), call.who,
                ": xform must be 19 float32 (16 do for a full transform)");
    return call.in_place(*xform, "xform");
}

void set_transform(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles,
                   int64_t normal_group, Tensor param, const std::optional<Tensor>& xform, int64_t flags) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    const Call call("set_transform", param, "param");
    float* p = param_ptr(call, L, param);
    const float* xf = xform_ptr(call, xform, flags);
    check(r3dg_set_transform(&L, (int)normal_group, p, xf, (int)flags, call.stream()), call.who);
}

// outs: [xyz, scaling, rotation, normal, opacity, base_color, roughness, metallic, shs, incidents, visibility_dc,
// visibility_rest, symm_inv (None: skipped)], the composite's arrays; the object writes rows [row, row + P)
void compose_object(int64_t P, const std::vector<int64_t>& widths, const std::vector<int64_t>& roles,
                    const std::vector<int64_t>& role_groups, const Tensor& param, const std::optional<Tensor>& xform,
                    int64_t flags, const std::vector<std::optional<Tensor>>& outs, int64_t row) {
    const r3dg_param_layout L = make_layout(P, widths, roles);
    const Call call("compose_object", param, "param");
    const float* p = param_ptr(call, L, param);
    Tensor cp;
    const r3dg_activation_io io = make_activation_io(call, &L, role_groups, std::nullopt, cp);
    const float* xf = xform_ptr(call, xform, flags);
    TORCH_CHECK(outs.size() == 13, call.who, ": 13 output slots");
    TORCH_CHECK(row >= 0, call.who, ": negative row offset");
    const int64_t width[13] = {3, 3, 4, 3, 1, 3, 1, 1, 48, 48, 1, 24, 6};
    float* ptr[13];
    for (int i = 0; i < 13; ++i) {
        ptr[i] = nullptr;
        if (!outs[i].has_value()) {
            TORCH_CHECK(i == 12, call.who, ": only symm_inv may be None");
            continue;
        }
        const std::string name = "output " + std::to_string(i);
        ptr[i] = call.in_place(*outs[i], name.c_str());
        TORCH_CHECK(outs[i]->numel() >= (row + P) * width[i], call.who, ": ", name, " holds fewer than row + P rows");
    }
    r3dg_compose_out o{};
    o.struct_size = sizeof(o);
    o.xyz = ptr[0]; o.scaling = ptr[1]; o.rotation = ptr[2]; o.normal = ptr[3]; o.opacity = ptr[4];
    o.base_color = ptr[5]; o.roughness = ptr[6]; o.metallic = ptr[7]; o.shs = ptr[8]; o.incidents = ptr[9];
    o.visibility_dc = ptr[10]; o.visibility_rest = ptr[11]; o.symm_inv = ptr[12];
    check(r3dg_compose_object(&io, p, xf, (int)flags, &o, row, call.stream()), call.who);
}

// bg: 3 floats on the device, or None with the 3 host numbers bg_value (passed to the kernel by value)
// -> (rgb [3,H,W], depth [H,W] or None)
std::tuple<Tensor, std::optional<Tensor>> render_points(const Tensor& xyz, const Tensor& color, const Tensor& world_view,
                                                        const Tensor& intrinsics, int64_t H, int64_t W,
                                                        const std::optional<Tensor>& bg,
                                                        const std::vector<double>& bg_value, bool return_depth) {
    const Call call("render_points", xyz, "xyz");
    auto sized = [&](const Tensor& t, int64_t n, const char* name) {
        TORCH_CHECK(t.numel() == n, call.who, ": ", name, " must hold ", n, " floats");
        return call.on_device(t, name);
    };
    TORCH_CHECK(xyz.dim() == 2 && xyz.size(1) == 3 && color.dim() == 2 && color.size(1) == 3 &&
                    color.size(0) == xyz.size(0),
                call.who, ": xyz and color must be [P, 3]");
    TORCH_CHECK(H > 0 && W > 0 && H * W <= 0x7fffffffLL, call.who, ": bad H or W");
    TORCH_CHECK(xyz.size(0) <= 0x7fffffffLL, call.who, ": more than 2^31 - 1 points (a pixel's key holds a 32-bit index)");
    const auto x = call.on_device(xyz, "xyz"), c = call.on_device(color, "color");
    const auto v = sized(world_view, 16, "world_view_transform"), k = sized(intrinsics, 9, "intrinsics");
    Tensor b;
    float bgv[3] = {0.0f, 0.0f, 0.0f};
    if (bg.has_value()) {
        b = sized(*bg, 3, "bg");
    } else {
        TORCH_CHECK(bg_value.size() == 3, call.who, ": bg_value must hold 3 numbers");
        for (int i = 0; i < 3; ++i) bgv[i] = (float)bg_value[i];
    }
    Tensor rgb = torch::empty({3, H, W}, xyz.options());
    std::optional<Tensor> depth;
    if (return_depth) depth = torch::empty({H, W}, xyz.options());
    const int64_t P = xyz.size(0);
    Scratch scratch(call);
    check(r3dg_render_points((int)P, P ? x.data_ptr<float>() : nullptr, P ? c.data_ptr<float>() : nullptr,
                             v.data_ptr<float>(), k.data_ptr<float>(), (int)H, (int)W,
                             bg.has_value() ? b.data_ptr<float>() : nullptr, bgv, rgb.data_ptr<float>(),
                             depth ? depth->data_ptr<float>() : nullptr, Scratch::alloc, &scratch, call.stream()),
          call.who);
    return {rgb, depth};
}

}  // namespace

void bind_training(py::module_& m) {
    // optimiser and densification (§8f rank 3)
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
}
