// module.cpp -- pybind module `_C`: the reference operator surface over the C ABI (include/r3dg_hip.h),
// bound one operator family per source file of this directory; binding.h is what they share.
//
// Mirrors r3dg_rasterization._C (reference r3dg-rasterization/ext.cu:21-35): the same 14
// function names, argument order and return tuples, so gaussian_renderer/neilf.py and
// scene/gaussian_model.py call it unchanged. Documented extensions:
//   (1) None / 0 shader-manager, texture and post-pass handles mean "defaults";
//   (2) every launch goes on the current HIP stream of the device of the call's anchor tensor (means3D,
//       base_color, param, ...), which must be a GPU; the reference's own entry points copy their other
//       tensors there, every other entry point refuses a tensor that lives elsewhere, and all buffers
//       (including the three state buffers) live on that device;
//   (3) extra entry points used by the shipped wrapper and the parity tests
//       (rasterize_gaussians_backward_ex / _chunked / _chunked_packed, render_equation_forward_with_rand,
//       rasterizer_state, feature_groups, create_shader_manager, shader_manager_info), and the operators
//       the reference leaves to torch or to other extensions: the training step, the losses, relighting,
//       the BVH tracer (bvh_tracing._C) and the nearest-neighbour distances (simple_knn._C);
//   (4) the submodule `_C.pbr`: the PBR image head and the light regulariser (pbr.cpp);
//   (5) the submodule `_C.display`: the display and capture head and the environment background (display.cpp).
// Errors from the C ABI surface as RuntimeError with the library's message.
#include <pybind11/pybind11.h>

namespace py = pybind11;

void bind_rasterizer(py::module_& m);       // rasterizer.cpp
void bind_render_equation(py::module_& m);  // render_equation.cpp
void bind_training(py::module_& m);         // training.cpp
void bind_losses(py::module_& m);           // losses.cpp
void bind_bvh(py::module_& m);              // bvh.cpp
void bind_pbr(py::module_& m);              // pbr.cpp (the submodule _C.pbr)
void bind_display(py::module_& m);          // display.cpp (the submodule _C.display)

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "MI355X-native relightable Gaussian-splat rasterizer (drop-in for r3dg_rasterization._C)";
    bind_rasterizer(m);
    bind_render_equation(m);
    bind_training(m);
    bind_losses(m);
    bind_bvh(m);
    bind_pbr(m);
    bind_display(m);
}
