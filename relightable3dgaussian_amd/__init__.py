"""MI355X-native relightable Gaussian-splat rasterizer (drop-in for r3dg_rasterization._C).

`relightable3dgaussian_amd._C` is the pybind module built from csrc/binding/ on top of
lib/libr3dg_hip.so (HIP kernels for gfx950 + the C ABI in include/r3dg_hip.h). There is no
CPU fallback: importing `_C` raises if the extension has not been built, and every operator
requires GPU tensors.

`install_alias()` registers this package as `r3dg_rasterization` so the reference's
`from r3dg_rasterization import _C` (gaussian_renderer/r3dg_rasterization.py:7-8,
scene/gaussian_model.py:18) resolves here, and `relightable3dgaussian_amd.bvh` as the reference's
`bvh` package (`from bvh import RayTracer`, scene/gaussian_model.py:16) and
`relightable3dgaussian_amd.simple_knn` as its `simple_knn` extension (`from simple_knn._C import
distCUDA2`, scene/gaussian_model.py:13).

`relightable3dgaussian_amd.loss` is the training image loss (`ssim` of utils/loss_utils.py and the
fused L1 + SSIM term of calculate_loss).

`relightable3dgaussian_amd.relight` is the relighting script's render equation and environment-map
light (gaussian_renderer/neilf_composite.py, scene/envmap.py).

`relightable3dgaussian_amd.visibility` is visibility baking: the traced per-sample visibility that
render equation reads (relighting.py `update_visibility`), the visibility-SH training term
(neilf.py `lambda_visibility`) and `finetune_visibility` (scene/gaussian_model.py).

`relightable3dgaussian_amd.activation` is the parameter activations of a training iteration
(`GaussianTrainState.activate`): the getters of scene/gaussian_model.py and neilf.py's view
directions from the flat parameter buffer, and their backward into the flat gradient buffer.

`relightable3dgaussian_amd.compose` is the relighting script's scene composition (`set_transform`,
`compose_scene`, `load_scene`: relighting.py `scene_composition`), and `relight.render_points` its
`points` capture.

`relightable3dgaussian_amd.pbr` is the PBR image head (`pbr_image`: the composite over the background and
the tone step between the rasterizer and the image loss, neilf.py:169-175) and the `lambda_light` term
(`light_loss`, neilf.py:278-283).

`relightable3dgaussian_amd.display` is the display and capture head (`frame_buffers`: from the rasterizer's
buffers to the 8-bit or float32 images a GUI frame, a relighting frame's captures or the evaluation report
shows, in one launch), and `relight.env_background` the environment behind the object as an image.
"""
from __future__ import annotations

import importlib.machinery
import importlib.util
import os
import sys

import torch  # noqa: F401  (loads libtorch / the HIP runtime before our libraries)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.environ.get("R3DG_LIB_DIR") or os.path.join(_PKG, "lib")  # override: experiment builds
HIP_LIB = os.path.join(LIB_DIR, "libr3dg_hip.so")
EXT_LIB = os.path.join(LIB_DIR, "_C.so")


def _load_ext():
    if not os.path.exists(EXT_LIB) or not os.path.exists(HIP_LIB):
        raise ImportError(
            "relightable3dgaussian_amd: native extension not built (expected %s and %s); run "
            "`python relightable3dgaussian_amd/build.py` or __graft_entry__.build()" % (HIP_LIB, EXT_LIB))
    loader = importlib.machinery.ExtensionFileLoader("relightable3dgaussian_amd._C", EXT_LIB)
    spec = importlib.util.spec_from_file_location("relightable3dgaussian_amd._C", EXT_LIB, loader=loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    sys.modules["relightable3dgaussian_amd._C"] = mod
    return mod


_C = _load_ext()


def install_alias() -> None:
    """Make `import r3dg_rasterization` / `from r3dg_rasterization import _C` resolve here."""
    from . import r3dg_rasterization as wrapper

    sys.modules.setdefault("r3dg_rasterization", wrapper)
    sys.modules.setdefault("r3dg_rasterization._C", _C)
    # the reference's BVH tracer package (bvh/__init__.py) and its extension bvh_tracing._C
    from .bvh import install_bvh_alias

    install_bvh_alias()
    # the reference's nearest-neighbour extension simple_knn._C (scene/gaussian_model.py:13)
    from .simple_knn import install_simple_knn_alias

    install_simple_knn_alias()


__all__ = ["_C", "install_alias", "HIP_LIB", "EXT_LIB"]
