"""Nearest-neighbour distances: drop-in for the reference's `simple_knn` extension
(submodules/simple-knn, `from simple_knn._C import distCUDA2`, scene/gaussian_model.py:13).

`distCUDA2(points)` -- f32 [P, 3] GPU tensor -> f32 [P]: the mean squared distance of every point to
its three nearest other points (csrc/knn.hip; semantics in include/r3dg_hip.h `r3dg_knn_mean_dist2`).
`GaussianModel.create_from_pcd` (gaussian_model.py:548-549) turns it into the initial scales, as does
`trainer.GaussianTrainState.create_from_pcd` here.

`_C` is the package's extension, which carries the reference's `simple_knn._C` name (`distCUDA2`);
`install_simple_knn_alias()` registers this module as `simple_knn` and the extension as `simple_knn._C`.

No CPU path: the extension rejects CPU tensors (the reference's module is CUDA-only too).
"""
from __future__ import annotations

import sys

from . import _C

distCUDA2 = _C.distCUDA2


def install_simple_knn_alias() -> None:
    """Make `from simple_knn._C import distCUDA2` resolve here."""
    sys.modules.setdefault("simple_knn", sys.modules[__name__])
    sys.modules.setdefault("simple_knn._C", _C)


__all__ = ["distCUDA2", "install_simple_knn_alias"]
