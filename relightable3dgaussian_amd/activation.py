"""Parameter activations of a training iteration: from `GaussianTrainState`'s flat parameter buffer to every
per-Gaussian input of the rasterizer, the render equation and the tracer, and from their upstream gradients
straight into the flat gradient buffer (csrc/activation.hip; semantics in include/r3dg_hip.h).

  activate(st, campos=None, inverse_covariance=False, accumulate=False) -> dict
      (`GaussianTrainState.activate` is this function.) What the reference's getters compute per iteration
      (scene/gaussian_model.py:23-44, 331-413; gaussian_renderer/neilf.py:102), in two launches:
        xyz        the xyz block of st.param itself (same data_ptr as st.view("xyz"), no copy)
        scaling    exp                              rotation   F.normalize
        normal     F.normalize(eps=1e-3)            opacity    sigmoid
        shs        cat(f_dc, f_rest) [P,16,3]
        base_color, roughness, metallic (sigmoid), incidents [P,16,3], visibility [P,16,1]   14-group states
        viewdirs   F.normalize(campos - xyz)                                              campos given
        symm_inv   get_inverse_covariance() [P,6], not differentiable                  inverse_covariance=True
      The outputs carry autograd history. `loss.backward()` runs two launches that write the gradient of
      EVERY group into st.grad: all of grad[0 : st.total()) is overwritten (zeros for a group no output of
      which reached the loss), so `st.step(zero_grad=False)` is correct afterwards and nothing has to be
      copied into `st.grad_view(name)`. accumulate=True adds to st.grad instead (several views per step).
      If no output reaches the loss, no backward runs and st.grad stays as it was.

The differentiable input of the autograd node is a zero-size anchor leaf kept on the state, not st.param:
st.param stays a plain buffer that `st.step()` and densification write in place. The backward recomputes the
activations from st.param, so the parameters must not change between `activate` and the `backward()` that
belongs to it (the result is unspecified if they do; a densification in between is such a change). Under
`torch.no_grad()` only the forward runs.

No CPU path and no torch fallback: the extension rejects CPU tensors.
"""
from __future__ import annotations

import torch

from . import _C

# the order of `_C.activate_forward`'s result and of `_C.activate_backward`'s upstream slots
FORWARD_SLOTS = ("scaling", "rotation", "normal", "opacity", "shs", "base_color", "roughness", "metallic",
                 "incidents", "visibility", "viewdirs", "symm_inv")
UPSTREAM_SLOTS = ("xyz", "scaling", "rotation", "normal", "opacity", "shs", "base_color", "roughness", "metallic",
                  "incidents", "visibility", "viewdirs")
# the roles that the param layout does not name itself, in `role_groups` order
ROLE_NAMES = ("normal", "f_dc", "f_rest", "base_color", "roughness", "metallic", "incidents_dc", "incidents_rest",
              "visibility_dc", "visibility_rest")


def role_groups(st) -> list:
    names = [n for n, _ in st.groups]
    return [names.index(n) if n in names else -1 for n in ROLE_NAMES]


def _output_names(st, campos, inverse_covariance) -> list:
    pbr = any(g == "base_color" for g, _ in st.groups)
    skip = set() if pbr else {"base_color", "roughness", "metallic", "incidents", "visibility"}
    if campos is None:
        skip.add("viewdirs")
    if not inverse_covariance:
        skip.add("symm_inv")
    return ["xyz"] + [n for n in FORWARD_SLOTS if n not in skip]


class _Activate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, st, campos, inverse_covariance, accumulate):
        # the buffers of this forward: a densification later replaces the state's, not these
        ctx.layout = (st.P, st.widths(), st.roles(), role_groups(st))
        ctx.param, ctx.grad, ctx.campos, ctx.accumulate = st.param, st.grad, campos, bool(accumulate)
        ctx.names = _output_names(st, campos, inverse_covariance)
        ctx.set_materialize_grads(False)
        outs = dict(zip(FORWARD_SLOTS, _C.activate_forward(*ctx.layout, st.param, campos, bool(inverse_covariance))))
        outs["xyz"] = st.view("xyz")
        if inverse_covariance:
            ctx.mark_non_differentiable(outs["symm_inv"])
        return tuple(outs[n] for n in ctx.names)

    @staticmethod
    def backward(ctx, *grads):
        given = dict(zip(ctx.names, grads))
        _C.activate_backward(*ctx.layout, ctx.param, ctx.campos, [given.get(n) for n in UPSTREAM_SLOTS], ctx.grad,
                             ctx.accumulate)
        return None, None, None, None, None


def activate(st, campos=None, inverse_covariance: bool = False, accumulate: bool = False) -> dict:
    anchor = getattr(st, "_anchor", None)
    if anchor is None or anchor.device != st.param.device:
        anchor = st._anchor = torch.zeros(0, device=st.param.device, requires_grad=True)
    if campos is not None:
        campos = campos.detach()
    outs = _Activate.apply(anchor, st, campos, bool(inverse_covariance), accumulate)
    return dict(zip(_output_names(st, campos, inverse_covariance), outs))


__all__ = ["activate"]
