"""The display and capture head (csrc/display.hip; semantics in include/r3dg_hip.h `r3dg_display_frame`): from
the rasterizer's buffers to the images that are copied to the host, all of a frame's in one launch.

`frame_buffers(specs, opacity=None, bg=None, encoding="u8")` -> [K,H,W,3], uint8 or float32. `specs` is a list
of 1 to 16 entries `(source, mode, tone)` or `(source, mode, tone, "chw")`. A source is a float32 [H,W,1] or
[H,W,3] tensor, the rasterizer's outputs and the block views of its feature buffer as they are; with "chw" it
is [1,H,W] or [3,H,W] (gt_image). A one-channel source gives three equal channels. With s the source,
o = `opacity` [H,W,1] and b = `bg`, every operation float32 and rounded on its own:
  mode "plain"        y = s
       "over"         y = s + (1 - o) * b                  relighting.py:229
       "normal_over"  y = (s * 0.5 + 0.5) + (1 - o) * b    relighting.py:226-227
       "normal_mask"  y = s * 0.5 + 0.5 * o                gui.py:167, train.py:249-250
       "range"        y = (s - mn) / (mx - mn)             gui.py:145, train.py:248: mn, mx over every element of
                      this spec's source; a NaN in it makes every y NaN (torch.min); mx == mn gives what the
                      division gives
       "count"        y = float(min(s, 1000)) / 1000       gui.py:147: the int32 [H,W,1] contribution map
  tone "none" | "clamp" clamp(y, 0, 1), a NaN stays NaN | "aces" hdr2ldr of utils/graphics_utils.py:197-201
  encoding "f32"  y as it is (the GUI's raw texture)
           "u8"   floor(clamp(y * 255 + 0.5, 0, 255)), torchvision's save_image; a NaN gives 0: the reference casts
                  a NaN to uint8, which is undefined, so no value is the reference's there
`bg` is a [3] tensor, a Python number (relighting's scalar bg, passed to the kernel by value) or an [H,W,3]
image (`relight.env_background`). Everything but the "aces" tone is exactly rounded: those images are the
reference's bits. The result is always a fresh contiguous tensor.

One launch; two more when any spec has mode "range" (min and max of all such sources, deterministic), however
many do. Nothing synchronises with the host. Forward only. No CPU path and no torch fallback: the extension
rejects CPU tensors.
"""
from __future__ import annotations

import torch

from . import _C

_MODES = dict(_C.display.MODES)
_TONES = dict(_C.display.TONES)
_ENCODINGS = dict(_C.display.ENCODINGS)
MAX_SPECS = int(_C.display.MAX_SPECS)
_NEED_OPACITY = ("over", "normal_over", "normal_mask")
_NEED_BG = ("over", "normal_over")


def frame_buffers(specs, opacity: torch.Tensor | None = None, bg=None, encoding: str = "u8") -> torch.Tensor:
    """[K,H,W,3] uint8 ("u8") or float32 ("f32") from K specs (source, mode, tone[, "chw"]) in one launch."""
    who = "frame_buffers"
    if encoding not in _ENCODINGS:
        raise ValueError(f"{who}: encoding one of {sorted(_ENCODINGS)} expected, got {encoding!r}")
    specs = list(specs)
    if not 1 <= len(specs) <= MAX_SPECS:
        raise ValueError(f"{who}: 1 to {MAX_SPECS} specs expected, got {len(specs)}")
    sources, modes, tones, chws, hw = [], [], [], [], None
    for k, spec in enumerate(specs):
        if not isinstance(spec, (tuple, list)) or len(spec) not in (3, 4):
            raise ValueError(f"{who}: spec {k}: (source, mode, tone) or (source, mode, tone, 'chw') expected")
        src, mode, tone = spec[:3]
        layout = spec[3] if len(spec) == 4 else "hwc"
        if layout not in ("chw", "hwc"):
            raise ValueError(f"{who}: spec {k}: layout 'chw' or 'hwc' expected, got {layout!r}")
        if mode not in _MODES:
            raise ValueError(f"{who}: spec {k}: mode one of {sorted(_MODES)} expected, got {mode!r}")
        if tone not in _TONES:
            raise ValueError(f"{who}: spec {k}: tone one of {sorted(_TONES)} expected, got {tone!r}")
        want = torch.int32 if mode == "count" else torch.float32
        if not isinstance(src, torch.Tensor) or src.dtype != want:
            raise ValueError(f"{who}: spec {k}: source: {'an int32' if mode == 'count' else 'a float32'} tensor "
                             f"expected with mode {mode!r}")
        chw = layout == "chw"
        c = 0 if chw else 2
        if src.dim() != 3 or src.shape[c] not in ((1,) if mode == "count" else (1, 3)) or src.numel() == 0:
            raise ValueError(f"{who}: spec {k}: shape mismatch: source {'[1|3,H,W]' if chw else '[H,W,1|3]'} with "
                             f"H, W >= 1 expected in layout {layout!r}"
                             f"{' (one channel with mode count)' if mode == 'count' else ''}, got {tuple(src.shape)}")
        this = tuple(src.shape[1:]) if chw else tuple(src.shape[:2])
        hw = hw or this
        if this != hw:
            raise ValueError(f"{who}: spec {k}: shape mismatch: every source must be {hw[0]} x {hw[1]}, got "
                             f"{this[0]} x {this[1]}")
        if mode in _NEED_OPACITY and opacity is None:
            raise ValueError(f"{who}: spec {k}: mode {mode!r} needs opacity")
        if mode in _NEED_BG and bg is None:
            raise ValueError(f"{who}: spec {k}: mode {mode!r} needs bg")
        sources.append(src), modes.append(_MODES[mode]), tones.append(_TONES[tone]), chws.append(chw)
    if opacity is not None:
        if not isinstance(opacity, torch.Tensor) or opacity.dtype != torch.float32:
            raise ValueError(f"{who}: opacity: a float32 tensor expected")
        if tuple(opacity.shape) != hw + (1,):
            raise ValueError(f"{who}: shape mismatch: opacity [H,W,1] = {hw + (1,)} expected, got {tuple(opacity.shape)}")
    bg_dev, bg_value = None, []
    if isinstance(bg, torch.Tensor):
        if bg.dtype != torch.float32:
            raise ValueError(f"{who}: bg: a float32 tensor expected")
        if tuple(bg.shape) != (3,) and tuple(bg.shape) != hw + (3,):
            raise ValueError(f"{who}: shape mismatch: bg [3], a number or an [H,W,3] image expected, got {tuple(bg.shape)}")
        bg_dev = bg
    elif bg is not None:
        if isinstance(bg, bool) or not isinstance(bg, (int, float)):
            raise ValueError(f"{who}: bg: a float32 tensor [3] or [H,W,3] or a number expected, got {type(bg).__name__}")
        bg_value = [float(bg)] * 3
    tensors = [(f"spec {k}: source", s) for k, s in enumerate(sources)] + [("opacity", opacity), ("bg", bg_dev)]
    for name, t in tensors:
        if t is not None and t.device != sources[0].device:
            raise ValueError(f"{who}: {name} is on {t.device}, spec 0's source on {sources[0].device}: one device expected")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for _, t in tensors):
        raise ValueError(f"{who}: forward only: detach the inputs, or call under no_grad")
    return _C.display.frame(sources, modes, tones, chws, opacity, bg_dev, bg_value, _ENCODINGS[encoding])


__all__ = ["frame_buffers", "MAX_SPECS"]
