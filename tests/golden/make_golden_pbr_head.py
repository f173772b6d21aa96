"""Golden vectors for the PBR image head and the light regulariser (relightable3dgaussian_amd/pbr.py), from the
REFERENCE's float32 torch code on CPU tensors.

utils/graphics_utils.py is loaded by file, so the ACES `hdr2ldr` is the reference's own, and utils/loss_utils.py
likewise for the call-site case's `ssim`. gaussian_renderer/neilf.py and scene/gamma_trans.py import native and
argument modules and cannot be imported without them, so their lines (neilf.py:169-175, 278-283 and
gamma_trans.py:45-51) are restated here in this project's own words, one float32 tensor operation per
operation of the reference, so that the float32 evaluation rounds where the reference's does. Gradients are
torch autograd's on those expressions, with the fixed upstream G: L = sum(image * G).

  pbr_head.npz
    head, head_full            the head cases; those of head_full hold every float64 result, the others (the
                               large shape, kept under the size limit) inputs, the exact float32 image and floors
    <case>/pbr [H,W,3], opacity [H,W,1], bg [3], bgimg [H,W,3], G [H,W,3], gamma [1], all float32 ("hwc"; a
                               "chw" run permutes inputs and results)
    <case>/<vec|img>/f32/y_none, y_clamp   the float32 images of the two exact modes (bg [3] | per-pixel bgimg)
    <case>/<vec|img>/f64/y_gamma, y_aces, d_pbr_gamma, d_opacity_gamma, d_gamma, d_opacity_none
    <case>/floor/<output>      the distance of the float32 evaluation from the float64 one in the measure of
                               tests/pbr_ref64.py (rel_err; gradients without the pixels near a clamp bound),
                               the larger of the two bg kinds
    edge_g<gamma>              1 x 5 images with opacity 1 and x = 1, nextafter(1, 2), lo, 0, -0.5 on every channel
    callsite/gt [3,33,31], gamma [1], f64/d_pbr, d_opacity, d_gamma, floor/...   head("gamma") on r_33x31's inputs
                               -> (1 - 0.2) L1 + 0.2 (1 - SSIM) against gt -> backward
    light                      the stored light cases' P; light_<P>/d [P,3], f64/value, f64/grad, floor/value,
                               floor/grad; light_drawn = (P, seed) of the case tests draw again with
                               tests/pbr_ref64.draw_light (too large to store), with its floors

Usage:  python tests/golden/make_golden_pbr_head.py --reference <checkout of the reference project>
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import pbr_ref64 as p64  # noqa: E402

SHAPES = [(1, 1), (1, 3), (2, 2), (5, 7), (16, 16), (33, 31), (67, 131)]
FULL_BELOW = 2000  # pixels: larger shapes store no float64 arrays
GAMMAS = (0.45, 2.2, 1.0)
LIGHT_P = (1, 3, 4, 255, 256, 257, 1025)
LIGHT_DRAWN = (70001, 70001)  # P, seed
LAMBDA_DSSIM = 0.2
f32 = np.float32


def load(reference: str, rel: str):
    """A module of the reference's utils package by file, under a stub package so that its relative imports
    resolve to the files next to it."""
    pkg = "r3dg_reference_utils"
    if pkg not in sys.modules:
        stub = types.ModuleType(pkg)
        stub.__path__ = [os.path.join(reference, "utils")]
        sys.modules[pkg] = stub
    name = pkg + "." + os.path.basename(rel)[:-3]
    spec = importlib.util.spec_from_file_location(name, os.path.join(reference, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def draw_head(rng, h, w, gamma):
    """x spreads over [-0.15, 2.25]: both clamp bounds of both clamping modes are crossed. bgimg and G are
    multiples of 1/256 and 1/64 (they compress; the roundings under test are the composite's and the tone's)."""
    c = {"pbr": rng.uniform(-0.15, 1.25, (h, w, 3)).astype(f32), "opacity": rng.uniform(0, 1, (h, w, 1)).astype(f32),
         "bg": rng.uniform(0, 1, 3).astype(f32), "bgimg": (rng.integers(0, 257, (h, w, 3)) / 256).astype(f32),
         "G": (rng.integers(-64, 65, (h, w, 3)) / 64).astype(f32), "gamma": np.array([gamma], f32)}
    c["opacity"].flat[0] = 1.0
    if h * w > 1:
        c["opacity"].flat[1] = 0.0
    return c


def edge_case(rng, gamma):
    lo = f32(1e-9)
    x = np.array([1.0, np.nextafter(f32(1), f32(2)), lo, 0.0, -0.5], f32)
    c = draw_head(rng, 1, 5, gamma)
    c["pbr"] = np.repeat(x[None, :, None], 3, 2).astype(f32)
    c["opacity"][:] = 1.0
    c["G"] = np.where(c["G"] == 0, f32(0.5), c["G"]).astype(f32)
    return c


def head(gu, c, bgk, tone, dt):
    """-> (image, (d_pbr, d_opacity, d_gamma or None)) as numpy, evaluated in dtype dt with the reference's sequence."""
    t = {k: torch.from_numpy(v).to(dt) for k, v in c.items()}
    pbr, opacity, gamma = t["pbr"].requires_grad_(True), t["opacity"].requires_grad_(True), t["gamma"].requires_grad_(True)
    bg = t["bg"][None, None, :] if bgk == "vec" else t["bgimg"]
    x = pbr + (1 - opacity) * bg                                   # neilf.py:170
    if tone == "none":
        y = x
    elif tone == "gamma":                                          # gamma_trans.py:47-48
        y = x.clamp(1e-9 if dt == torch.float32 else p64.LO, 1) ** gamma
    elif tone == "aces":
        y = gu.hdr2ldr(x)                                          # graphics_utils.py:197-201, the reference's own
    else:
        y = torch.clamp(x, 0, 1)
    grads = None
    if tone in ("none", "gamma"):
        g = torch.autograd.grad((y * t["G"]).sum(), [pbr, opacity] + ([gamma] if tone == "gamma" else []))
        grads = tuple(a.numpy() for a in g) + ((None,) if tone == "none" else ())
    return y.detach().numpy(), grads


def head_case(gu, name, c, out, full):
    floors = {}
    for bgk in ("vec", "img"):
        bg = c["bg"] if bgk == "vec" else c["bgimg"]
        skip = p64.near_clamp_bound(c["pbr"], c["opacity"], bg)
        assert skip.mean() <= p64.MAX_LEFT_OUT, (name, bgk, skip.mean())
        res = {}
        for tone in p64.TONES:
            y32, g32 = head(gu, c, bgk, tone, torch.float32)
            y64, g64 = head(gu, c, bgk, tone, torch.float64)
            assert y32.dtype == f32 and y64.dtype == np.float64
            # this project's float64 restatement is the yardstick of the GPU tests: it must be the autograd result
            mine = p64.head_forward(c["pbr"], c["opacity"], bg, c["gamma"], tone)
            assert p64.rel_err(mine, y64) <= 1e-14, (name, bgk, tone)
            if tone in ("none", "clamp"):
                out[f"{name}/{bgk}/f32/y_{tone}"] = y32
                assert p64.rel_err(y32, y64) <= 2.0 ** -23, (name, tone)
            else:
                res[f"y_{tone}"] = (y32, y64, None)
            if g64 is not None:
                mg = p64.head_backward(c["pbr"], c["opacity"], bg, c["G"], c["gamma"], tone)
                for a, b in zip(mg, g64):
                    assert (a is None) == (b is None) and (a is None or p64.rel_err(a, b) <= 1e-13), (name, bgk, tone)
                res[f"d_opacity_{tone}"] = (g32[1], g64[1], p64.pixel_mask(skip) if tone == "gamma" else None)
                if tone == "gamma":
                    res["d_pbr_gamma"] = (g32[0], g64[0], skip)
                    res["d_gamma"] = (g32[2], g64[2], None)
                else:
                    assert np.array_equal(g32[0], c["G"])  # d_pbr of "none" is the upstream itself
        for k, (a32, a64, m) in res.items():
            if full:
                out[f"{name}/{bgk}/f64/{k}"] = a64
            e = p64.rel_err(a32, a64) if m is None else p64.masked_rel_err(a32, a64, m)
            floors[k] = max(floors.get(k, 0.0), e)
    for k, v in floors.items():
        out[f"{name}/floor/{k}"] = np.float64(v)
    print(name, {k: f"{v:.2e}" for k, v in floors.items()})


def light(d, dt):
    """neilf.py:279-281 on a [P,3] tensor -> (value, gradient)."""
    t = torch.from_numpy(d).to(dt).requires_grad_(True)
    mean_light = t.mean(-1, keepdim=True).expand_as(t)
    loss = F.l1_loss(t, mean_light)
    g, = torch.autograd.grad(loss, t)
    return loss.detach().numpy(), g.numpy()


def light_case(name, d, out, store):
    v32, g32 = light(d, torch.float32)
    v64, g64 = light(d, torch.float64)
    skip = p64.ambiguous_sign(d)
    assert skip.mean() <= p64.MAX_LEFT_OUT, (name, skip.mean())
    assert abs(p64.light_loss(d) - float(v64)) <= 1e-14 * abs(float(v64))
    assert p64.rel_err(p64.light_loss_backward(d), g64) <= 1e-13
    if store:
        out[f"{name}/d"], out[f"{name}/f64/value"], out[f"{name}/f64/grad"] = d, np.float64(v64), g64
    out[f"{name}/floor/value"] = np.float64(p64.rel_err(v32, v64))
    out[f"{name}/floor/grad"] = np.float64(p64.masked_rel_err(g32, g64, skip))
    print(name, f"value {float(out[f'{name}/floor/value']):.2e} grad {float(out[f'{name}/floor/grad']):.2e}")


def callsite(lu, c, gt, dt):
    """head("gamma", bg [3]) -> calculate_loss's L1 + SSIM term (neilf.py:216-222) -> the three gradients."""
    from tests.test_image_loss import ssim64

    t = {k: torch.from_numpy(v).to(dt) for k, v in c.items()}
    pbr, opacity, gamma = t["pbr"].requires_grad_(True), t["opacity"].requires_grad_(True), t["gamma"].requires_grad_(True)
    x = pbr + (1 - opacity) * t["bg"][None, None, :]
    y = (x.clamp(1e-9 if dt == torch.float32 else p64.LO, 1) ** gamma).permute(2, 0, 1)
    g = torch.from_numpy(gt).to(dt)
    s = lu.ssim(y, g) if dt == torch.float32 else ssim64(y, g)
    loss = (1.0 - LAMBDA_DSSIM) * F.l1_loss(y, g) + LAMBDA_DSSIM * (1.0 - s)
    return [a.numpy() for a in torch.autograd.grad(loss, [pbr, opacity, gamma])]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    a = ap.parse_args()
    gu = load(a.reference, "utils/graphics_utils.py")
    lu = load(a.reference, "utils/loss_utils.py")
    rng = np.random.default_rng(2026)
    out, names, full_names, cases = {}, [], [], {}
    for i, (h, w) in enumerate(SHAPES):
        cases[f"r_{h}x{w}"] = draw_head(rng, h, w, GAMMAS[i % 3])
    for g in GAMMAS:
        cases[f"edge_g{g}"] = edge_case(rng, g)
    for name, c in cases.items():
        full = c["pbr"].shape[0] * c["pbr"].shape[1] < FULL_BELOW
        names.append(name)
        if full:
            full_names.append(name)
        for k, v in c.items():
            assert v.dtype == f32
            out[f"{name}/{k}"] = v
        head_case(gu, name, c, out, full)
    out["head"], out["head_full"] = np.array(names), np.array(full_names)

    c = dict(cases["r_33x31"], gamma=np.array([2.2], f32))
    gt = rng.uniform(0, 1, (3, 33, 31)).astype(f32)
    g32, g64 = callsite(lu, c, gt, torch.float32), callsite(lu, c, gt, torch.float64)
    skip = p64.near_clamp_bound(c["pbr"], c["opacity"], c["bg"])
    out["callsite/gt"], out["callsite/gamma"] = gt, c["gamma"]
    for k, a32, a64, m in zip(("d_pbr", "d_opacity", "d_gamma"), g32, g64, (skip, p64.pixel_mask(skip), None)):
        out[f"callsite/f64/{k}"] = a64
        out[f"callsite/floor/{k}"] = np.float64(p64.rel_err(a32, a64) if m is None else p64.masked_rel_err(a32, a64, m))
        print("callsite", k, f"{float(out[f'callsite/floor/{k}']):.2e}")

    for P in LIGHT_P:
        light_case(f"light_{P}", p64.draw_light(P, P), out, True)
    light_case("light_drawn", p64.draw_light(*LIGHT_DRAWN), out, False)
    out["light"], out["light_drawn"] = np.array(LIGHT_P), np.array(LIGHT_DRAWN)
    path = os.path.join(HERE, "pbr_head.npz")
    np.savez_compressed(path, **out)
    print("wrote pbr_head.npz", len(names), "head cases,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
