"""Float64 restatements of the rasterizer's two differentiable stages, in torch with autograd.

Test infrastructure only (not collected: no test_ prefix). Two functions restate what the oracle's C
does, independently of it, so that tests/test_ref64.py can hold the oracle's analytic backward to the
derivative of a plain high-precision forward:

  * per_gaussian: mean -> NDC / view depth, (scale, quaternion) -> cov3D -> cov2D -> conic, SH -> rgb
    (forward.cu preprocessCUDA, backward.cu computeCov2DCUDA / computeCov3D / preprocessCUDA);
  * tile_blend: the per-pixel front-to-back blend over the oracle's own tile ranges and point list
    (forward.cu / backward.cu renderCUDA).

Where the reference's backward is NOT the derivative of its forward, the departure is written as a
`detach` with a comment naming the reference line. The keyword switches `clamp`, `scale_grad` and
`alpha_cap` exist for the mutation tests only: they replace one such convention by a plausible wrong
one, which must then fail the bar.
"""
from __future__ import annotations

import numpy as np
import torch

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)

BLOCK = 16
ALPHA_MIN = 1.0 / 255.0
T_MIN = 1e-4
NEAR = 1e-5  # a pair within this (relative) of a skip threshold may fall on either side in f32


def _t(a, dtype, grad=False):
    x = torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    return x.requires_grad_(True) if grad else x


def _scale_grad(x, k):
    """x in the forward, k * dx in the backward (k carries no gradient)."""
    k = k.detach()
    return x * k + (x - x * k).detach()


def sh_colour(dirs, sh, degree):
    """Colour of degree `degree` from sh [P, M >= (degree + 1)^2, 3] along unit dirs [P, 3], before the + 0.5."""
    x, y, z = (dirs[:, i:i + 1] for i in range(3))
    r = C0 * sh[:, 0]
    if degree > 0:
        r = r - C1 * y * sh[:, 1] + C1 * z * sh[:, 2] - C1 * x * sh[:, 3]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        r = (r + C2[0] * xy * sh[:, 4] + C2[1] * yz * sh[:, 5] + C2[2] * (2 * zz - xx - yy) * sh[:, 6]
             + C2[3] * xz * sh[:, 7] + C2[4] * (xx - yy) * sh[:, 8])
    if degree > 2:
        r = (r + C3[0] * y * (3 * xx - yy) * sh[:, 9] + C3[1] * xy * z * sh[:, 10]
             + C3[2] * y * (4 * zz - xx - yy) * sh[:, 11] + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12]
             + C3[4] * x * (4 * zz - xx - yy) * sh[:, 13] + C3[5] * z * (xx - yy) * sh[:, 14]
             + C3[6] * x * (xx - 3 * yy) * sh[:, 15])
    return r


def per_gaussian(cam, means3D, scales=None, rotations=None, sh=None, degree=3, scale_modifier=1.0, cov3D=None,
                 dtype=torch.float64, clamp="reference", scale_grad="s"):
    """The per-Gaussian chain on every row of means3D (the caller passes visible Gaussians only).

    Returns a dict: `ndc` [P, 2], `depth` [P] (view-space z), `conic` [P, 3] (xx, xy, yy), `rgb` [P, 3]
    (None without sh), and the tensors gradients are read from: `means3D`, `cov6` (the six upper
    entries of cov3D; a leaf when cov3D is given), `s` (the scale gradient's variable), `rotations`,
    `sh`. clamp: "reference" | "autograd" | "off"; scale_grad: "s" | "scale"."""
    m = _t(means3D, dtype, True)
    view, proj = _t(cam.view, dtype), _t(cam.proj, dtype)
    campos = _t(cam.campos, dtype)
    out = {"means3D": m}
    # row-vector convention: p_view = [p, 1] @ view, p_hom = [p, 1] @ proj
    t = m @ view[:3, :3] + view[3, :3]
    ph = m @ proj[:3, :] + proj[3, :]
    out["ndc"] = ph[:, :2] / (ph[:, 3:4] + 1e-7)
    out["depth"] = t[:, 2]

    if cov3D is not None:
        cov6 = _t(cov3D, dtype, True)
        out["s"] = out["rotations"] = None
    else:
        q = _t(rotations, dtype, True)  # raw quaternion (r, x, y, z): never normalised (forward.cu computeCov3D)
        if scale_grad == "s":
            # backward.cu:297 `s = mod * scale` and :325-327 report dL/ds as dL_dscale, without the factor mod
            s = _t(np.asarray(scales, np.float64) * float(np.float32(scale_modifier)), dtype, True)
            out["s"] = s
        else:  # mutation: the true derivative with respect to `scale`
            out["s"] = _t(scales, dtype, True)
            s = out["s"] * float(np.float32(scale_modifier))
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)], 1),
                         torch.stack([2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)], 1),
                         torch.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], 1)], 1)
        M = s[:, :, None] * R
        Sigma = M.transpose(1, 2) @ M
        cov6 = torch.stack([Sigma[:, 0, 0], Sigma[:, 0, 1], Sigma[:, 0, 2], Sigma[:, 1, 1], Sigma[:, 1, 2],
                            Sigma[:, 2, 2]], 1)
        if cov6.requires_grad:
            cov6.retain_grad()
        out["rotations"] = q
    out["cov6"] = cov6
    # each off-diagonal entry of cov6 fills both symmetric places: its gradient is their sum (backward.cu:226-228)
    i6 = torch.tensor([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    V = cov6[:, i6]

    fx, fy = cam.width / (2.0 * cam.tanfovx), cam.height / (2.0 * cam.tanfovy)
    tz = t[:, 2]
    lim = (1.3 * cam.tanfovx, 1.3 * cam.tanfovy)
    txy = []
    for i in range(2):
        ratio = t[:, i] / tz
        if clamp == "off":
            txy.append(t[:, i])
        elif clamp == "autograd":
            txy.append(torch.clamp(ratio, -lim[i], lim[i]) * tz)
        else:
            # backward.cu:173-177, :263-265: a clamped t.x is a constant of the backward (x_grad_mul = 0 and no
            # d(lim * t.z)/dt.z term in dL_dtz); an unclamped one is t.x itself
            outside = (ratio.detach() < -lim[i]) | (ratio.detach() > lim[i])
            txy.append(torch.where(outside, (torch.clamp(ratio, -lim[i], lim[i]) * tz).detach(), t[:, i]))
    j00, j11 = fx / tz, fy / tz
    j20, j21 = -(fx * txy[0]) / (tz * tz), -(fy * txy[1]) / (tz * tz)
    W3 = view[:3, :3]
    g0 = W3[None, :, 0] * j00[:, None] + W3[None, :, 2] * j20[:, None]
    g1 = W3[None, :, 1] * j11[:, None] + W3[None, :, 2] * j21[:, None]
    Vg0 = (V @ g0[:, :, None])[:, :, 0]
    Vg1 = (V @ g1[:, :, None])[:, :, 0]
    a = (g0 * Vg0).sum(1) + 0.3
    b = (g1 * Vg0).sum(1)
    c = (g1 * Vg1).sum(1) + 0.3
    det = a * c - b * b
    conic = torch.stack([c, -b, a], 1) / det[:, None]
    # backward.cu:204 denom2inv = 1 / (denom^2 + 1e-7) multiplies every dconic/d(a, b, c): the true 1 / denom^2
    # scaled by denom^2 / (denom^2 + 1e-7)
    out["conic"] = _scale_grad(conic, (det * det / (det * det + 1e-7))[:, None])

    out["sh"] = out["rgb"] = None
    if sh is not None:
        shs = _t(sh, dtype, True)
        d = m - campos
        d = d / torch.sqrt((d * d).sum(1, keepdim=True))
        out["rgb"] = torch.clamp_min(sh_colour(d, shs, degree) + 0.5, 0.0)
        out["sh"] = shs
    return out


def per_gaussian_backward(cam, visible, dL_dmean2D, dL_dconic, dL_dcolor, means3D, scales=None, rotations=None,
                          sh=None, degree=3, scale_modifier=1.0, cov3D=None, dtype=torch.float64, **switches):
    """Gradients of  sum d2.xy ndc.xy + d2.z depth + dc.x conic_xx + 2 dc.y conic_xy + dc.w conic_yy + dcol rgb
    over the `visible` Gaussians (the blend stores half of the off-diagonal conic gradient, backward.cu:607), as
    float64 numpy arrays of the full size, zero on the rest: the contract of BACKWARD::preprocess."""
    idx = np.nonzero(visible)[0]
    sub = lambda a: None if a is None else np.asarray(a)[idx]  # noqa: E731
    o = per_gaussian(cam, sub(means3D), sub(scales), sub(rotations), sub(sh), degree, scale_modifier, sub(cov3D),
                     dtype, **switches)
    d2, dcn = _t(sub(dL_dmean2D), dtype), _t(sub(dL_dconic), dtype)
    loss = (d2[:, :2] * o["ndc"]).sum() + (d2[:, 2] * o["depth"]).sum()
    loss = loss + (dcn[:, 0] * o["conic"][:, 0] + 2 * dcn[:, 1] * o["conic"][:, 1] + dcn[:, 3] * o["conic"][:, 2]).sum()
    if o["rgb"] is not None:
        loss = loss + (_t(sub(dL_dcolor), dtype) * o["rgb"]).sum()
    loss.backward()
    P = np.asarray(means3D).shape[0]

    def full(x, shape):
        g = np.zeros((P,) + shape)
        if x is not None and x.grad is not None:
            g[idx] = x.grad.double().numpy()
        return g

    M = 0 if sh is None else np.asarray(sh).shape[1]
    return {"dL_dmeans3D": full(o["means3D"], (3,)), "dL_dcov3D": full(o["cov6"], (6,)),
            "dL_dscales": full(o["s"], (3,)), "dL_drotations": full(o["rotations"], (4,)),
            "dL_dsh": full(o["sh"], (M, 3))}


def tile_blend(W, H, ranges, point_list, means2D, depths, conic, opacity, colors, features, bg, upstream=None,
               dtype=torch.float64, alpha_cap=True):
    """forward.cu / backward.cu renderCUDA, one 16 x 16 tile at a time over the given ranges and point list.
    means2D in pixels, conic [P, 3] = (xx, xy, yy). Returns float64 numpy arrays: `color` [H, W, 3], `opacity`,
    `depth` [H, W], `feature` [H, W, S], `final_T` [H, W]; `near` [H, W] (a pair of the pixel sits within NEAR of
    a skip threshold), `capped` [P] (contributing pairs per Gaussian whose opacity * G exceeds 0.99); and, with
    upstream = (dcolor [3, H, W], dopacity [H W], ddepth [H W], dfeature [S, H, W]), the gradients of
    sum upstream * output in the reference's units."""
    P = np.asarray(means2D).shape[0]
    S = np.asarray(features).shape[1]
    grad = upstream is not None
    m2, dep, con = _t(means2D, dtype, grad), _t(depths, dtype, grad), _t(conic, dtype, grad)
    op, col, feat = _t(np.asarray(opacity).reshape(-1), dtype, grad), _t(colors, dtype, grad), _t(features, dtype, grad)
    bgt = _t(bg, dtype)
    img = {"color": torch.zeros(H, W, 3, dtype=dtype), "opacity": torch.zeros(H, W, dtype=dtype),
           "depth": torch.zeros(H, W, dtype=dtype), "feature": torch.zeros(H, W, S, dtype=dtype),
           "final_T": torch.ones(H, W, dtype=dtype)}
    near = torch.zeros(H, W, dtype=torch.bool)
    capped = torch.zeros(P, dtype=torch.long)
    if grad:
        uc, uo, ud, uf = upstream
        uc = _t(uc, dtype).reshape(3, H, W).permute(1, 2, 0)
        uo, ud = _t(uo, dtype).reshape(H, W), _t(ud, dtype).reshape(H, W)
        uf = _t(uf, dtype).reshape(S, H, W).permute(1, 2, 0)
    loss = torch.zeros((), dtype=dtype)
    gx, gy = (W + BLOCK - 1) // BLOCK, (H + BLOCK - 1) // BLOCK
    plist = torch.as_tensor(np.asarray(point_list).astype(np.int64))
    with torch.set_grad_enabled(grad):
        for ty in range(gy):
            for tx in range(gx):
                r0, r1 = (int(v) for v in ranges[ty * gx + tx])
                y0, y1, x0, x1 = ty * BLOCK, min(ty * BLOCK + BLOCK, H), tx * BLOCK, min(tx * BLOCK + BLOCK, W)
                hh, ww = y1 - y0, x1 - x0
                ids = plist[r0:r1]
                n = ids.numel()
                if n == 0:
                    img["color"][y0:y1, x0:x1] = bgt
                    continue
                py, px = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
                pxf, pyf = px.reshape(-1).to(dtype), py.reshape(-1).to(dtype)
                dx = m2[ids, 0:1] - pxf[None]
                dy = m2[ids, 1:2] - pyf[None]
                c = con[ids]
                power = -0.5 * (c[:, 0:1] * dx * dx + c[:, 2:3] * dy * dy) - c[:, 1:2] * dx * dy
                oG = op[ids, None] * torch.exp(power)
                # backward.cu:528, :594: alpha = min(0.99, o G), yet dL_dG = o dL_dalpha also where the cap is
                # active: straight-through
                alpha = oG + (torch.clamp(oG, max=0.99) - oG).detach() if alpha_cap else oG
                pw, al = power.detach(), alpha.detach()
                skip = (pw > 0) | (al < ALPHA_MIN)                              # forward.cu `continue`s
                a_eff = torch.where(skip, torch.zeros_like(alpha), alpha)
                T_all = torch.cumprod(1 - a_eff.detach(), 0)
                live = T_all >= T_MIN                                           # forward.cu `done` (T only falls)
                a_live = torch.where(live, a_eff, torch.zeros_like(alpha))
                T_incl = torch.cumprod(1 - a_live, 0)
                T_excl = torch.cat([torch.ones_like(T_incl[:1]), T_incl[:-1]], 0)
                w = a_live * T_excl
                T_fin = T_incl[-1]
                o_col = w.t() @ col[ids] + T_fin[:, None] * bgt
                o_op = w.sum(0)
                o_dep = w.t() @ dep[ids]
                o_feat = w.t() @ feat[ids]
                img["color"][y0:y1, x0:x1] = o_col.detach().reshape(hh, ww, 3)
                img["opacity"][y0:y1, x0:x1] = o_op.detach().reshape(hh, ww)
                img["depth"][y0:y1, x0:x1] = o_dep.detach().reshape(hh, ww)
                img["feature"][y0:y1, x0:x1] = o_feat.detach().reshape(hh, ww, S)
                img["final_T"][y0:y1, x0:x1] = T_fin.detach().reshape(hh, ww)
                # pairs the walk reaches, with NEAR of slack on the stop itself
                reached = torch.cat([torch.ones_like(T_all[:1]), T_all[:-1]], 0) >= T_MIN * (1 - NEAR)
                close = reached & ((pw.abs() < NEAR) | ((pw <= 0) & ((al - ALPHA_MIN).abs() < NEAR * ALPHA_MIN))
                                   | (~skip & ((T_all - T_MIN).abs() < NEAR * T_MIN)))
                near[y0:y1, x0:x1] = close.any(0).reshape(hh, ww)
                capped.index_add_(0, ids, ((oG.detach() > 0.99) & ~skip & live).sum(1))
                if grad:
                    loss = loss + (o_col * uc[y0:y1, x0:x1].reshape(-1, 3)).sum() \
                        + (o_op * uo[y0:y1, x0:x1].reshape(-1)).sum() + (o_dep * ud[y0:y1, x0:x1].reshape(-1)).sum() \
                        + (o_feat * uf[y0:y1, x0:x1].reshape(-1, S)).sum()
    res = {k: v.double().numpy() for k, v in img.items()}
    res["near"] = near.numpy()
    res["capped"] = capped.numpy()
    if grad:
        loss.backward()
        g = lambda x: torch.zeros_like(x).double().numpy() if x.grad is None else x.grad.double().numpy()  # noqa: E731
        gm, gc = g(m2), g(con)
        # the reference reports dL/dmean2D per NDC unit (backward.cu:481-482 ddelx_dx = 0.5 W) and the view-depth
        # gradient in its third column (:603); dL_dconic.y holds half of the off-diagonal's gradient (:607)
        res["dL_dmeans2D"] = np.stack([gm[:, 0] * 0.5 * W, gm[:, 1] * 0.5 * H, g(dep)], 1)
        res["dL_dconic"] = np.stack([gc[:, 0], 0.5 * gc[:, 1], np.zeros(P), gc[:, 2]], 1)
        res["dL_dopacity"] = g(op).reshape(P, 1)
        res["dL_dcolors"] = g(col)
        res["dL_dfeatures"] = g(feat)
    return res
