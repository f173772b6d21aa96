"""The display and capture head and the environment background on the MI355X (`display.frame_buffers`,
`relight.env_background`; csrc/display.hip, csrc/relight.hip) against the same work composed from torch tensor
operations the way the reference does it, in one process.

At 1920x1080 and 800x800, with the sources as block views of one [21 H W] feature buffer:
  captures   relighting.py's default --capture_list (:139), K = 10, "u8": the composites of :225-229 and
             torchvision's save_image conversion up to the bytes on the device (the copy to the host is the same
             for both forms and is not timed)
  gui depth  gui.py:145 with :162's repeat, "f32" (mode "range": three launches)
  gui pbr    gui.py:150 hdr2ldr, "f32"
  report     train.py:243-272's nine tiles up to the stacked [9,3,H,W] that make_grid receives, "f32"
  env map / env sh3   neilf_composite.py:210-215 with scene/cameras.py:87-99's direction image, for a 1024x2048
             map (the composed form runs EnvLight.direct_light, the kernel this project already had) and for
             degree-3 SH (eval_sh of utils/sh_utils.py:71-116 restated in torch)
Each pair is timed alternating, fused then composed, with CUDA events around one call: the median of --iters
calls after two warm-up calls. A single call includes launch latency and the host's work, for both forms.
Launches (kernels and device copies) come from one profiled call outside the timed window (null when the
profiler yields nothing). `share_of_copy_rate` is the fused form's algorithmic bytes over its single-call time
as a share of the 6.3 TB/s copy rate DESIGN.md section 2k uses. `forms_agree`: the two forms were compared once
at the timed size (bit for bit where every operation is exactly rounded, within 1e-5 for ACES and SH, in the mean
for the map lookup).

Usage: python tools/bench_display.py [--iters 20] [--out profiles/display/display_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.3e12  # B/s, DESIGN.md section 2k
C0, C1 = 0.28209479177387814, 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435]


def timed_pair(fused, composed, iters):
    for _ in range(2):
        fused()
        composed()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tf, tc = [], []
    for _ in range(iters):
        for fn, ts in ((fused, tf), (composed, tc)):
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ts.append(s.elapsed_time(e))
    return float(np.median(tf)), float(np.median(tc))


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = len([ev for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA")])
        return n or None
    except Exception:
        return None


def row(name, fused, composed, iters, bytes_, agree):
    f, c = timed_pair(fused, composed, iters)
    return {"what": name, "forms_agree": bool(agree), "fused_ms": f, "composed_ms": c, "ratio": c / f, "fused_launches": launches(fused),
            "composed_launches": launches(composed), "algorithmic_bytes": bytes_,
            "share_of_copy_rate": bytes_ / (f * 1e-3) / COPY_RATE}


def to_bytes(x):
    """save_image's conversion of a [C,H,W] image (make_grid triples one channel) up to the device bytes."""
    if x.shape[0] == 1:
        x = torch.cat((x, x, x), 0)
    return x.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)


def hdr2ldr(img, scale=0.666667):
    img = img * scale
    return (img * (2.51 * img + 0.03)) / (img * (2.43 * img + 0.59) + 0.14)


def frames(H, W, iters):
    from relightable3dgaussian_amd.display import frame_buffers

    n = H * W
    g = torch.Generator(device="cuda").manual_seed(H)
    feat = torch.rand(21 * n, device="cuda", generator=g) * 1.4 - 0.15
    blk = lambda at, c: feat[at * n:(at + c) * n].view(H, W, c)  # noqa: E731
    rgb, normal, base, rough, metal, pbr, pbr_env, shader, vis = (blk(0, 3), blk(3, 3), blk(6, 3), blk(9, 1), blk(10, 1),
                                                                  blk(11, 3), blk(14, 3), blk(17, 3), blk(20, 1))
    opacity = torch.rand(H, W, 1, device="cuda", generator=g)
    depth = torch.rand(H, W, 1, device="cuda", generator=g) * 7
    points, gt = torch.rand(3, H, W, device="cuda", generator=g), torch.rand(3, H, W, device="cuda", generator=g)
    chw = lambda t: t.permute(2, 0, 1)  # noqa: E731  the reference's tensors are [C,H,W]
    bg = 1
    rows = []
    with torch.no_grad():
        # ---- the relighting captures
        specs = [(base, "over", "none"), (metal, "over", "none"), (normal, "normal_over", "none"), (pbr, "plain", "none"),
                 (pbr_env, "plain", "none"), (shader, "plain", "none"), (points, "plain", "none", "chw"),
                 (rgb, "plain", "none"), (rough, "over", "none"), (vis, "over", "none")]
        ref = {"base_color": chw(base).contiguous(), "metallic": chw(metal).contiguous(), "normal": chw(normal).contiguous(),
               "pbr": chw(pbr).contiguous(), "pbr_env": chw(pbr_env).contiguous(), "shader": chw(shader).contiguous(),
               "points": points, "render": chw(rgb).contiguous(), "roughness": chw(rough).contiguous(),
               "visibility": chw(vis).contiguous(), "opacity": chw(opacity).contiguous()}

        def fused():
            return frame_buffers(specs, opacity=opacity, bg=bg, encoding="u8")

        def composed():
            out = []
            for k in ("base_color", "metallic", "normal", "pbr", "pbr_env", "shader", "points", "render", "roughness",
                      "visibility"):
                x = ref[k]
                if k == "normal":
                    x = x * 0.5 + 0.5
                    x = x + (1 - ref["opacity"]) * bg
                elif k in ("base_color", "roughness", "metallic", "visibility"):
                    x = x + (1 - ref["opacity"]) * bg
                out.append(to_bytes(x))
            return out

        agree = all(torch.equal(a, b) for a, b in zip(fused(), composed()))
        rows.append(row(f"captures K=10 u8 {W}x{H}", fused, composed, iters, (7 * 12 + 3 * 4 + 4 + 30) * n, agree))

        # ---- the GUI's depth view
        def fused():
            return frame_buffers([(depth, "range", "none")], encoding="f32")[0]

        def composed():
            out = (depth - depth.min()) / (depth.max() - depth.min())
            return out.repeat(1, 1, 3).contiguous()

        agree = torch.equal(fused(), composed())
        rows.append(row(f"gui depth f32 {W}x{H}", fused, composed, iters, (4 + 4 + 12) * n, agree))

        # ---- the GUI's pbr view with hdr2ldr
        def fused():
            return frame_buffers([(pbr, "plain", "aces")], encoding="f32")[0]

        def composed():
            return hdr2ldr(pbr).contiguous()

        agree = float((fused() - composed()).abs().max()) <= 1e-5
        rows.append(row(f"gui pbr aces f32 {W}x{H}", fused, composed, iters, (12 + 12) * n, agree))

        # ---- the evaluation report's nine tiles
        tiles = [(rgb, "plain", "clamp"), (pbr, "plain", "clamp"), (gt, "plain", "clamp", "chw"), (opacity, "plain", "clamp"),
                 (depth, "range", "none"), (normal, "normal_mask", "clamp"), (base, "plain", "clamp"),
                 (rough, "plain", "clamp"), (metal, "plain", "clamp")]
        ref["depth"] = chw(depth).contiguous()

        def fused():
            return frame_buffers(tiles, opacity=opacity, encoding="f32")

        def composed():
            image, image_pbr = ref["render"], ref["pbr"]
            o = torch.clamp(ref["opacity"], 0.0, 1.0)
            d = ref["depth"]
            d = (d - d.min()) / (d.max() - d.min())
            nrm = torch.clamp(ref["normal"] / 2 + 0.5 * o, 0.0, 1.0)
            b = torch.clamp(ref["base_color"], 0.0, 1.0)
            r = torch.clamp(ref["roughness"], 0.0, 1.0)
            m = torch.clamp(ref["metallic"], 0.0, 1.0)
            return torch.stack([torch.clamp(image, 0.0, 1.0), torch.clamp(image_pbr, 0.0, 1.0), torch.clamp(gt, 0.0, 1.0),
                                o.repeat(3, 1, 1), d.repeat(3, 1, 1), nrm, b, r.repeat(3, 1, 1), m.repeat(3, 1, 1)], dim=0)

        # opacity here is within [0, 1], so train.py:246's clamp of it changes nothing
        agree = torch.equal(fused(), composed().permute(0, 2, 3, 1))
        rows.append(row(f"report 9 tiles f32 {W}x{H}", fused, composed, iters, (5 * 12 + 4 * 4 + 4 + 4 + 9 * 12) * n, agree))
    return rows


def eval_sh3(sh, dirs):
    """utils/sh_utils.py:71-116 for degree 3: sh [..., C, 16], dirs [..., 3]."""
    x, y, z = dirs[..., 0:1], dirs[..., 1:2], dirs[..., 2:3]
    result = C0 * sh[..., 0] - C1 * y * sh[..., 1] + C1 * z * sh[..., 2] - C1 * x * sh[..., 3]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    result = (result + C2[0] * xy * sh[..., 4] + C2[1] * yz * sh[..., 5] + C2[2] * (2.0 * zz - xx - yy) * sh[..., 6] +
              C2[3] * xz * sh[..., 7] + C2[4] * (xx - yy) * sh[..., 8])
    return (result + C3[0] * y * (3 * xx - yy) * sh[..., 9] + C3[1] * xy * z * sh[..., 10] +
            C3[2] * y * (4 * zz - xx - yy) * sh[..., 11] + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[..., 12] +
            C3[4] * x * (4 * zz - xx - yy) * sh[..., 13] + C3[5] * z * (xx - yy) * sh[..., 14] +
            C3[6] * x * (xx - 3 * yy) * sh[..., 15])


def environment(H, W, iters):
    import torch.nn.functional as Fn

    from relightable3dgaussian_amd.relight import EnvLight, env_background

    g = torch.Generator(device="cuda").manual_seed(W)
    light = EnvLight(torch.rand(1024, 2048, 3, device="cuda", generator=g))
    shs = torch.randn(1, 16, 3, device="cuda", generator=g) * 0.3
    K = torch.tensor([[1.1 * W, 0, W / 2 + 3.5], [0, 1.1 * W, H / 2 - 2.25], [0, 0, 1]], device="cuda")
    c2w = torch.eye(4, device="cuda")
    c2w[:3, :3] = torch.linalg.qr(torch.randn(3, 3, device="cuda", generator=g))[0]

    def directions():  # scene/cameras.py:87-99
        v, u = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
        d = torch.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], torch.ones_like(u)], dim=0)
        d = Fn.normalize(d, dim=0)
        return (c2w[:3, :3] @ d.reshape(3, -1)).reshape(3, H, W)

    rows = []
    with torch.no_grad():
        def fused():
            return env_background(light, K, c2w, H, W)

        def composed():
            return light.direct_light(directions().permute(1, 2, 0)).permute(2, 0, 1)

        # a direction one rounding apart can sit in the next texel of a random map: the mean says the rest
        agree = float((fused() - composed().permute(1, 2, 0)).abs().mean()) <= 1e-3
        rows.append(row(f"env map 1024x2048 {W}x{H}", fused, composed, iters, 12 * H * W, agree))

        def fused():
            return env_background(shs, K, c2w, H, W)

        def composed():
            sv = shs.transpose(1, 2).unsqueeze(1)
            return torch.clamp_min(eval_sh3(sv, directions().permute(1, 2, 0)) + 0.5, 0).permute(2, 0, 1)

        agree = float((fused() - composed().permute(1, 2, 0)).abs().max()) <= 1e-5
        rows.append(row(f"env sh3 {W}x{H}", fused, composed, iters, 12 * H * W, agree))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "display", "display_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_display: needs the GPU (no CPU path, and a CPU time says nothing)")
    rows = []
    for H, W in ((1080, 1920), (800, 800)):
        rows += frames(H, W, args.iters) + environment(H, W, args.iters)
    line = json.dumps({"copy_rate_Bps": COPY_RATE, "iters": args.iters, "warmup": 2,
                       "timing": "CUDA events around one call (launch latency and host work included), fused and "
                                 "composed alternating, median", "rows": rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
