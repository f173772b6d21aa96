"""Generate tests/golden/relight.npz from the REFERENCE's own relighting render equation (CPU).

Runs gaussian_renderer/neilf_composite.py rendering_equation_python (is_training=False) and
scene/envmap.py EnvLight.direct_light of the reference checkout on seeded inputs and stores inputs and
outputs only (data, no reference source). The reference is imported as tests/golden/make_golden.py does
it (stub modules for the CUDA-only imports, device='cuda' rewritten to CPU), plus:

  scene.derect_light_sh  a stub with a DirectLightEnv class, so that the reference's isinstance takes
                         its SH branch for the SH light
  cv2, nvdiffrast.torch  stubs. nvdiffrast is not installable here; the stub's texture() is the filter of
                         dr.texture(filter_mode='linear') with the default boundary_mode='wrap' as
                         nvdiffrast documents it: u <- u - floor(u), x = u W - 0.5, x0 = floor(x), weight
                         x - x0, texels x0 and x0 + 1 modulo W, the same in v with H. The reference's
                         EnvLight is built without its __init__ (which reads an .hdr file through cv2), so
                         its own direct_light body supplies the direction -> texture coordinate mapping.
                         tests/test_relight_ref.py pins the same filter to torch's grid_sample.

Inputs: P = 64 with Ns = 24 ("s24") and P = 8 with Ns = 384 ("s384"), drawn like make_golden.brdf_inputs
(roughness in [0.05, 1]) with 16 incident, 16 environment and 25 visibility coefficients. Cases:
  a  baked visibility (25 coefficients), SH light (16), 16 incident coefficients
  b  traced visibility, a 6 x 10 random HDR-range map with a random rotation
  c  traced visibility, no light
and "lookup": EnvLight.direct_light alone on 256 random unit directions, with and without the rotation.

The archive is written with fixed zip timestamps and one thread, so it regenerates byte for byte.

Usage:  python tests/golden/make_golden_relight.py [--reference /root/reference]
        python tests/golden/make_golden_relight.py --floors     (the noise floors of tests/relight_ref64.py)
"""
from __future__ import annotations

import argparse
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_golden import CpuMode, load_reference  # noqa: E402

OUT = os.path.join(HERE, "relight.npz")
SETS = {"s24": (64, 24, 10), "s384": (8, 384, 11)}  # name -> (P, Ns, seed)
OUTPUTS = ["rgb", "incident_lights", "local_incident_lights", "global_incident_lights", "incident_visibility"]


class DirectLightEnv:
    def __init__(self, shs):
        self.get_env_shs = shs


def texture_linear_wrap(tex, uv, filter_mode="linear", boundary_mode="wrap"):
    """tex [1, H, W, C], uv [1, 1, N, 2] -> [1, 1, N, C] (see the module docstring)."""
    assert filter_mode == "linear" and boundary_mode == "wrap"
    H, W = tex.shape[1], tex.shape[2]

    def axis(u, n):
        u = u - torch.floor(u)
        x = u * n - 0.5
        x0 = torch.floor(x)
        i0 = x0.to(torch.int64)
        return i0 % n, (i0 + 1) % n, (x - x0)[..., None]

    x0, x1, fx = axis(uv[0, 0, :, 0], W)
    y0, y1, fy = axis(uv[0, 0, :, 1], H)
    m = tex[0]
    out = (m[y0, x0] * (1 - fx) * (1 - fy) + m[y0, x1] * fx * (1 - fy) + m[y1, x0] * (1 - fx) * fy +
           m[y1, x1] * fx * fy)
    return out[None, None]


def load_composite(ref: str):
    """neilf_composite and envmap modules of the reference, on the CPU."""
    load_reference(ref)
    m = types.ModuleType("scene.derect_light_sh")
    m.DirectLightEnv = DirectLightEnv
    sys.modules["scene.derect_light_sh"] = m
    sys.modules["cv2"] = types.ModuleType("cv2")
    nv = types.ModuleType("nvdiffrast")
    nvt = types.ModuleType("nvdiffrast.torch")
    nvt.texture = texture_linear_wrap
    nv.torch = nvt
    sys.modules["nvdiffrast"], sys.modules["nvdiffrast.torch"] = nv, nvt
    mods = []
    for name, rel in [("gaussian_renderer.neilf_composite", ("gaussian_renderer", "neilf_composite.py")),
                      ("r3dg_reference_envmap", ("scene", "envmap.py"))]:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, *rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def make_env_light(envmod, envmap: np.ndarray, transform):
    env = envmod.EnvLight.__new__(envmod.EnvLight)  # not its __init__: that reads an .hdr through cv2
    torch.nn.Module.__init__(env)
    env.to_opengl = torch.tensor([[1, 0, 0], [0, 0, 1], [0, -1, 0]], dtype=torch.float32)
    env.envmap = torch.from_numpy(envmap)
    env.transform = None if transform is None else torch.from_numpy(transform)
    return env


def relight_inputs(P: int, Ns: int, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(P, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
    v = rng.normal(size=(P, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return dict(base=f(rng.uniform(0, 1, (P, 3))), rough=f(rng.uniform(0.05, 1, (P, 1))),
                metal=f(rng.uniform(0, 1, (P, 1))), normals=f(n), viewdirs=f(v),
                incidents=f(rng.normal(0, 0.1, (P, 16, 3))), visibility=f(rng.normal(0, 0.1, (P, 25, 1))),
                env=f(rng.normal(0, 0.1, (1, 16, 3))), traced=f(rng.uniform(0, 1, (P, Ns, 1))))


def light_inputs() -> dict:
    rng = np.random.default_rng(12)
    envmap = np.exp(rng.normal(0, 1.5, (6, 10, 3)))  # HDR range: ~0.01 .. ~100
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    d = rng.normal(size=(256, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return dict(envmap=envmap.astype(np.float32), transform=np.ascontiguousarray(q, np.float32),
                lookup_dirs=d.astype(np.float32))


def generate(ref: str) -> dict:
    torch.set_num_threads(1)
    out = {}
    with CpuMode(), torch.no_grad():
        comp, envmod = load_composite(ref)
        li = light_inputs()
        out.update(li)
        env_map = make_env_light(envmod, li["envmap"], li["transform"])
        d = torch.from_numpy(li["lookup_dirs"])
        out["lookup_light"] = make_env_light(envmod, li["envmap"], None).direct_light(d).numpy()
        out["lookup_light_rot"] = env_map.direct_light(d).numpy()
        for name, (P, Ns, seed) in SETS.items():
            inp = relight_inputs(P, Ns, seed)
            t = {k: torch.from_numpy(v) for k, v in inp.items()}
            for k, v in inp.items():
                out[f"{name}_{k}"] = v
            out[f"{name}_sample_num"] = np.int32(Ns)
            cases = {"a": dict(light=DirectLightEnv(t["env"]), bake=True, pre=None),
                     "b": dict(light=env_map, bake=False, pre=t["traced"]),
                     "c": dict(light=None, bake=False, pre=t["traced"])}
            for c, kw in cases.items():
                rgb, extra = comp.rendering_equation_python(
                    t["base"], t["rough"], t["metal"], t["normals"], t["viewdirs"], t["incidents"], False, kw["light"],
                    t["visibility"], sample_num=Ns, bake=kw["bake"], visibility_precompute=kw["pre"])
                out[f"{name}_{c}_rgb"] = rgb.numpy()
                for k in OUTPUTS[1:]:
                    out[f"{name}_{c}_{k}"] = extra[k].numpy()
    return out


def write_npz(path: str, arrays: dict) -> None:
    """np.savez_compressed with fixed member timestamps, so that the bytes depend on the data only."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def case_args(g, name: str, c: str) -> dict:
    """The tests/relight_ref64.render arguments of golden case (name, c)."""
    from tests import relight_ref64 as r64

    inp = {k: g[f"{name}_{k}"] for k in ["base", "rough", "metal", "normals", "viewdirs", "incidents", "visibility",
                                         "env"]}
    kw = dict(inp=inp, Ns=int(g[f"{name}_sample_num"]))
    if c == "a":
        kw.update(light_mode=r64.LIGHT_SH)
    elif c == "b":
        kw.update(light_mode=r64.LIGHT_MAP, envmap=g["envmap"], transform=g["transform"], traced=g[f"{name}_traced"])
    else:
        kw.update(light_mode=r64.LIGHT_NONE, traced=g[f"{name}_traced"])
    return kw


def floors() -> None:
    from tests import relight_ref64 as r64

    g = np.load(OUT)
    worst = {k: 0.0 for k in OUTPUTS}
    for name in SETS:
        for c in "abc":
            ref = r64.render(**case_args(g, name, c))
            for k in OUTPUTS:
                e = r64.rel_err(g[f"{name}_{c}_{k}"], ref[k])
                print(f"{name} {c} {k:24s} {e:.3e}")
                worst[k] = max(worst[k], e)
    for k in OUTPUTS:
        print(f"floor {k:24s} {worst[k]:.3e}")
    e0 = r64.rel_err(g["lookup_light"], r64.envmap_direct_light(g["lookup_dirs"], g["envmap"]))
    e1 = r64.rel_err(g["lookup_light_rot"], r64.envmap_direct_light(g["lookup_dirs"], g["envmap"], g["transform"]))
    print(f"lookup {e0:.3e}  rotated {e1:.3e}\nfloor envmap {max(e0, e1):.3e}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--floors", action="store_true", help="print golden-vs-ref64 distances of the stored file")
    args = ap.parse_args()
    if args.floors:
        floors()
        return
    write_npz(OUT, generate(args.reference))
    print("written", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
