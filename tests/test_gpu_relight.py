"""csrc/relight.hip on the GPU against tests/golden/relight.npz (the reference's own float32 results) and
against tests/relight_ref64.py (the float64 restatement) at the shapes the golden file does not hold.

Bar: max|hip - ref| / max|ref| <= relight_ref64.BARS[output] = 4 x the measured float32 noise floor,
for each of rgb and the four means, over every element (nothing is masked: every forward term is
continuous in its inputs). The copied columns (normal, base_color, roughness, metallic) are bit-equal to
the inputs. The lookup-only op is held to ENVMAP_BAR against the ref64 lookup.
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests import relight_ref64 as r64
from tests.test_relight_ref import edge_dirs, golden_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "relight.npz")


class ShLight:
    def __init__(self, shs):
        self.get_env_shs = shs


def inputs(P, Ns, widths=(16, 16, 25), seed=0):
    """Drawn like tests/golden/make_golden.py brdf_inputs (roughness in [0.05, 1]) with the three SH widths
    (incident, direct, visibility), a traced visibility in [0, 1] and an HDR-range value scale for maps."""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(P, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
    v = rng.normal(size=(P, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    si, sd, sv = widths
    return dict(base=f(rng.uniform(0, 1, (P, 3))), rough=f(rng.uniform(0.05, 1, (P, 1))),
                metal=f(rng.uniform(0, 1, (P, 1))), normals=f(n), viewdirs=f(v),
                incidents=f(rng.normal(0, 0.1, (P, si, 3))), visibility=f(rng.normal(0, 0.1, (P, sv, 1))),
                env=f(rng.normal(0, 0.1, (1, sd, 3))), traced=f(rng.uniform(0, 1, (P, Ns))))


def env_map(shape, seed=3):
    rng = np.random.default_rng(seed)
    return np.exp(rng.normal(0, 1.5, shape + (3,))).astype(np.float32)


def rotation(seed=4):
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return np.ascontiguousarray(q, np.float32)


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_hip(inp, Ns, mode, traced, envmap=None, transform=None, slc=slice(None)):
    """(rgb, extra_results, features) of relight.render_equation_relight for Gaussians inp[...][slc]."""
    from relightable3dgaussian_amd import relight

    if mode == r64.LIGHT_SH:
        light = ShLight(cuda(inp["env"]))
    elif mode == r64.LIGHT_MAP:
        light = relight.EnvLight(cuda(envmap))
        light.transform = cuda(transform)
    else:
        light = None
    t = {k: cuda(inp[k][slc]) for k in ["base", "rough", "metal", "normals", "viewdirs", "incidents", "visibility",
                                        "traced"]}
    return relight.render_equation_relight(t["base"], t["rough"], t["metal"], t["normals"], t["viewdirs"],
                                           t["incidents"], light, t["visibility"], Ns, bake=not traced,
                                           visibility_precompute=t["traced"] if traced else None)


def hold(what, feats, ref, inp, Ns):
    """Every element of the [P, 21] result against ref (a dict with OUTPUT_KEYS) and the inputs."""
    feats = feats.cpu().numpy()
    assert feats.shape == (inp["base"].shape[0], 21) and np.isfinite(feats).all(), what
    bars = r64.BARS
    worst = {}
    for k in r64.OUTPUT_KEYS:
        a, b = r64.FEATURE_COLUMNS[k]
        worst[k] = r64.rel_err(feats[:, a:b], ref[k])
    print(what, {k: f"{v:.2e}/{bars[k]:.1e}" for k, v in worst.items()})
    for k, nm in [("normal", "normals"), ("base_color", "base"), ("roughness", "rough"), ("metallic", "metal")]:
        a, b = r64.FEATURE_COLUMNS[k]
        np.testing.assert_array_equal(feats[:, a:b], inp[nm], err_msg=f"{what} {k}")
    for k in r64.OUTPUT_KEYS:
        assert worst[k] <= bars[k], (what, k, worst[k], bars[k])


def check(what, inp, Ns, mode, traced, envmap=None, transform=None):
    ref = r64.render(inp, Ns, mode, envmap=envmap, transform=transform, traced=inp["traced"] if traced else None)
    _, _, feats = run_hip(inp, Ns, mode, traced, envmap, transform)
    hold(what, feats, ref, inp, Ns)
    return feats


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("c", "abc")
@pytest.mark.parametrize("name", ["s24", "s384"])
def test_golden_cases(hip_ext, golden, name, c):
    """The reference's own float32 results and the float64 restatement of the same case."""
    kw = golden_case(golden, name, c)
    inp = dict(kw["inp"], traced=golden[f"{name}_traced"][..., 0])
    mode, Ns, traced = kw["light_mode"], kw["Ns"], c != "a"
    _, _, feats = run_hip(inp, Ns, mode, traced, kw.get("envmap"), kw.get("transform"))
    hold(f"{name} {c} vs golden", feats, {k: golden[f"{name}_{c}_{k}"] for k in r64.OUTPUT_KEYS}, inp, Ns)
    hold(f"{name} {c} vs ref64", feats, r64.render(**kw), inp, Ns)


MODES = {"baked+sh": (r64.LIGHT_SH, False), "traced+map": (r64.LIGHT_MAP, True), "traced+none": (r64.LIGHT_NONE, True),
         "baked+map": (r64.LIGHT_MAP, False), "baked+none": (r64.LIGHT_NONE, False), "traced+sh": (r64.LIGHT_SH, True)}

# P x Ns, sparsely: the last partial workgroup (257 Gaussians at 10, 36 or 256 per workgroup), a workgroup
# that holds one Gaussian (Ns = 256), lanes left over in a workgroup (Ns = 7, 24), the pass loop with a short
# last pass (257: one sample; 384: half a pass), and one sample. 257 x 256 runs in test_alone_equals_in_batch.
#
# The pairings are those on which the reference's own float32 result (its Python on the CPU, same draws)
# stays within half of each bar against ref64; last column: its worst distance / bar. A bar below the
# reference's own rounding tests nothing, and the floors come from 64 + 8 Gaussians: the reference itself
# is at 0.9 to 1.6 x the rgb bar at 257 x 256 (the lobe's 2 / r^2 times the late samples' angle rounding,
# over 257 draws of the roughness), and at 1.6 to 2.4 x the light bars at 10 x 256 under the 5 x 7 map (a
# late sample 3e-3 rad from a pole of the lookup). The kernel measured the same figures there to 2 digits.
SHAPES = [(1, 1, "baked+sh"),        # 0.05
          (1, 24, "traced+none"),    # 0.04
          (1, 384, "traced+map"),    # 0.15
          (10, 7, "traced+map"),     # 0.24
          (10, 256, "traced+sh"),    # 0.45
          (10, 257, "baked+sh"),     # 0.33
          (10, 384, "baked+none"),   # 0.29
          (257, 1, "traced+map"),    # 0.07
          (257, 7, "traced+none"),   # 0.19
          (257, 7, "traced+map"),    # 0.19
          (257, 24, "baked+sh"),     # 0.27
          (257, 24, "traced+map")]   # 0.33


@pytest.mark.parametrize("P,Ns,mode", SHAPES, ids=[f"P{p}-Ns{n}-{m}" for p, n, m in SHAPES])
def test_shapes(hip_ext, P, Ns, mode):
    light, traced = MODES[mode]
    inp = inputs(P, Ns, (16, 16, 25), seed=P * 1000 + Ns)
    check(f"P{P} Ns{Ns} {mode}", inp, Ns, light, traced, env_map((5, 7)) if light == r64.LIGHT_MAP else None,
          rotation() if light == r64.LIGHT_MAP else None)


# (incident, direct, visibility) from {0, 1, 4, 9, 16, 25}; (16, 16, 16) is the register fast path in
# every mode, (16, 25, 25) is it where neither the SH light nor the baked visibility is read
WIDTHS = [(16, 16, 16), (25, 25, 25), (0, 0, 0), (0, 1, 4), (9, 0, 25), (1, 25, 0), (4, 9, 16), (25, 16, 9),
          (16, 25, 25), (16, 16, 9)]


@pytest.mark.parametrize("mode", ["baked+sh", "traced+map", "traced+none", "baked+map", "traced+sh"])
@pytest.mark.parametrize("widths", WIDTHS, ids=["-".join(map(str, w)) for w in WIDTHS])
def test_widths(hip_ext, widths, mode):
    light, traced = MODES[mode]
    P, Ns = 37, 24
    inp = inputs(P, Ns, widths, seed=sum(w * 31 ** i for i, w in enumerate(widths)) + 7)
    check(f"widths {widths} {mode}", inp, Ns, light, traced, env_map((5, 7)) if light == r64.LIGHT_MAP else None)


@pytest.mark.parametrize("mode", ["baked+sh", "traced+map"])
def test_normal_minus_z(hip_ext, mode):
    """n = (0, 0, -1): 1 + n_z = 0, where the reference turns the samples by -I (utils/sh_utils.py:66-67)
    instead of dividing by the floored 1 + n_z."""
    light, traced = MODES[mode]
    P, Ns = 10, 24
    inp = inputs(P, Ns, seed=77)
    inp["normals"][0] = (0, 0, -1)
    inp["normals"][1] = (0, 0, 1)
    inp["viewdirs"][0] = np.float32([0.3, 0.2, -0.9]) / np.linalg.norm([0.3, 0.2, -0.9])
    feats = check(f"-z {mode}", inp, Ns, light, traced, env_map((5, 7)) if light == r64.LIGHT_MAP else None)
    assert float(feats[0, :3].abs().max()) > 1e-3  # lit: its samples face the view direction's side


@pytest.mark.parametrize("with_transform", [False, True], ids=["plain", "rotated"])
@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (5, 7)], ids=["1x1", "2x3", "5x7"])
def test_maps(hip_ext, shape, with_transform):
    tr = rotation(9) if with_transform else None
    envmap = env_map(shape, seed=shape[0] * 10 + shape[1])
    inp = inputs(10, 24, seed=5)
    check(f"map {shape} rotated={with_transform}", inp, 24, r64.LIGHT_MAP, True, envmap, tr)
    # and the lookup alone, on random directions and the edge ones
    from relightable3dgaussian_amd import relight

    rng = np.random.default_rng(8)
    d = rng.normal(size=(500, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.concatenate([d, edge_dirs()]).astype(np.float32)
    got = relight.EnvLight(cuda(envmap)).direct_light(cuda(d), cuda(tr)).cpu().numpy()
    e = r64.rel_err(got, r64.envmap_direct_light(d, envmap, tr))
    print(f"lookup {shape} rotated={with_transform}: {e:.2e}/{r64.ENVMAP_BAR:.1e}")
    assert e <= r64.ENVMAP_BAR


def test_lookup_golden(hip_ext, golden):
    from relightable3dgaussian_amd import relight

    env = relight.EnvLight(cuda(golden["envmap"]))
    d = cuda(golden["lookup_dirs"])
    for key, tr in [("lookup_light", None), ("lookup_light_rot", golden["transform"])]:
        got = env.direct_light(d, cuda(tr)).cpu().numpy()
        e = r64.rel_err(got, golden[key])
        print(key, f"{e:.2e}/{r64.ENVMAP_BAR:.1e}")
        assert e <= r64.ENVMAP_BAR


def test_direct_light_leading_shape_scale_and_transform(hip_ext):
    """EnvLight.direct_light on a [4, 5, 3] tensor holding the seam, pole and axis directions; `scale`
    multiplies the map; `.transform` is used when no transform is passed."""
    from relightable3dgaussian_amd import relight

    envmap = env_map((5, 7), seed=21)
    d = edge_dirs().astype(np.float32).reshape(4, 5, 3)
    env = relight.EnvLight(cuda(envmap), scale=2.0)
    got = env.direct_light(cuda(d))
    assert got.shape == (4, 5, 3)
    ref = r64.envmap_direct_light(d, 2.0 * envmap.astype(np.float64))
    e = r64.rel_err(got.cpu().numpy(), ref)
    print(f"[4, 5, 3] edge directions: {e:.2e}/{r64.ENVMAP_BAR:.1e}")
    assert e <= r64.ENVMAP_BAR
    tr = rotation(2)
    env.transform = cuda(tr)
    assert torch.equal(env.direct_light(cuda(d)), env.direct_light(cuda(d), cuda(tr)))
    assert r64.rel_err(env.direct_light(cuda(d)).cpu().numpy(),
                       r64.envmap_direct_light(d, 2.0 * envmap.astype(np.float64), tr)) <= r64.ENVMAP_BAR
    assert env.direct_light(torch.empty(0, 3, device="cuda")).shape == (0, 3)


def test_features_layout_and_aliasing(hip_ext):
    """features columns are the concatenation of neilf_composite.py:129-133, and rgb and the extra_results
    entries are views into the features buffer."""
    inp = inputs(10, 24, seed=11)
    rgb, extra, feats = run_hip(inp, 24, r64.LIGHT_SH, False)
    assert feats.shape == (10, 21) and feats.is_contiguous() and feats.dtype == torch.float32
    cat = torch.cat([rgb, cuda(inp["normals"]), cuda(inp["base"]), cuda(inp["rough"]), cuda(inp["metal"]),
                     extra["incident_lights"], extra["local_incident_lights"], extra["global_incident_lights"],
                     extra["incident_visibility"]], dim=-1)
    assert torch.equal(cat, feats)
    assert list(extra) == ["incident_lights", "local_incident_lights", "global_incident_lights",
                           "incident_visibility"]
    for t, col in [(rgb, 0), (extra["incident_lights"], 11), (extra["local_incident_lights"], 14),
                   (extra["global_incident_lights"], 17), (extra["incident_visibility"], 20)]:
        assert t.data_ptr() == feats.data_ptr() + 4 * col and t.stride(0) == 21
    assert rgb.shape == (10, 3) and extra["incident_visibility"].shape == (10, 1)
    # P = 0 returns at once
    z = {k: (v if k == "env" else v[:0]) for k, v in inp.items()}
    assert run_hip(z, 24, r64.LIGHT_SH, False)[2].shape == (0, 21)
    assert run_hip(z, 24, r64.LIGHT_NONE, True)[2].shape == (0, 21)
    # [P, Ns, 1] traced visibility is the [P, Ns] one
    from relightable3dgaussian_amd import relight

    t = {k: cuda(v) for k, v in inp.items()}
    args = (t["base"], t["rough"], t["metal"], t["normals"], t["viewdirs"], t["incidents"], None, t["visibility"], 24)
    a = relight.render_equation_relight(*args, bake=False, visibility_precompute=t["traced"])[2]
    b = relight.render_equation_relight(*args, bake=False, visibility_precompute=t["traced"][..., None])[2]
    assert torch.equal(a, b)


def test_binding_refuses_bad_shapes(hip_ext):
    inp = inputs(4, 24, seed=1)
    t = {k: cuda(v) for k, v in inp.items()}
    C = hip_ext
    ok = [t["base"], t["rough"], t["metal"], t["normals"], t["viewdirs"], t["incidents"], t["env"], t["visibility"], 24, 1,
          None, None, None]
    assert C.render_equation_relight(*ok).shape == (4, 21)

    def bad(i, v):
        a = list(ok)
        a[i] = v
        with pytest.raises(RuntimeError):
            C.render_equation_relight(*a)

    bad(1, t["rough"][:3])                                   # P mismatch
    bad(5, torch.zeros(4, 26, 3, device="cuda"))             # 26 coefficients
    bad(5, t["incidents"].double())                          # not float32
    bad(3, t["normals"].cpu())                               # not on the GPU
    bad(6, None)                                             # SH light without direct_shs
    bad(7, None)                                             # neither baked nor traced visibility
    bad(9, 2)                                                # map light without a map
    bad(8, 0)                                                # sample_num 0
    bad(12, t["traced"][:, :5])                              # traced visibility of another Ns
    with pytest.raises(RuntimeError):
        C.envmap_direct_light(torch.zeros(5, 2, device="cuda"), torch.ones(2, 2, 3, device="cuda"), None)
    with pytest.raises(RuntimeError):
        C.envmap_direct_light(torch.zeros(5, 3, device="cuda"), torch.ones(2, 2, 4, device="cuda"), None)


@pytest.mark.parametrize("Ns,mode", [(24, "baked+sh"), (24, "traced+map"), (7, "traced+none"), (384, "traced+map"),
                                     (256, "baked+sh")])
def test_alone_equals_in_batch(hip_ext, Ns, mode):
    """A Gaussian's row is bitwise the same whether it runs alone or inside a batch of 257: wherever it
    sits in its workgroup, whoever its neighbours are."""
    light, traced = MODES[mode]
    inp = inputs(257, Ns, seed=123 + Ns)
    envmap = env_map((5, 7)) if light == r64.LIGHT_MAP else None
    batch = run_hip(inp, Ns, light, traced, envmap, rotation())[2]
    for g in [0, 1, 9, 10, 128, 255, 256]:
        alone = run_hip(inp, Ns, light, traced, envmap, rotation(), slc=slice(g, g + 1))[2]
        assert torch.equal(alone[0], batch[g]), (g, Ns, mode)
    again = run_hip(inp, Ns, light, traced, envmap, rotation())[2]
    assert torch.equal(again, batch)
