"""The render equation's test cases, shared by tests/test_brdf_ref64.py (CPU: oracle against the float64
restatement) and tests/test_gpu_brdf_paths.py (GPU: every brdf.hip kernel against both).

A case is (sample_num, (S_incident, S_direct, S_visibility)) at P = 301 Gaussians, in two variants:

  plain  synthetic.brdf_inputs cut to the case's SH widths;
  edges  the same with every clamp of the formulas driven: roughness 0 and 1e-4 (the r^2 floor) on a
         stride, metallic exactly 0 and 1, normals (0, 0, -1) (the 1 + n_z floor), (0, 0, 1) and one a
         hair off -z (1 + n_z = 5e-7, above the floor), a view direction equal to the normal and one
         equal to minus the normal to one ulp (n.v <= 0, and at sample 0 -- the direction along the
         normal -- a half vector of length 6e-8: the |h| floor), visibility SH x 8 (both ends of the clamp),
         environment SH x 6 and incident SH with a negative constant term (both ReLUs).

Inputs chosen so that no element needs an exemption:
  * the two Gaussians with v = +-n get roughness 0.3 / 0.5: at sample 0 (the direction along the normal)
    v = n gives h.n = 1 to the last bit, and under the roughness floor the lobe exp(2e7 (h.n - 1)) turns
    that bit into a factor e, in float32 and float64 alike -- no reference has a value there.
  * v = -n is minus the oracle's own sample-0 direction with one component moved one ulp, so that
    h = d_0 + v is exactly one ulp long (6e-8: under the |h| floor, not zero) in float32 and float64
    alike. With v = -n exactly, h would be the float32 rounding residue of the direction: zero or an
    ulp or two, under the floor for one normal and over it for the next.
  * the shading is evaluated on the oracle's own directions, and the directions are compared on their
    own. The float32 angle r pi (3 - sqrt 5) is off by up to 4e-5 at r = 383, which a lobe of sharpness
    2 / 0.05^2 = 800 turns into percents of a sample's specular term (measured end to end: rgb_s 2.3e-4,
    training pbr 1.6e-3 of scale, bars under which the mutations of tests/test_brdf_ref64.py would pass),
    and the half vector of the v = -n Gaussian is a different residue on any other direction.
  * no unit normal strictly between the 1 + n_z floor and (0, 0, -1): the only float32 one is
    n_z = -1 + 2^-24, where the floored "rotation" scales x and z by -0.19 and so multiplies the float32
    angle error by 5 (measured 1.8e-4 on the directions instead of 4e-5): it would loosen the direction
    bar of every case until pi = numpy.pi passes it.

Bars: |got - ref| <= 1e-3 |ref| + FRAC[output] max|ref| over every element. FRAC is 4 x the largest
max|oracle - ref64| / max|ref64| measured over all cases and both variants (DESIGN.md section 5 has
the table; `python -m tests._brdf_cases` prints the measurement).
"""
from __future__ import annotations

import functools

import numpy as np

import oracle
from relightable3dgaussian_amd import synthetic
from tests import brdf_ref64 as r64

P = 301
S16 = (16, 16, 16)
CASES = [(ns, S16) for ns in (1, 2, 24, 100, 128, 129, 256, 257, 384)] + \
        [(24, w) for w in ((9, 9, 9), (16, 16, 9), (16, 4, 9), (9, 4, 1), (4, 16, 9), (1, 1, 1))]
VARIANTS = ["plain", "edges"]
REL = 1e-3
INPUT_KEYS = ["base", "rough", "metal", "normals", "viewdirs", "incidents", "env", "visibility"]
TRAIN_KEYS = ["pbr", "incident_dirs", "diffuse_light"]
# Gaussians of the edges variant with a fixed role
G_NEG_Z, G_POS_Z, G_NEAR_NEG_Z, G_V_IS_MINUS_N, G_V_IS_N = 10, 11, 12, 20, 21

# 4 x the measured oracle-vs-float64 distance (module docstring)
FRAC = {
    "pbr": 1.4e-4, "incident_dirs": 1.7e-4, "incident_lights": 1.6e-6, "local_incident_lights": 1.0e-6,
    "global_incident_lights": 1.7e-6, "incident_visibility": 2.3e-6, "diffuse_light": 4.4e-6,
    "local_diffuse_light": 2.3e-6, "accum": 1.2e-4, "rgb_d": 2.5e-6, "rgb_s": 1.9e-4,
    "train_pbr": 1.4e-4, "train_incident_dirs": 2.8e-4, "train_diffuse_light": 4.0e-6,
    "grad_base": 1.4e-4, "grad_rough": 2.1e-3, "grad_metal": 1.5e-4, "grad_incidents": 1.2e-4,
    "grad_env": 2.0e-5, "grad_visibility": 1.2e-4,
}


def case_id(case):
    ns, w = case
    return f"Ns{ns}-S{w[0]}_{w[1]}_{w[2]}"


def cut(inp, widths):
    si, sd, sv = widths
    out = {k: np.ascontiguousarray(v, np.float32) for k, v in inp.items()}
    out["incidents"] = np.ascontiguousarray(out["incidents"][:, :si])
    out["env"] = np.ascontiguousarray(out["env"][:, :sd])
    out["visibility"] = np.ascontiguousarray(out["visibility"][:, :sv])
    return out


def edges(inp):
    """The edges variant of 16-wide inputs (module docstring)."""
    e = {k: v.copy() for k, v in inp.items()}
    n = e["base"].shape[0]
    assert n > G_V_IS_N
    e["rough"][0::7] = 0.0
    e["rough"][3::7] = 1e-4
    e["metal"][0::5] = 0.0
    e["metal"][2::5] = 1.0
    e["normals"][G_NEG_Z] = (0.0, 0.0, -1.0)
    e["normals"][G_POS_Z] = (0.0, 0.0, 1.0)
    hair = np.array([1e-3, 0.0, -1.0])
    e["normals"][G_NEAR_NEG_Z] = (hair / np.linalg.norm(hair)).astype(np.float32)
    # v = -n to one ulp: minus the oracle's sample-0 direction (the normal, to float32 rounding) with its
    # largest component moved one ulp towards zero, so that h = d_0 + v is exactly one ulp (6e-8) long:
    # under the |h| floor, not zero, and the same in float32 and float64
    one = {k: np.ascontiguousarray(e[k][G_V_IS_MINUS_N:G_V_IS_MINUS_N + 1]) for k in INPUT_KEYS if k != "env"}
    d0 = oracle.brdf_forward_complex(dict(one, env=e["env"]), 1)["incident_dirs"][0, 0]
    v = -d0
    j = int(np.abs(v).argmax())
    v[j] = np.nextafter(v[j], np.float32(0.0))
    e["viewdirs"][G_V_IS_MINUS_N] = v
    e["viewdirs"][G_V_IS_N] = e["normals"][G_V_IS_N]
    e["rough"][G_V_IS_MINUS_N] = 0.5
    e["rough"][G_V_IS_N] = 0.3
    e["visibility"] *= 8.0
    e["env"] *= 6.0
    e["incidents"][0::2, 0, :] -= 0.6
    return e


@functools.lru_cache(maxsize=None)
def inputs(case, variant, n=P):
    """Read-only inputs of one case; n: another Gaussian count on the same recipe."""
    ns, widths = case
    full = synthetic.brdf_inputs(n, seed=100 + CASES.index(case) if case in CASES else 99)
    if variant == "edges":
        full = edges(full)
    inp = cut(full, widths)
    for v in inp.values():
        v.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def upstream(n=P, seed=6):
    rng = np.random.default_rng(seed)
    gp, gd = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
    gp.setflags(write=False)
    gd.setflags(write=False)
    return gp, gd


@functools.lru_cache(maxsize=None)
def randoms(ns, n=P, seed=9):
    r = np.random.default_rng(seed).uniform(0, 1, (n, ns, 1)).astype(np.float32)
    r.setflags(write=False)
    return r


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def oracle_run(case, variant):
    """The oracle's complex forward ("cx"), training forward with explicit randoms ("tr") and backward on
    the complex forward's directions ("bw"). Read-only."""
    ns = case[0]
    inp = inputs(case, variant)
    cx = oracle.brdf_forward_complex(inp, ns)
    tr = oracle.brdf_forward(inp, ns, True, randoms(ns))
    gp, gd = upstream()
    bw = oracle.brdf_backward(inp, cx["incident_dirs"], gp, gd, ns)
    return dict(cx=_freeze(cx), tr=_freeze(tr), bw=_freeze(bw))


def restate(case, variant, **mutation):
    """The restatement of the same three calls: the directions from its own float64 Fibonacci spiral
    ("cx" / "tr" incident_dirs), everything else evaluated on the oracle's directions (module docstring;
    the backward receives them as an input anyway). mutation: brdf_ref64.render's switches."""
    ns = case[0]
    inp = inputs(case, variant)
    o = oracle_run(case, variant)
    pi = mutation.get("pi", r64.PI)
    bw = r64.render(inp, ns, dirs=o["cx"]["incident_dirs"], upstream=upstream(), **mutation)
    cx = dict(bw, incident_dirs=r64.fibonacci_dirs(inp["normals"], ns, pi=pi).numpy())
    tr = dict(r64.render(inp, ns, dirs=o["tr"]["incident_dirs"], **mutation),
              incident_dirs=r64.fibonacci_dirs(inp["normals"], ns, randoms(ns), pi=pi).numpy())
    return dict(cx=_freeze(cx), tr=_freeze(tr), bw=_freeze(bw))


@functools.lru_cache(maxsize=None)
def ref_run(case, variant):
    """restate() without a mutation, computed once. Read-only."""
    return restate(case, variant)


def outputs_of(run):
    """{FRAC key: array} of an oracle_run / ref_run style result (also of the GPU's, same layout)."""
    out = {k: run["cx"][k] for k in r64.FORWARD_KEYS}
    out.update({"train_" + k: run["tr"][k] for k in TRAIN_KEYS})
    out.update({"grad_" + k: run["bw"]["grad_" + k] if "grad_" + k in run["bw"] else run["bw"][k]
                for k in r64.GRAD_KEYS})
    return out


def distance(got, ref):
    """max |got - ref| / max |ref| (the measurement FRAC is set from)."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    m = float(np.abs(ref).max(initial=0.0))
    d = float(np.abs(got - ref).max(initial=0.0))
    return d / m if m > 0 else d


def excess(got, ref, frac):
    """The worst |got - ref| / (REL |ref| + frac max|ref|) over every element: <= 1 passes."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64).reshape(got.shape)
    if got.size == 0:
        return 0.0
    m = float(np.abs(ref).max())
    d = np.abs(got - ref)
    bar = REL * np.abs(ref) + frac * m
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bar > 0, d / bar, np.where(d > 0, np.inf, 0.0))
    return float(q.max())


def hold(tag, got, ref, keys=None):
    """Every output of `got` against the restatement at FRAC, all elements; prints each figure first."""
    worst = {}
    for k in keys or FRAC:
        worst[k] = excess(got[k], ref[k], FRAC[k])
        print(f"brdf ref64 {tag} {k}: max|d|/max|ref| {distance(got[k], ref[k]):.2e} (bar frac {FRAC[k]:.1e}), "
              f"worst |d| / bar {worst[k]:.2f}")
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, f"{tag}: outside the bar (worst |d| / bar): {bad}"


def measure():
    """max|oracle - ref64| / max|ref64| per output over all cases and variants, and where."""
    top = {}
    for case in CASES:
        for variant in VARIANTS:
            o, r = outputs_of(oracle_run(case, variant)), outputs_of(ref_run(case, variant))
            for k in FRAC:
                dist = distance(o[k], r[k])
                if dist >= top.get(k, (-1.0, ""))[0]:
                    top[k] = (dist, f"{case_id(case)} {variant}")
    return top


if __name__ == "__main__":
    for key, (dist, where) in measure().items():
        print(f"{key:26s} measured {dist:.2e} at {where:24s} x4 = {4 * dist:.2e}   FRAC {FRAC[key]:.1e}")
