"""Every kernel instantiation of csrc/brdf.hip against the oracle and the float64 restatement, at every
sample count and SH width the render equation accepts (tests/_brdf_cases.py).

Which test launches which kernel (launch_fwd: a lane per sample for 1 <= sample_num <= 256, a thread per
Gaussian beyond; the <16, 16, 16> instantiations for 16 / 16 / 16 coefficients, <0, 0, 0> otherwise):

  brdf_fwd_lane_kernel<16,16,16, complex | training>  test_paths_match_oracle_and_restatement[Ns1 .. Ns256-S16_16_16]
  brdf_fwd_lane_kernel<0,0,0, complex | training>     test_paths_match_oracle_and_restatement[Ns24-S9_9_9 .. S1_1_1]
  brdf_fwd_kernel<16,16,16, complex | training>       test_paths_match_oracle_and_restatement[Ns257, Ns384],
                                                      test_thread_forward_prefetch[S16_16_16]
  brdf_fwd_kernel<0,0,0, complex | training>          test_thread_forward_prefetch[S9_4_1]
  brdf_bwd_kernel<16,16,16>, <0,0,0>                  test_paths_match_oracle_and_restatement, test_gaussian_counts
  brdf_dir_reduce_kernel                              every backward; its second trip: test_reducer_second_trip

Against the oracle: tests/_helpers.py assert_brdf, unchanged (1e-4 absolute; the summed environment
gradient 1e-4 of its scale). Against tests/brdf_ref64.py: the bars of tests/_brdf_cases.py, every element.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle
from relightable3dgaussian_amd import synthetic
from tests import _brdf_cases as bc
from tests import brdf_ref64 as r64
from tests._helpers import assert_brdf, tt

pytestmark = pytest.mark.gpu

CASE_IDS = [bc.case_id(c) for c in bc.CASES]
GRADS = ["base", "rough", "metal", "normals", "viewdirs", "incidents", "env", "visibility"]
PER_SAMPLE = ["incident_dirs", "incident_lights", "local_incident_lights", "global_incident_lights",
              "incident_visibility"]


def _dev(a):
    return tt(np.array(a, np.float32))  # a copy: the shared cases are read-only arrays


def _tensors(inp):
    return [_dev(inp[k]) for k in bc.INPUT_KEYS]


def gpu_complex(hip_ext, inp, ns):
    out = hip_ext.render_equation_forward_complex(*_tensors(inp), ns)
    return {k: v.cpu().numpy() for k, v in zip(r64.FORWARD_KEYS, out)}


def gpu_training(hip_ext, inp, ns, rand):
    out = hip_ext.render_equation_forward_with_rand(*_tensors(inp), ns, True, _dev(rand))
    return {k: v.cpu().numpy() for k, v in zip(bc.TRAIN_KEYS, out)}


def gpu_backward(hip_ext, inp, ns, dirs, gp, gd):
    out = hip_ext.render_equation_backward(*_tensors(inp), ns, _dev(dirs), _dev(gp), _dev(gd), False)
    return {k: v.cpu().numpy() for k, v in zip(GRADS, out)}


def against_oracle(tag, g, o):
    """The three calls' outputs, every one, against the oracle's at assert_brdf."""
    for k in r64.FORWARD_KEYS:
        assert_brdf(f"{tag} complex {k}", g["cx"][k], o["cx"][k])
    for k in bc.TRAIN_KEYS:
        assert_brdf(f"{tag} training {k}", g["tr"][k], o["tr"][k])
    for k in GRADS:
        assert_brdf(f"{tag} d_{k}", g["bw"][k], o["bw"][k], summed=k == "env")


@functools.lru_cache(maxsize=None)
def gpu_run(hip_ext, case, variant):
    """The GPU's three calls on one case, in oracle_run's layout (the backward on the oracle's directions,
    as the oracle's own). Read-only."""
    ns = case[0]
    inp = bc.inputs(case, variant)
    gp, gd = bc.upstream()
    return dict(cx=gpu_complex(hip_ext, inp, ns), tr=gpu_training(hip_ext, inp, ns, bc.randoms(ns)),
                bw=gpu_backward(hip_ext, inp, ns, bc.oracle_run(case, variant)["cx"]["incident_dirs"], gp, gd))


@pytest.mark.parametrize("variant", bc.VARIANTS)
@pytest.mark.parametrize("case", bc.CASES, ids=CASE_IDS)
def test_paths_match_oracle_and_restatement(hip_ext, case, variant):
    tag = f"{bc.case_id(case)} {variant}"
    g = gpu_run(hip_ext, case, variant)
    against_oracle(tag, g, bc.oracle_run(case, variant))
    for k in GRADS:
        assert np.isfinite(g["bw"][k]).all(), k
    bc.hold("gpu " + tag, bc.outputs_of(g), bc.outputs_of(bc.ref_run(case, variant)))


@pytest.mark.parametrize("variant", bc.VARIANTS)
@pytest.mark.parametrize("ns", [256, 257])
def test_lane_and_thread_forward_bit_identical_to_oracle(hip_ext, ns, variant):
    """sample_num = 256 is the lane kernel's last, 257 the thread-per-Gaussian kernel's first: no
    sample_num runs on both, so each one's per-sample outputs (and the training directions, rotated) must
    equal the oracle's bit for bit, as brdf.hip's header promises -- which makes them equal each other's
    arithmetic."""
    case = (ns, bc.S16)
    g, o = gpu_run(hip_ext, case, variant), bc.oracle_run(case, variant)
    differ = {k: int((g["cx"][k] != o["cx"][k]).sum()) for k in PER_SAMPLE}
    differ["training incident_dirs"] = int((g["tr"]["incident_dirs"] != o["tr"]["incident_dirs"]).sum())
    print(f"Ns {ns} {variant}: elements differing from the oracle {differ}")
    assert not any(differ.values()), differ


def _small(P, widths, seed):
    return bc.cut(synthetic.brdf_inputs(P, seed=seed), widths)


def _three_calls(hip_ext, inp, ns, seed):
    P = inp["base"].shape[0]
    rng = np.random.default_rng(seed)
    rand = rng.uniform(0, 1, (P, ns, 1)).astype(np.float32)
    gp, gd = rng.normal(size=(P, 3)).astype(np.float32), rng.normal(size=(P, 3)).astype(np.float32)
    o = dict(cx=oracle.brdf_forward_complex(inp, ns), tr=oracle.brdf_forward(inp, ns, True, rand))
    o["bw"] = oracle.brdf_backward(inp, o["cx"]["incident_dirs"], gp, gd, ns)
    g = dict(cx=gpu_complex(hip_ext, inp, ns), tr=gpu_training(hip_ext, inp, ns, rand),
             bw=gpu_backward(hip_ext, inp, ns, o["cx"]["incident_dirs"], gp, gd))
    return g, o


@pytest.mark.parametrize("widths", [bc.S16, (9, 4, 1)], ids=["S16_16_16", "S9_4_1"])
@pytest.mark.parametrize("ns,P", [(24, 1), (24, 255), (24, 256), (24, 257), (24, 41), (128, 3)])
def test_gaussian_counts(hip_ext, ns, P, widths):
    """Gaussian counts around the 256-thread block of the backward, and lane workgroups whose last one
    holds fewer Gaussians than GB = 256 / sample_num (24: GB = 10, P = 41, 255, 256, 257 leave 1, 5, 6, 7;
    128: GB = 2, P = 3 leaves 1; P = 1)."""
    g, o = _three_calls(hip_ext, _small(P, widths, seed=31 + P), ns, seed=P)
    against_oracle(f"P={P} Ns={ns}", g, o)


@pytest.mark.parametrize("widths", [bc.S16, (9, 4, 1)], ids=["S16_16_16", "S9_4_1"])
def test_reducer_second_trip(hip_ext, widths):
    """P = 65537 gives 257 block partials of the environment gradient: brdf_dir_reduce_kernel's strided
    loop takes its second trip (thread 0 only). Against the oracle's double-accumulated sum, and bit-equal
    run to run."""
    P = 65537
    inp = _small(P, widths, seed=41)
    rng = np.random.default_rng(42)
    gp, gd = rng.normal(size=(P, 3)).astype(np.float32), rng.normal(size=(P, 3)).astype(np.float32)
    dirs = oracle.brdf_forward(inp, 1)["incident_dirs"]
    o = oracle.brdf_backward(inp, dirs, gp, gd, 1)
    a = gpu_backward(hip_ext, inp, 1, dirs, gp, gd)
    b = gpu_backward(hip_ext, inp, 1, dirs, gp, gd)
    for k in GRADS:
        assert_brdf(f"P=65537 d_{k}", a[k], o[k], summed=k == "env")
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert np.abs(o["env"]).max() > 0


@pytest.mark.parametrize("widths", [bc.S16, (9, 4, 1)], ids=["S16_16_16", "S9_4_1"])
def test_thread_forward_prefetch(hip_ext, widths):
    """sample_num = 257: the thread-per-Gaussian forward, whose training branch reads rand_float one sample
    ahead. Explicit randoms as [P, Ns] and as [P, Ns, 1] give the same bits and match the oracle; the complex
    forward of the same inputs too (P = 300: a partial second block)."""
    P, ns = 300, 257
    inp = _small(P, widths, seed=51)
    rand = np.random.default_rng(52).uniform(0, 1, (P, ns)).astype(np.float32)
    o = oracle.brdf_forward(inp, ns, True, rand)
    flat = gpu_training(hip_ext, inp, ns, rand)
    col = gpu_training(hip_ext, inp, ns, rand.reshape(P, ns, 1))
    for k in bc.TRAIN_KEYS:
        assert_brdf(f"Ns=257 training {k}", flat[k], o[k])
        np.testing.assert_array_equal(flat[k], col[k], err_msg=k)
    assert int((flat["incident_dirs"] != o["incident_dirs"]).sum()) == 0
    ocx, gcx = oracle.brdf_forward_complex(inp, ns), gpu_complex(hip_ext, inp, ns)
    for k in r64.FORWARD_KEYS:
        assert_brdf(f"Ns=257 complex {k}", gcx[k], ocx[k])


def test_half_vector_floor(hip_ext):
    """View direction = minus sample 0's direction (taken from the oracle's forward) on every third
    Gaussian: h = d_0 + v is exactly zero there, half = 0 / 1e-7. In float64 the same inputs give another
    rounding residue, so this is held to the oracle only; every output stays finite."""
    case = (24, bc.S16)
    inp = dict(bc.inputs(case, "plain"))
    v = inp["viewdirs"].copy()
    v[::3] = -bc.oracle_run(case, "plain")["cx"]["incident_dirs"][::3, 0]
    inp["viewdirs"] = v
    g, o = _three_calls(hip_ext, inp, 24, seed=61)
    against_oracle("v = -d_0", g, o)
    for part in g.values():
        for k, a in part.items():
            assert np.isfinite(a).all(), k


@pytest.mark.parametrize("widths", [bc.S16, (9, 4, 1)], ids=["S16_16_16", "S9_4_1"])
@pytest.mark.parametrize("P,ns", [(301, 0), (0, 24), (0, 0)])
def test_no_samples_or_no_gaussians(hip_ext, P, ns, widths):
    """sample_num = 0 and P = 0: output shapes as usual, sums and gradients zero, no launch error."""
    import torch

    si, sd, sv = widths
    inp = _small(max(P, 1), widths, seed=71)
    inp = {k: (v if k == "env" else np.ascontiguousarray(v[:P])) for k, v in inp.items()}
    cx = gpu_complex(hip_ext, inp, ns)
    tr = gpu_training(hip_ext, inp, ns, np.zeros((P, ns, 1), np.float32))
    bw = gpu_backward(hip_ext, inp, ns, np.zeros((P, ns, 3), np.float32), np.ones((P, 3), np.float32),
                      np.ones((P, 3), np.float32))
    torch.cuda.synchronize()
    shapes = dict(pbr=(P, 3), incident_dirs=(P, ns, 3), incident_lights=(P, ns, 3), local_incident_lights=(P, ns, 3),
                  global_incident_lights=(P, ns, 3), incident_visibility=(P, ns, 1), diffuse_light=(P, 3),
                  local_diffuse_light=(P, 3), accum=(P, 1), rgb_d=(P, 3), rgb_s=(P, 3))
    for k, s in shapes.items():
        assert cx[k].shape == s, (k, cx[k].shape)
        assert not cx[k].any(), k
    for k in bc.TRAIN_KEYS:
        assert tr[k].shape == shapes[k] and not tr[k].any(), k
    gshapes = dict(base=(P, 3), rough=(P, 1), metal=(P, 1), normals=(P, 3), viewdirs=(P, 3), incidents=(P, si, 3),
                   env=(1, sd, 3), visibility=(P, sv, 1))
    for k, s in gshapes.items():
        assert bw[k].shape == s, (k, bw[k].shape)
        assert not bw[k].any(), k
