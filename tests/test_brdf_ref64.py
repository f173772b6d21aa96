"""The oracle's render equation (oracle/r3dg_oracle.c) against the float64 restatement
(tests/brdf_ref64.py) at every sample count and SH width of tests/_brdf_cases.py, plain and with
every clamp driven. CPU only.

Bar: |oracle - ref64| <= 1e-3 |ref64| + FRAC[output] max|ref64| over every element of every output
(tests/_brdf_cases.py; no element or Gaussian is left out). FRAC is 4 x the measured distance; the
mutation tests below show that each bar still separates the reference's conventions from a plausible
wrong one. The gradients of the normals and view directions are not gradients of the forward
(tests/brdf_ref64.py) and are held to the oracle only (tests/test_gpu_brdf_paths.py).
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import _brdf_cases as bc
from tests import brdf_ref64 as r64

CASE_IDS = [bc.case_id(c) for c in bc.CASES]


@pytest.mark.parametrize("variant", bc.VARIANTS)
@pytest.mark.parametrize("case", bc.CASES, ids=CASE_IDS)
def test_oracle_matches_restatement(case, variant):
    o, r = bc.outputs_of(bc.oracle_run(case, variant)), bc.outputs_of(bc.ref_run(case, variant))
    for k in bc.FRAC:
        assert o[k].size == r[k].size and o[k].size > 0, k
    bc.hold(f"{bc.case_id(case)} {variant}", o, r)


def test_incident_gradient_stays_in_its_row():
    """S_incident < S_direct: the incident-SH gradient is that of the zero-padded 16-wide run cut to 4
    coefficients (the reference's loop bound S_direct would run into the next Gaussians' rows), and the
    other gradients do not change."""
    import oracle

    case = (24, (4, 16, 9))
    inp = bc.inputs(case, "plain")
    dirs = bc.oracle_run(case, "plain")["cx"]["incident_dirs"]
    gp, gd = bc.upstream()
    padded = dict(inp, incidents=np.concatenate([inp["incidents"], np.zeros((bc.P, 12, 3), np.float32)], 1))
    got, wide = bc.oracle_run(case, "plain")["bw"], oracle.brdf_backward(padded, dirs, gp, gd, 24)
    np.testing.assert_array_equal(got["incidents"], wide["incidents"][:, :4])
    for k in ["base", "rough", "metal", "normals", "viewdirs", "env", "visibility"]:
        np.testing.assert_array_equal(got[k], wide[k], err_msg=k)


@pytest.mark.parametrize("case", bc.CASES, ids=CASE_IDS)
def test_edges_cover_every_clamp(case):
    """From the float64 intermediates of the edges variant: each clamp is active for at least one
    (Gaussian, sample) and inactive for another. The three light clamps need a few SH coefficients to
    vary over the samples: asserted where every width is >= 4."""
    ns, widths = case
    r = bc.ref_run(case, "edges")["bw"]
    inp = bc.inputs(case, "edges")

    def both(name, active):
        active = np.asarray(active)
        print(f"{bc.case_id(case)} {name}: active for {int(active.sum())} of {active.size}")
        assert active.any() and not active.all(), name

    both("roughness floor", r["raw_r2"] < r64.EPS)
    assert (inp["rough"] == 0).any() and (inp["rough"] == np.float32(1e-4)).any()
    assert (inp["metal"] == 0).any() and (inp["metal"] == 1).any()
    both("1 + n_z floor", r["raw_cp1"] < r64.EPS)
    assert 0 < r["raw_cp1"][bc.G_NEAR_NEG_Z] - r64.EPS < 1e-6  # a hair off -z: just above the floor
    both("n.v <= 0", r["raw_ndo"] <= 0)
    assert r["raw_ndo"][bc.G_V_IS_MINUS_N] < -0.999 and r["raw_ndo"][bc.G_V_IS_N] > 0.999
    both("|h| floor", r["raw_half"] < r64.EPS)
    assert r["raw_half"][bc.G_V_IS_MINUS_N, 0] < r64.EPS
    assert not (r["raw_den_i"] < r64.EPS).any() and not (r["raw_den_o"] < r64.EPS).any()  # >= (1 + 0)^2 / 8
    if ns > 1:  # one sample: the direction is the normal, n.d = 1
        both("n.d <= 0", r["raw_ndi"] <= 0)  # the normal (0, 0, -1): the samples stay around +z
    if min(widths) >= 4 and ns >= 24:
        both("visibility clamped at 0", r["raw_vis"] < 0)
        both("visibility clamped at 1", r["raw_vis"] > 1)
        both("visibility unclamped", (r["raw_vis"] > 0) & (r["raw_vis"] < 1))
        both("incident light ReLU", r["raw_local"] < 0)
        both("environment light ReLU", r["raw_global"] < 0)


# ------------------------------------------------------------------------------------------------
# the bars can fail: one convention replaced by a plausible wrong one
# ------------------------------------------------------------------------------------------------
def _must_fail(tag, case, variant, keys, **mutation):
    """The oracle meets the bar of every output against the restatement (test_oracle_matches_restatement)
    and misses it against the mutated restatement on each of `keys`; prints by how much."""
    o = bc.outputs_of(bc.oracle_run(case, variant))
    r = bc.outputs_of(bc.ref_run(case, variant))
    m = bc.outputs_of(bc.restate(case, variant, **mutation))
    out = {}
    for k in keys:
        assert bc.excess(o[k], r[k], bc.FRAC[k]) <= 1.0, (tag, k)
        out[k] = bc.excess(o[k], m[k], bc.FRAC[k])
        print(f"mutation {tag} {bc.case_id(case)} {variant} {k}: worst |d| / bar {out[k]:.1f} "
              f"(the unmutated restatement: {bc.excess(o[k], r[k], bc.FRAC[k]):.2f})")
    assert min(out.values()) > 1.0, (tag, out)


def test_mutated_true_clamp_gradients_fail_bar():
    """Autograd's own gradient through the three light clamps (zero where a clamp is active)."""
    _must_fail("straight_through=False", (24, bc.S16), "edges", ["grad_incidents", "grad_env", "grad_visibility"],
               straight_through=False)


def test_mutated_incident_cap_fails_bar():
    """The true incident-SH gradient for coefficients 4..15 at S_direct = 4."""
    _must_fail("incident_cap=False", (24, (16, 4, 9)), "plain", ["grad_incidents"], incident_cap=False)


def test_mutated_dropped_sample_fails_bar():
    """One of 384 samples (the middle one) left out of the sums."""
    _must_fail("drop_sample=191", (384, bc.S16), "plain",
               ["diffuse_light", "local_diffuse_light", "rgb_d", "pbr", "train_diffuse_light", "grad_env"],
               drop_sample=191)


def test_mutated_pi_fails_bar():
    """pi = numpy.pi instead of the reference's 3.14159: 8.4e-7 relative, visible in the azimuth of the
    last of 384 samples (920 rad) and nowhere else at float32."""
    _must_fail("pi=np.pi", (384, bc.S16), "plain", ["incident_dirs", "train_incident_dirs"], pi=float(np.pi))


def test_mutated_half_floor_fails_bar():
    """A half-vector floor of 1e-12: v = -n at sample 0 leaves |h| = 6e-8, so h / max(|h|, floor) is a unit
    vector instead of 0.6 of one (the base-colour and metallic gradients do not see it: h.v < 0 there, so
    the Fresnel term is 1 whatever F0 is)."""
    _must_fail("half_floor=1e-12", (24, bc.S16), "edges", ["rgb_s", "pbr", "grad_rough"], half_floor=1e-12)
