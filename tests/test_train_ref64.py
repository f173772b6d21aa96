"""The float64 Adam of tests/train_ref64.py pinned to torch.optim.Adam itself, the bounds an fp32
Adam is held to established on the oracle, and oracle/train_oracle.densify_and_prune held to the
reference's own GaussianModel on the edge fixture tests/golden/train_edges.npz (CPU only)."""
from __future__ import annotations

import os

import numpy as np
import pytest

from tests import _train_cases as tc
from tests import train_ref64 as r64

EDGES = os.path.join(os.path.dirname(__file__), "golden", "train_edges.npz")


def test_adam64_matches_torch_adam_float64():
    """Three steps with fresh gradients on float64 parameters, one learning rate per group, group 1
    with grad = None in step 2 (so its step count falls behind): param, exp_avg and exp_avg_sq agree
    with torch.optim.Adam(foreach=False, eps=1e-15) to rtol 1e-12 after every step."""
    import torch

    rng = np.random.default_rng(0)
    shapes = [(5, 3), (7,), (4, 1, 3), (1,)]
    lrs = [1e-3, 2.5e-2, 1.6e-4, 5e-2]
    params = [torch.nn.Parameter(torch.from_numpy(rng.normal(size=s))) for s in shapes]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(params, lrs)], lr=0.0, eps=1e-15,
                           foreach=False)
    p = [x.detach().numpy().copy() for x in params]
    m = [np.zeros(s) for s in shapes]
    v = [np.zeros(s) for s in shapes]
    steps = [0] * len(shapes)
    for k in range(3):
        for i, s in enumerate(shapes):
            g = rng.normal(size=s) * 10.0 ** rng.uniform(-4, -1)
            g.reshape(-1)[::3] = 0.0
            if k == 1 and i == 1:
                params[i].grad = None
                p[i], m[i], v[i] = r64.adam64(p[i], g, m[i], v[i], lrs[i], 0)
                continue
            params[i].grad = torch.from_numpy(g.copy())
            steps[i] += 1
            # a per-element step count, as the flat buffer's groups have
            p[i], m[i], v[i] = r64.adam64(p[i], g, m[i], v[i], np.full(s, lrs[i]), np.full(s, steps[i]), eps=1e-15)
        opt.step()
        for i in range(len(shapes)):
            st = opt.state[params[i]]
            assert int(st["step"]) == steps[i]
            np.testing.assert_allclose(p[i], params[i].detach().numpy(), rtol=1e-12, atol=0, err_msg=f"p {i} step {k}")
            np.testing.assert_allclose(m[i], st["exp_avg"].numpy(), rtol=1e-12, atol=0, err_msg=f"m {i} step {k}")
            np.testing.assert_allclose(v[i], st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0, err_msg=f"v {i} step {k}")
    assert steps == [3, 2, 3, 3]


def test_adam64_leaves_skipped_elements_untouched():
    rng = np.random.default_rng(1)
    p, g, m, v = (rng.normal(size=9) for _ in range(4))
    v = v * v
    step = np.array([0, 1, -1, 2, 0, 3, 1, 0, 5])
    p1, m1, v1 = r64.adam64(p, g, m, v, 1e-2, step)
    skip = step <= 0
    for a, b in ((p1, p), (m1, m), (v1, v)):
        assert np.array_equal(a[skip], b[skip]) and not np.any(a[~skip] == b[~skip])


@pytest.mark.parametrize("skip", [(), (8,), (9, 10)], ids=["all", "skip-roughness", "skip-metallic-incidents_dc"])
@pytest.mark.parametrize("P", tc.ADAM_P)
def test_oracle_adam_within_bounds(P, skip):
    """The fp32 oracle alone stays inside the bounds of tests/train_ref64.py against the float64
    reference, on the inputs the GPU tests use: this is what makes them the bounds of an fp32 Adam
    and not of one kernel. Prints the worst ratios (recorded in tests/train_ref64.py)."""
    c = tc.adam_case(P)
    p, m, v = c.p0, c.m0, c.v0
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for k in range(3):
        steps = tc.steps_at(c, k, skip)
        p1, m1, v1 = tc.oracle_adam(c, p, c.grads[k], m, v, steps)
        r = r64.assert_adam_bounds(f"oracle P={P} step {k}", p1, m1, v1, p, c.grads[k], m, v,
                                   tc.per_elem(c, c.lrs), tc.per_elem(c, steps))
        worst = {q: max(worst[q], r[q]) for q in worst}
        assert not np.array_equal(p1, p)
        p, m, v = p1, m1, v1
    print(f"oracle vs float64, P={P} skip={skip}: worst error / bound", worst)


def test_adam_case_boundaries_fall_at_every_residue():
    """The sizes are chosen so that group boundaries fall at every residue mod 4, and at P = 1 one
    float4 spans four groups."""
    res = set()
    for P in tc.ADAM_P:
        res |= {int(b) % 4 for b in tc.adam_case(P).bounds[1:-1]}
    assert res == {0, 1, 2, 3}
    b = tc.adam_case(1).bounds
    assert max(len({int(x) for x in tc.adam_case(1).gid[i:i + 4]}) for i in range(0, int(b[-1]) - 3, 4)) >= 4


# ---- oracle densify / prune vs the reference on the edge fixture --------------------------------

@pytest.fixture(scope="module")
def edges():
    return dict(np.load(EDGES))


def test_edges_fixture_is_unambiguous_and_has_every_class(edges):
    c = tc.edges_case(edges)
    mg, mo, ext, mss, mgn, pd = edges["densify_args"]
    assert (mg, mo, ext, mgn, pd) == tuple(tc.DENSIFY[k] for k in ("max_grad", "min_opacity", "extent",
                                                                  "max_grad_normal", "percent_dense"))
    tc.assert_unambiguous(c.model, c.xyz_accum, c.normal_accum, c.denom, c.max_radii, 2, float(mss))
    zero = c.denom == 0
    assert (zero & (c.xyz_accum == 0)).any() and (zero & (c.xyz_accum != 0)).any()
    # scenario b: split parents whose children exceed 0.1 * extent, clones whose original is pruned
    *_, counts_a = tc.oracle_densify(c, None)
    *_, counts_b = tc.oracle_densify(c, float(mss))
    assert counts_b[3] < counts_b[2] and counts_a[3] > counts_b[3], (counts_a, counts_b)
    sel = (c.xyz_accum / np.where(zero, 1, c.denom) >= mg) & ~zero
    small = np.exp(c.model["scaling"]).max(1) <= pd * ext
    low = 1 / (1 + np.exp(-c.model["opacity"][:, 0])) < mo
    assert (sel & small & low).any(), "no clone with a pruned original"
    assert int(edges["a_P"]) != int(edges["b_P"]) != int(edges["c_P"])


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_oracle_densify_edges_match_reference(edges, tag):
    """a: max_screen_size None (opacity prune only); b: max_screen_size 20 (children pruned by world
    size, clones with pruned originals); c: `prune` with max_radii2D, and the survivors' statistics."""
    c = tc.edges_case(edges)
    mss = float(edges["densify_args"][3])
    out, om, ov, src, counts = tc.oracle_densify(c, None if tag == "a" else mss, prune_only=tag == "c")
    assert out["xyz"].shape[0] == int(edges[f"{tag}_P"]) == len(src)
    tc.assert_densified(f"scenario {tag}", (out, om, ov), tc.edges_want(edges, tag), counts[0] + counts[1])
    if tag == "c":
        assert counts[1:] == [0, 0, 0] and (src >= 0).all()
        for k, a in (("xyz_accum", c.xyz_accum), ("normal_accum", c.normal_accum), ("denom", c.denom),
                     ("max_radii2D", c.max_radii)):
            np.testing.assert_array_equal(a[src], edges[f"c_{k}"], err_msg=k)
