"""The training-step kernels of csrc/optim.hip at their shard, alignment and densify edges, through
the bindings themselves (`_C.adam_step`, `_C.adam_step_groups`, `_C.densification_stats`,
`_C.densify_and_prune`, `_C.reset_opacity`) and, where a case is about the trainer, through
GaussianTrainState.

Adam is held to the float64 restatement of torch.optim.Adam (tests/train_ref64.py) with the bounds
established there on the fp32 oracle; each step is checked from the fp32 state the kernel itself
held before it. Densify / prune is held to the reference's own results (tests/golden/train_edges.npz)
and to oracle/train_oracle.py on synthetic models in which every class of Gaussian is present
(tests/_train_cases.py): counts, order, every copy, the zeroed Adam state of new rows and the source
map exactly, child xyz / scaling to the fp32 tolerance of tests/test_train.py. Every compared value
keeps 1e-3 from its threshold (asserted on the inputs), so every mask is unambiguous.

Every shape is a few thousand floats; buffers passed to the bindings hold exactly what the layout
says (the bindings do not check lengths)."""
from __future__ import annotations

import itertools
import os

import numpy as np
import pytest

from oracle import train_oracle as T
from tests import _train_cases as tc
from tests import train_ref64 as r64

pytestmark = pytest.mark.gpu

EDGES = os.path.join(os.path.dirname(__file__), "golden", "train_edges.npz")
ROLES14 = tc.roles_of(tc.LAYOUT14)
CANARY = np.float32(-777.25)
F = np.float32


def _dev():
    import torch

    return torch.device("cuda", 0)


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- Adam ---------------------------------------------------------------------------------------

def _launch_adam(_C, c, p_full, g, m, v, lo, hi, steps, offs=(0, 0, 0), uniform_step=None, pad=0):
    """One kernel launch over [lo, hi). p_full: the whole parameter buffer (numpy, >= c.total floats);
    g / m / v: numpy arrays of hi - lo floats, passed as the contiguous slices buf[off : off + n] of
    larger canary-filled buffers. Returns the new (p_full, m, v) and asserts that every canary and
    every parameter outside [lo, hi) is bit-identical afterwards."""
    import torch

    n = hi - lo
    assert 0 <= lo <= hi <= c.total <= p_full.size and g.size == m.size == v.size == n
    bufs, views = [], []
    for a, off in zip((g, m, v), offs):
        buf = torch.full((n + 8 + pad,), float(CANARY), device=_dev())
        view = buf[off:off + n]
        view.copy_(_t(a))
        assert view.is_contiguous() and view.numel() == n
        bufs.append(buf)
        views.append(view)
    p = _t(p_full)
    args = (c.P, c.widths, ROLES14, p, views[0], views[1], views[2], lo, hi, list(c.lrs), 0.9, 0.999, 1e-15)
    if uniform_step is not None:
        _C.adam_step(*args, uniform_step)
    else:
        _C.adam_step_groups(*args, list(steps))
    torch.cuda.synchronize()
    p1 = p.cpu().numpy()
    outside = np.ones(p_full.size, bool)
    outside[lo:hi] = False
    assert np.array_equal(_bits(p1)[outside], _bits(p_full)[outside]), "param outside [lo, hi) changed"
    for name, buf, off in zip(("grad", "exp_avg", "exp_avg_sq"), bufs, offs):
        b = buf.cpu().numpy()
        edge = np.ones(b.size, bool)
        edge[off:off + n] = False
        assert (_bits(b)[edge] == _bits(CANARY)).all(), f"{name}: canary around the slice changed"
    assert np.array_equal(_bits(views[0].cpu().numpy()), _bits(g)), "grad changed"
    return p1, views[1].cpu().numpy(), views[2].cpu().numpy()


def _check(c, what, new, old, g, steps, lo=0, hi=None):
    hi = c.total if hi is None else hi
    (p1, m1, v1), (p0, m0, v0) = new, old
    return r64.assert_adam_bounds(what, p1[lo:hi], m1, v1, p0[lo:hi], g, m0, v0, tc.per_elem(c, c.lrs, lo, hi),
                                  tc.per_elem(c, steps, lo, hi))


@pytest.mark.parametrize("P", tc.ADAM_P)
def test_adam_every_group_three_steps(hip_ext, P):
    """lo = 0, every group with its own learning rate and step count, three steps with fresh
    gradients: p, m and v of every group inside the bounds after every step. At these sizes the
    group boundaries fall inside float4s at every residue, and the last float4 is a scalar tail."""
    c = tc.adam_case(P)
    assert c.total % 4 != 0  # the i4 + 4 > n tail runs
    p, m, v = c.p0, c.m0, c.v0
    for k in range(3):
        steps = tc.steps_at(c, k)
        new = _launch_adam(hip_ext, c, p, c.grads[k], m, v, 0, c.total, steps)
        for gi, (a, b) in enumerate(zip(c.bounds[:-1], c.bounds[1:])):  # name the group that fails
            r64.assert_adam_bounds(f"P={P} step {k} group {tc.NAMES[gi]}", new[0][a:b], new[1][a:b], new[2][a:b],
                                   p[a:b], c.grads[k][a:b], m[a:b], v[a:b], c.lrs[gi], steps[gi])
        p, m, v = new


@pytest.mark.parametrize("P", tc.ADAM_P)
def test_adam_uniform_step_binding(hip_ext, P):
    """`_C.adam_step` (one step count for all groups), from a non-zero state."""
    c = tc.adam_case(P, seed=1)
    new = _launch_adam(hip_ext, c, c.p0, c.grads[0], c.m0, c.v0, 0, c.total, None, uniform_step=3)
    _check(c, f"P={P}", new, (c.p0, c.m0, c.v0), c.grads[0], [3] * len(c.widths))


def _shard_ranges(P, world):
    """[lo, hi) of every rank by the trainer's own shard_size / shard_range."""
    from relightable3dgaussian_amd import trainer

    out = []
    for rank in range(world):
        st = trainer.GaussianTrainState(groups=trainer.BASE_GROUPS + trainer.PBR_GROUPS, P=P, param=None, grad=None,
                                        exp_avg=None, exp_avg_sq=None, dist=trainer._Dist(world, rank))
        assert st.widths() == tc.WIDTHS
        out.append(st.shard_range() + (st.shard_size(),))
    return out


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("P", tc.ADAM_P)
def test_adam_shards_assemble_to_the_unsharded_step(hip_ext, P, world):
    """One launch per rank's shard [lo, hi) with shard-local grad / exp_avg / exp_avg_sq (param is
    indexed globally), three steps: the assembled p, m, v meet the bounds against the unsharded
    float64 reference. P = 1 at world 8 has a short and an empty last shard."""
    c = tc.adam_case(P, seed=2)
    ranges = _shard_ranges(P, world)
    cap = ranges[0][2] * world
    if (P, world) == (1, 8):
        assert any(hi == lo for lo, hi, _ in ranges) and any(0 < hi - lo < s for lo, hi, s in ranges)
    assert sorted(set(i for lo, hi, _ in ranges for i in range(lo, hi))) == list(range(c.total))
    p = np.zeros(cap, F)  # the trainer pads the parameter buffer to shard_size * world
    p[:c.total] = c.p0
    m, v = c.m0, c.v0
    for k in range(3):
        steps = tc.steps_at(c, k)
        p1, m1, v1 = p.copy(), m.copy(), v.copy()
        for lo, hi, _ in ranges:
            p1, m1[lo:hi], v1[lo:hi] = _launch_adam(hip_ext, c, p1, c.grads[k][lo:hi], m[lo:hi], v[lo:hi], lo, hi, steps)
        _check(c, f"P={P} world={world} step {k}", (p1, m1, v1), (p, m, v), c.grads[k], steps)
        assert not p1[c.total:].any()
        p, m, v = p1, m1, v1


# (P, lo, n): lo % 4 in {1, 2, 3}, n in {0, 1, 2, 3, 5, 4k + 1}. P = 3 has its group ends at
# 9 18 30 39 42 51 186 195 198 201 210 345 348 393
RANGES = [
    (3, 53, 5),     # inside one group (f_rest)
    (3, 61, 41),    # inside one group, 4k + 1
    (3, 37, 9),     # scaling, opacity, f_dc
    (3, 194, 13),   # base_color, roughness, metallic, incidents_dc
    (3, 183, 3),    # ends exactly on a group boundary
    (3, 7, 2),      # ends exactly on a group boundary
    (3, 41, 1),     # one float, the last of its group
    (3, 5, 0),      # hi == lo
    (37, 3801, 1029),  # 4k + 1 over 258 float4 threads: two blocks, three groups
    (1, 62, 5),     # P = 1: one float per narrow group
]


def _range_case(hip_ext, P, lo, n, offs, what):
    c = tc.adam_case(P, seed=3)
    hi = lo + n
    steps = tc.steps_at(c, 1)
    p = np.full(c.total + 8, CANARY, F)
    p[lo:hi] = c.p0[lo:hi]
    old = (p, c.m0[lo:hi], c.v0[lo:hi])
    new = _launch_adam(hip_ext, c, p, c.grads[1][lo:hi], old[1], old[2], lo, hi, steps, offs=offs)
    if n:
        _check(c, what, new, old, c.grads[1][lo:hi], steps, lo, hi)
        assert not np.array_equal(new[0][lo:hi], p[lo:hi])


def test_adam_arbitrary_ranges_and_misaligned_pointers(hip_ext):
    """Ranges that start off a float4 boundary, with grad / exp_avg / exp_avg_sq each at its own
    offset 0..3 inside a larger buffer (the scalar fallback), a canary everywhere around them."""
    assert {lo % 4 for _, lo, _ in RANGES} == {1, 2, 3}
    trip = list(itertools.product(range(4), repeat=3))
    for i, (P, lo, n) in enumerate(RANGES):
        for j in range(4):
            offs = trip[(17 * i + 5 * j + 1) % 64]
            _range_case(hip_ext, P, lo, n, offs, f"P={P} [{lo}, {lo + n}) offs={offs}")
    for offs in trip:  # every combination of the three offsets, on the range across four groups
        _range_case(hip_ext, 3, 194, 13, offs, f"[194, 207) offs={offs}")


@pytest.mark.parametrize("offs", [(0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 3)], ids=lambda o: "offs%d%d%d" % o)
def test_adam_aligned_range_each_pointer_misaligned_alone(hip_ext, offs):
    """lo % 4 == 0, so only the named pointer decides between the float4 path and the fallback;
    n = 4k + 1 leaves a scalar tail on the float4 path."""
    P, lo, n = 3, 52, 141  # f_rest into base_color
    c = tc.adam_case(P, seed=4)
    steps = tc.steps_at(c, 2)
    p = np.full(c.total, CANARY, F)
    p[lo:lo + n] = c.p0[lo:lo + n]
    old = (p, c.m0[lo:lo + n], c.v0[lo:lo + n])
    new = _launch_adam(hip_ext, c, p, c.grads[2][lo:lo + n], old[1], old[2], lo, lo + n, steps, offs=offs)
    _check(c, f"offs={offs}", new, old, c.grads[2][lo:lo + n], steps, lo, lo + n)


@pytest.mark.parametrize("offs", [(0, 0, 0), (1, 0, 0)], ids=["float4", "misaligned"])
@pytest.mark.parametrize("skip", [(8,), (9, 10)], ids=["roughness", "metallic-incidents_dc"])
def test_adam_skip_bits_inside_one_float4(hip_ext, skip, offs):
    """P = 1: floats 64..67 are base_color[2], roughness, metallic, incidents_dc[0], one float4 with
    mixed skip bits. Skipped elements keep p, m and v bit for bit; the others step within bounds."""
    c = tc.adam_case(1, seed=5)
    assert [int(x) for x in c.gid[64:68]] == [7, 8, 9, 10]
    g = c.grads[0].copy()
    sk = np.isin(c.gid, skip)
    g[sk] = 0.0123  # a skipped element that stepped anyway would move
    p, m, v = c.p0, np.where(sk, F(0.004), c.m0).astype(F), np.where(sk, F(3e-5), c.v0).astype(F)
    for k in range(2):
        steps = tc.steps_at(c, k, skip)
        new = _launch_adam(hip_ext, c, p, g, m, v, 0, c.total, steps, offs=offs)
        _check(c, f"skip {skip} step {k}", new, (p, m, v), g, steps)
        assert not np.array_equal(new[0][~sk], p[~sk])
        p, m, v = new


# ---- densification statistics -------------------------------------------------------------------

@pytest.mark.parametrize("with_normal", [True, False], ids=["normal", "no-normal"])
@pytest.mark.parametrize("stride", [2, 3, 4])
def test_densification_stats_strides_and_short_normals(hip_ext, stride, with_normal):
    """P = 257 (two blocks), dL_dmeans2D of row stride 2 / 3 / 4, radii with 0 and negatives, normal
    gradients of length 0, 5e-4 (under normalize's eps = 1e-3) and 1; two calls, so the sums
    accumulate and the max is taken against an earlier radius."""
    import torch

    P = 257
    rng = np.random.default_rng(stride)
    acc, nacc, den, mr = (rng.uniform(0.5, 2.0, size=P).astype(F) for _ in range(4))
    den, mr = np.floor(den * 3).astype(F), np.floor(mr * 8).astype(F)
    start = [x.copy() for x in (acc, nacc, den, mr)]
    dev = [_t(x) for x in (acc, nacc, den, mr)]
    never = np.ones(P, bool)
    for call in range(2):
        d2 = (rng.normal(size=(P, stride)) * 3e-4).astype(F)
        radii = rng.integers(-3, 31, size=P).astype(np.int32)
        radii[call::7] = 0
        radii[3::11] = -2
        never &= radii <= 0
        dirs = rng.normal(size=(P, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        ng = (dirs * np.asarray([0.0, 5e-4, 1.0])[(np.arange(P) + call) % 3][:, None]).astype(F)
        T.densification_stats(d2, ng if with_normal else None, radii, acc, nacc, den, mr)
        hip_ext.densification_stats(_t(d2), _t(ng) if with_normal else torch.empty(0, device=_dev()), _t(radii), *dev)
    got = [x.cpu().numpy() for x in dev]
    assert never.any() and not never.all()
    np.testing.assert_allclose(got[0], acc, rtol=1e-6, atol=0, err_msg="xyz_accum")
    np.testing.assert_allclose(got[1], nacc, rtol=1e-6, atol=0, err_msg="normal_accum")
    np.testing.assert_array_equal(got[2], den, err_msg="denom")
    np.testing.assert_array_equal(got[3], mr, err_msg="max_radii2D")
    for a, b in zip(got, start):
        assert np.array_equal(_bits(a)[never], _bits(b)[never]), "a row with radii <= 0 changed"
    if not with_normal:
        assert np.array_equal(_bits(got[1]), _bits(start[1]))
    else:
        assert not np.array_equal(got[1], start[1])


# ---- densify / prune ----------------------------------------------------------------------------

def _flat(d, layout):
    return np.concatenate([np.asarray(d[n], F).reshape(-1) for n, _ in layout]) if layout else np.zeros(0, F)


def _unflat(flat, layout, P):
    out, o = {}, 0
    for n, w in layout:
        out[n] = flat[o:o + P * w].reshape(P, w)
        o += P * w
    assert o == flat.size
    return out


def _gpu_densify(_C, c, max_screen_size, prune_only=False, noise=None, **d):
    """`_C.densify_and_prune` on a case; buffers hold exactly P * W and P floats."""
    import torch

    d = {**tc.DENSIFY, **d}
    W = sum(w for _, w in c.layout)
    flat, fm, fv = (_flat(x, c.layout) for x in (c.model, c.m, c.v))
    assert flat.size == fm.size == fv.size == c.P * W
    stats = [np.asarray(x, F).reshape(-1) for x in (c.xyz_accum, c.normal_accum, c.denom, c.max_radii)]
    assert all(x.size == c.P for x in stats)
    nz = torch.empty(0, device=_dev()) if noise is None else _t(np.asarray(noise, F))
    newp, newm, newv, src, Pn, counts = _C.densify_and_prune(
        c.P, [w for _, w in c.layout], tc.roles_of(c.layout), _t(flat), _t(fm), _t(fv), _t(stats[0]), _t(stats[1]),
        _t(stats[2]), _t(stats[3]) if prune_only else torch.empty(0, device=_dev()), d["max_grad"],
        d["max_grad_normal"], d["percent_dense"], d["extent"], d["min_opacity"], float(max_screen_size or 0.0), c.N,
        bool(prune_only), nz)
    torch.cuda.synchronize()
    assert newp.numel() == newm.numel() == newv.numel() == Pn * W and src.numel() == Pn
    got = tuple(_unflat(x.cpu().numpy(), c.layout, Pn) for x in (newp, newm, newv))
    return got, src.cpu().numpy(), int(Pn), [int(x) for x in counts]


def _against_oracle(_C, c, max_screen_size, prune_only=False, what=""):
    tc.assert_unambiguous(c.model, c.xyz_accum, c.normal_accum, c.denom, c.max_radii, c.N, max_screen_size or 0.0)
    out, om, ov, src, counts = tc.oracle_densify(c, max_screen_size, prune_only)
    got, gsrc, Pn, gcounts = _gpu_densify(_C, c, max_screen_size, prune_only, noise=c.noise)
    assert gcounts == counts and Pn == len(src) == counts[0] + counts[1] + c.N * counts[3], (what, gcounts, counts)
    tc.assert_densified(what, got, (out, om, ov), counts[0] + counts[1])
    np.testing.assert_array_equal(gsrc, src, err_msg=f"{what}: source map")
    new = src < 0
    for n in got[1]:  # new rows start with a zero Adam state (also covered by the exact compare)
        assert not got[1][n][new].any() and not got[2][n][new].any()
    return counts


@pytest.fixture(scope="module")
def edges():
    return dict(np.load(EDGES))


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_densify_edge_scenarios_match_reference(hip_ext, edges, tag):
    """The three scenarios of tests/golden/train_edges.npz against the reference's own results:
    a max_screen_size None, b max_screen_size 20 (children pruned by world size, clones with pruned
    originals, denom = 0 rows), c `prune` with max_radii2D and the survivors' statistics."""
    c = tc.edges_case(edges)
    mss = None if tag == "a" else float(edges["densify_args"][3])
    counts = _against_oracle(hip_ext, c, mss, prune_only=tag == "c", what=f"scenario {tag} vs oracle")
    got, src, Pn, _ = _gpu_densify(hip_ext, c, mss, prune_only=tag == "c", noise=c.noise)
    assert Pn == int(edges[f"{tag}_P"])
    tc.assert_densified(f"scenario {tag} vs reference", got, tc.edges_want(edges, tag), counts[0] + counts[1])
    if tag == "c":
        for k, a in (("xyz_accum", c.xyz_accum), ("normal_accum", c.normal_accum), ("denom", c.denom),
                     ("max_radii2D", c.max_radii)):
            np.testing.assert_array_equal(a[src], edges[f"c_{k}"], err_msg=k)


@pytest.mark.parametrize("mss", [None, 20.0], ids=["no-screen-size", "screen-size"])
@pytest.mark.parametrize("N", [1, 3])
def test_densify_n_children(hip_ext, N, mss):
    c = tc.densify_case(64, N=N)
    counts = _against_oracle(hip_ext, c, mss, what=f"N={N} mss={mss}")
    assert counts[1] > 0 and counts[2] > counts[3] > 0


def test_densify_two_blocks_all_classes(hip_ext):
    """P = 257: the classification, the scan and the scatter cross a 256-thread block."""
    c = tc.densify_case(257)
    assert set(c.cls) == set(tc.ALL_CLASSES)
    counts = _against_oracle(hip_ext, c, 20.0, what="P=257")
    assert counts[0] < 257 and counts[1] > 0 and counts[2] > counts[3] > 0
    _against_oracle(hip_ext, c, None, what="P=257 no screen size")


def test_densify_roles_out_of_order(hip_ext):
    """opacity(1), rotation(4), extra(5), scaling(3), xyz(3): the roles are looked up, not assumed."""
    c = tc.densify_case(70, layout=tc.LAYOUT5)
    assert tc.roles_of(c.layout) == [4, 3, 1, 0]
    counts = _against_oracle(hip_ext, c, 20.0, what="5 groups")
    assert counts[1] > 0 and counts[3] > 0
    _against_oracle(hip_ext, c, 20.0, prune_only=True, what="5 groups prune")


def test_densify_nothing_selected_nothing_pruned(hip_ext):
    c = tc.densify_case(70, classes=(tc.KEEP,))
    got, src, Pn, counts = _gpu_densify(hip_ext, c, 20.0, noise=c.noise)
    assert Pn == 70 and counts == [70, 0, 0, 0]
    np.testing.assert_array_equal(src, np.arange(70))
    for g, w in zip(got, (c.model, c.m, c.v)):
        for n in g:
            assert np.array_equal(_bits(g[n]), _bits(w[n])), n
    _against_oracle(hip_ext, c, 20.0, what="nothing happens")


def test_densify_prune_only_without_screen_size(hip_ext):
    """`prune` with max_screen_size = 0: the opacity test alone, whatever max_radii2D and the scales are."""
    c = tc.densify_case(257)
    counts = _against_oracle(hip_ext, c, 0.0, prune_only=True, what="prune, screen size 0")
    kept_screen = _against_oracle(hip_ext, c, 20.0, prune_only=True, what="prune, screen size 20")
    assert counts[1:] == [0, 0, 0] and 0 < kept_screen[0] < counts[0] < 257


def test_densify_empty_model_in(hip_ext):
    for layout in (tc.LAYOUT14, tc.LAYOUT5):
        c = tc.densify_case(0, layout=layout)
        for prune_only in (False, True):
            got, src, Pn, counts = _gpu_densify(hip_ext, c, 20.0, prune_only=prune_only, noise=c.noise)
            assert Pn == 0 and counts == [0, 0, 0, 0] and src.size == 0
            assert all(got[0][n].shape == (0, w) for n, w in layout)


def _state_of(c):
    """A GaussianTrainState holding a 14-group case, its Adam state and statistics."""
    import torch

    from relightable3dgaussian_amd import trainer

    shapes = dict(trainer.BASE_GROUPS + trainer.PBR_GROUPS)
    st = trainer.GaussianTrainState.from_tensors({n: _t(c.model[n]).reshape(c.P, *shapes[n]) for n in tc.NAMES})
    st.percent_dense = tc.DENSIFY["percent_dense"]
    st.lrs = [1e-3 * (g + 1) for g in range(len(tc.NAMES))]
    st.exp_avg[:st.total()] = _t(_flat(c.m, c.layout))
    st.exp_avg_sq[:st.total()] = _t(_flat(c.v, c.layout))
    st.xyz_gradient_accum = _t(c.xyz_accum).reshape(c.P, 1)
    st.normal_gradient_accum = _t(c.normal_accum).reshape(c.P, 1)
    st.denom = _t(c.denom).reshape(c.P, 1)
    st.max_radii2D = _t(c.max_radii)
    torch.cuda.synchronize()
    return st


def _snapshot(st):
    return [st.P] + [x.cpu().numpy().copy() for x in (st.param, st.exp_avg, st.exp_avg_sq, st.xyz_gradient_accum,
                                                      st.normal_gradient_accum, st.denom, st.max_radii2D)]


def test_densify_everything_pruned_then_the_state_still_works(hip_ext):
    """Every Gaussian under min_opacity: P_new == 0 with the originals, the clones and the children
    all pruned; an empty GaussianTrainState then still steps, takes statistics, densifies, prunes
    and resets without error."""
    import torch

    c = tc.densify_case(60, classes=(tc.LOW_OPACITY, tc.CLONE_PRUNED, tc.SPLIT_LOW_OPACITY))
    counts = _against_oracle(hip_ext, c, 20.0, what="everything pruned")
    assert counts == [0, 0, 20, 0]
    st = _state_of(c)
    d = tc.DENSIFY
    st.densify_and_prune(d["max_grad"], d["min_opacity"], d["extent"], 20.0, d["max_grad_normal"], noise=_t(c.noise))
    assert st.P == 0 and st.total() == 0 and st.denom.shape == (0, 1)
    for _ in range(2):
        st.step()
        st.add_densification_stats(torch.zeros(0, 3, device=_dev()), torch.zeros(0, dtype=torch.int32, device=_dev()),
                                   normal_grad=torch.zeros(0, 3, device=_dev()))
        assert st.densify_and_prune(d["max_grad"], d["min_opacity"], d["extent"], None, d["max_grad_normal"]) == [0] * 4
        assert st.prune(d["min_opacity"], d["extent"], 20.0) == [0] * 4
        st.reset_opacity()
        assert st.P == 0 and not st.param.any()
    torch.cuda.synchronize()


@pytest.mark.parametrize("seed", [3, 11])
def test_densify_production_noise_is_torch_randn(hip_ext, seed):
    """With no noise given the split noise is drawn by torch.randn on the device: after
    torch.manual_seed(s) the result equals the oracle run with torch.randn(3 N n_split) of the same
    seed."""
    import torch

    c = tc.densify_case(64, N=3, seed=seed)
    n_split = tc.oracle_densify(c, 20.0)[4][2]
    assert n_split > 0
    torch.manual_seed(seed)
    got, src, Pn, counts = _gpu_densify(hip_ext, c, 20.0, noise=None)
    torch.manual_seed(seed)
    noise = torch.randn(3 * c.N * n_split, device=_dev()).cpu().numpy()
    out, om, ov, wsrc, wcounts = tc.oracle_densify(c, 20.0, noise=noise)
    assert counts == wcounts and Pn == len(wsrc)
    tc.assert_densified("randn noise", got, (out, om, ov), counts[0] + counts[1])
    moved = got[0]["xyz"][counts[0] + counts[1]:] - np.tile(c.model["xyz"][np.nonzero(
        np.isin(c.cls, (tc.SPLIT, tc.INF_GRAD_SPLIT, tc.NORMAL_ONLY_SPLIT)))[0]], (c.N, 1))
    assert np.abs(moved).max() > 1e-3  # the children did receive noise


def test_densify_given_noise_too_short_raises_and_leaves_the_state(hip_ext):
    c = tc.densify_case(64)
    n_split = tc.oracle_densify(c, 20.0)[4][2]
    st = _state_of(c)
    before = _snapshot(st)
    d = tc.DENSIFY
    with pytest.raises(RuntimeError):
        st.densify_and_prune(d["max_grad"], d["min_opacity"], d["extent"], 20.0, d["max_grad_normal"],
                             noise=_t(c.noise[:3 * c.N * n_split - 1]))
    after = _snapshot(st)
    assert after[0] == before[0]
    for a, b in zip(after[1:], before[1:]):
        assert np.array_equal(_bits(a), _bits(b))
    # the same state with enough noise densifies as the oracle does
    st.densify_and_prune(d["max_grad"], d["min_opacity"], d["extent"], 20.0, d["max_grad_normal"],
                         noise=_t(c.noise[:3 * c.N * n_split]))
    out, _, _, src, _ = tc.oracle_densify(c, 20.0)
    assert st.P == len(src)
    np.testing.assert_array_equal(st.view("opacity").cpu().numpy(), out["opacity"])
    assert not st.denom.any() and st.denom.shape == (st.P, 1)


# ---- reset_opacity ------------------------------------------------------------------------------

def _reset_case(P=300):
    """Raw opacities over [-80, 30] with values on both sides of logit(0.01) = -4.5951, and what
    torch's own fp32 CPU expression makes of them (gaussian_model.py:688-691)."""
    import torch

    rng = np.random.default_rng(9)
    op = rng.uniform(-80.0, 30.0, size=P).astype(F)
    op[:8] = [-80.0, 30.0, -4.7, -4.6, -4.59, -4.5, 0.0, -20.0]
    x = torch.from_numpy(op)
    y = torch.min(torch.sigmoid(x), torch.ones_like(x) * 0.01)
    want = torch.log(y / (1 - y)).numpy()
    assert (want[op < -4.6] < -4.5952).all() and (want[op > -4.59] > -4.5952).all()
    return op, want


@pytest.mark.parametrize("with_state", [True, False], ids=["state", "empties"])
def test_reset_opacity_binding(hip_ext, with_state):
    """Only the opacity segment of param (and of exp_avg / exp_avg_sq when they are passed, where it
    becomes zero) may change."""
    import torch

    P = 300
    op, want = _reset_case(P)
    rng = np.random.default_rng(10)
    total = P * sum(tc.WIDTHS)
    a, b = P * sum(tc.WIDTHS[:4]), P * sum(tc.WIDTHS[:5])
    p, m, v = (rng.uniform(0.5, 1.5, size=total).astype(F) for _ in range(3))
    p[a:b] = op
    dp, dm, dv = _t(p), _t(m), _t(v)
    empty = torch.empty(0, device=_dev())
    hip_ext.reset_opacity(P, tc.WIDTHS, ROLES14, dp, dm if with_state else empty, dv if with_state else empty)
    torch.cuda.synchronize()
    gp, gm, gv = (x.cpu().numpy() for x in (dp, dm, dv))
    np.testing.assert_allclose(gp[a:b], want, rtol=1e-6, atol=0)
    seg = np.zeros(total, bool)
    seg[a:b] = True
    assert np.array_equal(_bits(gp)[~seg], _bits(p)[~seg])
    for g, w in ((gm, m), (gv, v)):
        assert np.array_equal(_bits(g)[~seg], _bits(w)[~seg])
        if with_state:
            assert not g[seg].any()
        else:
            assert np.array_equal(_bits(g)[seg], _bits(w)[seg])


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_reset_opacity_through_the_trainer_on_a_shard(hip_ext, rank):
    """World 10 at P = 37 puts the opacity segment [481, 518) across the shards of rank 0 ([0, 488))
    and rank 1 ([488, 976)); rank 2 holds none of it. Each rank zeroes exactly its part of the
    opacity state (the trainer's slice arithmetic) and resets every opacity."""
    import torch

    from relightable3dgaussian_amd import trainer

    P, world = 37, 10
    op, want = _reset_case(P)
    rng = np.random.default_rng(12)
    shapes = dict(trainer.BASE_GROUPS + trainer.PBR_GROUPS)
    t = {n: _t(rng.normal(size=(P,) + shapes[n]).astype(F)) for n in tc.NAMES}
    t["opacity"] = _t(op).reshape(P, 1)
    st = trainer.GaussianTrainState.from_tensors(t, world=world, rank=rank)
    lo, hi = st.shard_range()
    assert (lo, hi) == (488 * rank, 488 * (rank + 1)) and st.exp_avg.numel() == 488
    m, v = (rng.uniform(0.5, 1.5, size=488).astype(F) for _ in range(2))
    st.exp_avg.copy_(_t(m))
    st.exp_avg_sq.copy_(_t(v))
    p = st.param.cpu().numpy().copy()
    st.reset_opacity()
    torch.cuda.synchronize()
    np.testing.assert_allclose(st.view("opacity").cpu().numpy()[:, 0], want, rtol=1e-6, atol=0)
    seg = np.zeros(p.size, bool)
    seg[481:518] = True
    assert np.array_equal(_bits(st.param.cpu().numpy())[~seg], _bits(p)[~seg])
    mine = seg[lo:hi]
    assert int(mine.sum()) == (7, 30, 0)[rank]
    for g, w in ((st.exp_avg.cpu().numpy(), m), (st.exp_avg_sq.cpu().numpy(), v)):
        assert not g[mine].any() and np.array_equal(_bits(g)[~mine], _bits(w)[~mine])
