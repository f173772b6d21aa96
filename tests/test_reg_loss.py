"""The fused depth, mask-entropy, normal, base-colour and smoothness terms (csrc/reg_loss.hip; the reference's
gaussian_renderer/neilf.py:233-321 and utils/loss_utils.py:65-96) through relightable3dgaussian_amd.loss, the
torch binding and the raw C ABI, against the f64 evaluation of tests/golden/reg_loss.npz (written by
tests/golden/make_golden_reg_loss.py, the smoothness terms by the reference's own function); plus the CPU
checks of the boundary and of the yardstick itself.

Distances, as in tests/test_image_loss.py. Values are compared absolutely (a NaN against a NaN is at distance
0); gradients as a fraction of max(max |f64 gradient| of the map, 1 / elements). A Sobel response within
rounding of 0 can take either sign in f32, so the smoothness gradients are compared except at the pixels within
the 3x3 reach of a response with 0 < |f64 response| < 1e-5 (about 20 x the largest f32 response error, 5.4e-7,
for these inputs); the excluded share is asserted to be at most 1 % per case.

Bars. Each bar is 4 x the reference's own f32-to-f64 distance for that quantity, the largest over all fixture
cases (the fixture's ref32 entries), rounded up to one significant digit: both are f32 evaluations of one
formula that differ in summation order and libm. They are computed from the fixture by bars() and do not depend
on what the kernels give. The measured HIP distances are in DESIGN.md section 2h.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "relightable3dgaussian_amd", "lib", "libr3dg_hip.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "reg_loss.npz")
ALLOC = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
PARITY = 1e-4  # the project's image parity bar
AMBIGUOUS = 1e-5

# in the order of R3DG_REG_* (include/r3dg_hip.h)
TERMS = ("loss_depth", "loss_mask_entropy", "loss_normal_render_depth", "loss_normal_mvs_depth", "loss_base_color",
         "loss_base_color_smooth", "loss_metallic_smooth", "loss_roughness_smooth")
WEIGHTS = ("lambda_depth", "lambda_mask_entropy", "lambda_normal_render_depth", "lambda_normal_mvs_depth",
           "lambda_base_color", "lambda_base_color_smooth", "lambda_metallic_smooth", "lambda_roughness_smooth")
RENDERED = {"opacity": 1, "depth": 1, "normal": 3, "pseudo_normal": 3, "base_color": 3, "roughness": 1, "metallic": 1}
TARGETS = {"gt_image": 3, "gt_depth": 1, "image_mask": 1, "mvs_normal": 3}
ORDER = tuple(RENDERED) + tuple(TARGETS)  # r3dg_reg_loss_inputs
REACHES = {"opacity": (1,), "depth": (0,), "normal": (2, 3), "base_color": (4, 5), "roughness": (7,), "metallic": (6,)}
GRADS = tuple("d_" + k for k in REACHES)
SMOOTH = ("base_color", "roughness", "metallic")
CLAMP32 = (float(np.float32(1e-6)), float(np.float32(1 - 1e-6)))
FIXTURE_CASES = ["r_1x1", "r_5x7", "r_16x16", "r_17x15", "r_16x33", "r_37x53", "flat_half", "no_depth_pixels"]


# ---- fixtures, the f64 restatement and the measure -----------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def case_of(golden, name):
    return {k: golden[f"{name}/{k}"] for k in ORDER}


def fixture64(golden, name):
    return {q: golden[f"{name}/f64/{q}"] for q in TERMS + GRADS}


def lambdas_of(golden):
    return tuple(float(v) for v in golden["lambdas"])


def sobel64(mean, replicate=False):
    """cal_gradient's two responses (loss_utils.py:65-82) of a [1,H,W] double map -> [2,H,W]."""
    kx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], dtype=torch.float64)[None, None]
    ky = torch.tensor([[-1., -2., -1.], [0., 0., 0.], [1., 2., 1.]], dtype=torch.float64)[None, None]
    x = F.pad(mean[None], (1, 1, 1, 1), mode="replicate" if replicate else "constant")
    return torch.cat([F.conv2d(x, kx), F.conv2d(x, ky)], 1)[0]


def smooth64(data, image, mask, replicate=False, over_channels=False):
    """bilateral_smooth_loss (loss_utils.py:85-96) on double tensors; `replicate` (edge-replicate instead of
    zero padding) and `over_channels` (the mean taken over 3N) are two of the deliberately wrong variants."""
    rgb_grad = sobel64(image.mean(0, keepdim=True), replicate).abs().sum(0, keepdim=True)
    data_grad = sobel64(data.mean(0, keepdim=True), replicate).abs().sum(0, keepdim=True)
    s = (data_grad * (-rgb_grad).exp() * mask).mean()
    return s / 3 if over_channels else s


def restate(case, lambdas, replicate=False, not_negated=False, over_channels=False):
    """Every value and the six gradient maps of sum lambda * term, from neilf.py:233-321 restated in f64 (the
    clamp bounds the f32 constants torch uses). The three keyword variants are the wrong restatements the bars
    must reject."""
    t = {k: torch.from_numpy(np.array(case[k])).double() for k in ORDER}
    for k in REACHES:
        t[k].requires_grad_(True)
    m, gd, gt = t["image_mask"], t["gt_depth"], t["gt_image"]
    sel = ~torch.logical_xor(m.bool(), gd > 0)
    if not_negated:
        sel = ~sel
    v = {"loss_depth": F.l1_loss(t["depth"][sel], gd[sel])}
    o = t["opacity"].clamp(*CLAMP32)
    v["loss_mask_entropy"] = -(m * torch.log(o) + (1 - m) * torch.log(1 - o)).mean()
    v["loss_normal_render_depth"] = F.mse_loss(t["normal"] * m, t["pseudo_normal"].detach() * m)
    dm = (gd > 0).double()
    v["loss_normal_mvs_depth"] = F.mse_loss(t["normal"] * dm, t["mvs_normal"] * dm)
    gm = gt * m
    w = 1 / (1 + torch.exp(-5 * (gm.max(0, keepdim=True)[0] - 0.5)))
    target = w * (gm * gm) + (1 - w) * (1 - (1 - gm) * (1 - gm))
    v["loss_base_color"] = F.l1_loss(target, t["base_color"])
    kw = dict(replicate=replicate, over_channels=over_channels)
    v["loss_base_color_smooth"] = smooth64(t["base_color"], gt, m, **kw)
    v["loss_metallic_smooth"] = smooth64(t["metallic"], gt, m, **kw)
    v["loss_roughness_smooth"] = smooth64(t["roughness"], gt, m, **kw)
    out = {k: x.item() for k, x in v.items()}
    for k, reach in REACHES.items():
        total = sum(lambdas[i] * v[TERMS[i]] for i in reach)
        out["d_" + k] = torch.autograd.grad(total, t[k], retain_graph=True)[0].numpy()
    return out


def ambiguous(case):
    """{smoothness map: [H,W] bool}, true within the 3x3 reach of a response with 0 < |f64 response| < AMBIGUOUS."""
    out = {}
    for k in SMOOTH:
        r = sobel64(torch.from_numpy(np.array(case[k])).double().mean(0, keepdim=True)).abs()
        bad = ((r > 0) & (r < AMBIGUOUS)).any(0)[None, None].double()
        out[k] = F.max_pool2d(bad, 3, stride=1, padding=1)[0, 0].bool().numpy()
    return out


def distance(q, got, ref, skip=None):
    """The measure of the module docstring."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (q, got.shape, ref.shape)
    if q in GRADS:
        err = np.abs(got - ref)
        if skip is not None:
            err = np.where(skip[None], 0.0, err)
        return float(err.max() / max(np.abs(ref).max(), 1.0 / ref.size))
    if np.isnan(ref).any():
        assert np.isnan(got).all(), (q, got, ref)
        return 0.0
    return float(np.abs(got - ref).max())


def distances(case, got, ref):
    """{quantity: distance} of one case, the smoothness gradients without their ambiguous pixels (<= 1 %)."""
    skip = ambiguous(case)
    for k, s in skip.items():
        assert s.mean() <= 0.01, (k, s.mean())
    return {q: distance(q, got[q], ref[q], skip.get(q[2:]) if q in GRADS else None) for q in TERMS + GRADS}


def round_up_1sd(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


def bars(golden):
    """4 x the reference's largest f32-to-f64 distance per quantity, rounded up to one significant digit."""
    return {q: round_up_1sd(4 * max(float(golden[f"{n}/ref32/{q}"]) for n in golden["names"])) for q in TERMS + GRADS}


def bits_equal(a, b):
    a, b = (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
            for t in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- CPU: the yardstick ----------------------------------------------------------------------------------

def test_fixture_case_list_is_complete(golden):
    assert FIXTURE_CASES == list(golden["names"])
    assert os.path.getsize(GOLDEN) <= 804 * 1024


def test_restatement_matches_fixture_f64(golden):
    """The f64 restatement above is the reference for shapes too large to commit: it must reproduce every
    fixture's f64 value and gradient."""
    lam = lambdas_of(golden)
    for name in FIXTURE_CASES:
        mine, ref = restate(case_of(golden, name), lam), fixture64(golden, name)
        for q in TERMS + GRADS:
            assert distance(q, mine[q], ref[q]) <= 1e-12, (name, q)
    assert math.isnan(float(golden["no_depth_pixels/f64/loss_depth"]))
    assert not golden["no_depth_pixels/f64/d_depth"].any()


def test_smoothness_restatement_is_the_references_function(golden):
    """smooth64 alone against the values the fixture generator took from the reference's bilateral_smooth_loss."""
    for name in FIXTURE_CASES:
        c = {k: torch.from_numpy(np.array(golden[f"{name}/{k}"])).double() for k in ORDER}
        for data, term in (("base_color", "loss_base_color_smooth"), ("metallic", "loss_metallic_smooth"),
                           ("roughness", "loss_roughness_smooth")):
            got = smooth64(c[data], c["gt_image"], c["image_mask"]).item()
            assert abs(got - float(golden[f"{name}/f64/{term}"])) <= 1e-12, (name, term)


def test_bars_are_tight_enough_to_fail(golden):
    """Every bar is at most the image parity bar, and each wrong restatement (edge-replicate Sobel padding; the
    depth selection not negated; the smoothness mean over 3N) misses the fixtures by more than the bars of the
    quantities it touches, on the case where it departs most."""
    b, lam = bars(golden), lambdas_of(golden)
    print(b)
    assert set(b) == set(TERMS + GRADS)
    assert all(0 < x <= PARITY for x in b.values()), b
    smooth_q = ("loss_base_color_smooth", "loss_metallic_smooth", "loss_roughness_smooth", "d_base_color",
                "d_roughness", "d_metallic")
    for variant, touched in (({"replicate": True}, smooth_q), ({"not_negated": True}, ("loss_depth", "d_depth")),
                             ({"over_channels": True}, smooth_q)):
        worst = dict.fromkeys(touched, 0.0)
        for name in FIXTURE_CASES:
            if name == "no_depth_pixels" and "not_negated" in variant:
                continue  # its f64 value is NaN; the variant's is not, which distance() refuses outright
            bad, ref = restate(case_of(golden, name), lam, **variant), fixture64(golden, name)
            for q in touched:
                worst[q] = max(worst[q], distance(q, bad[q], ref[q]))
        print(variant, worst)
        for q, d in worst.items():
            assert d > b[q], (variant, q, d, b[q])


def test_sign_ambiguity_share(golden):
    """The excluded share is 0 for every fixture and well below 1 % at the larger shapes."""
    for name in FIXTURE_CASES:
        assert all(not s.any() for s in ambiguous(case_of(golden, name)).values()), name
    for name in LARGE:
        share = max(s.mean() for s in ambiguous(large_case(name)[0]).values())
        print(name, share)
        assert share <= 0.01


# ---- CPU: the boundary -----------------------------------------------------------------------------------

class Map(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("plane_stride", ctypes.c_int64), ("row_stride", ctypes.c_int64),
                ("px_stride", ctypes.c_int64)]


class Inputs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("H", ctypes.c_int), ("W", ctypes.c_int), ("terms", ctypes.c_uint)] + \
               [(k, Map) for k in ORDER]


class Grads(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t)] + [(k, ctypes.c_void_p) for k in REACHES]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m relightable3dgaussian_amd.build")
    lib = ctypes.CDLL(LIB)
    lib.r3dg_last_error.restype = ctypes.c_char_p
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.r3dg_reg_loss_forward.restype = ci
    lib.r3dg_reg_loss_forward.argtypes = [ctypes.POINTER(Inputs), vp, vp, ALLOC, vp, vp]
    lib.r3dg_reg_loss_backward.restype = ci
    lib.r3dg_reg_loss_backward.argtypes = [ctypes.POINTER(Inputs), vp, vp, vp, ctypes.POINTER(Grads), vp]
    return lib


def host_inputs(p, H=4, W=4, terms=255, **override):
    """An Inputs whose every map points at p with CHW strides (never dereferenced by the argument checks)."""
    s = Inputs(struct_size=ctypes.sizeof(Inputs), H=H, W=W, terms=terms)
    for k in ORDER:
        setattr(s, k, Map(p, 16, 4, 1))
    for k, v in override.items():
        setattr(s, k, Map(None, 0, 0, 0) if v is None and k in ORDER else v)
    return s


def test_argument_errors_need_no_device(lib):
    """R3DG_ERR_ARG (-1) with a message before any device work or allocation; an empty image or an empty term
    set is R3DG_OK with nothing launched."""
    calls = []

    @ALLOC
    def never(ctx, nbytes):
        calls.append(nbytes)
        return None

    no_alloc = ctypes.cast(None, ALLOC)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    all_grads = Grads(ctypes.sizeof(Grads), *([p.value] * 6))

    def fwd(values=p, count=p, alloc=never, **kw):
        return lib.r3dg_reg_loss_forward(ctypes.byref(host_inputs(p, **kw)), values, count, alloc, None, None)

    def bwd(count=p, weights=p, grads=all_grads, **kw):
        return lib.r3dg_reg_loss_backward(ctypes.byref(host_inputs(p, **kw)), count, weights, None,
                                          ctypes.byref(grads) if grads is not None else None, None)

    needs = {"depth": 1 << 0, "gt_depth": 1 << 0, "opacity": 1 << 1, "normal": 1 << 2, "pseudo_normal": 1 << 2,
             "mvs_normal": 1 << 3, "gt_image": 1 << 4, "base_color": 1 << 5, "metallic": 1 << 6, "roughness": 1 << 7}
    bad = {"negative H": dict(H=-1), "negative W": dict(W=-1), "beyond int32": dict(H=65536, W=32768),
           "struct_size 0": dict(struct_size=0), "struct_size + 8": dict(struct_size=ctypes.sizeof(Inputs) + 8),
           "unknown term bit": dict(terms=1 << 8)}
    bad.update({f"null {k} with its term alone": {k: None, "terms": bit} for k, bit in needs.items()})
    bad["null gt_depth for the mvs term"] = dict(gt_depth=None, terms=1 << 3)
    bad["null normal for the mvs term"] = dict(normal=None, terms=1 << 3)
    bad["null gt_image for a smoothness term"] = dict(gt_image=None, terms=1 << 7)
    bad["null base_color for the guide"] = dict(base_color=None, terms=1 << 4)
    for what, kw in bad.items():
        for call in (fwd, bwd):
            assert call(**kw) == -1, (call.__name__, what)
            assert len(lib.r3dg_last_error()) > 0, what
    for what, call in {"fwd null values": lambda: fwd(values=None), "fwd null depth_count": lambda: fwd(count=None),
                       "fwd null scratch_alloc": lambda: fwd(alloc=no_alloc),
                       "bwd null weights": lambda: bwd(weights=None), "bwd null grads": lambda: bwd(grads=None),
                       "bwd null depth_count": lambda: bwd(count=None),
                       "bwd grads struct_size": lambda: bwd(grads=Grads(8, *([p.value] * 6)))}.items():
        assert call() == -1, what
        assert len(lib.r3dg_last_error()) > 0, what
    assert lib.r3dg_reg_loss_forward(None, p, p, never, None, None) == -1
    assert fwd(image_mask=None, alloc=never, terms=0) == 0  # the mask is optional; checked below with terms on
    for zero in (dict(H=0), dict(W=0), dict(terms=0)):
        assert fwd(**zero) == 0 and bwd(**zero) == 0, zero
        assert fwd(values=None, count=None, alloc=no_alloc, **zero) == 0, zero
    assert calls == []
    # an absent mask and maps that only disabled terms touch are no error: the call gets as far as the allocator
    assert fwd(image_mask=None, opacity=None, normal=None, pseudo_normal=None, mvs_normal=None, metallic=None,
               roughness=None, terms=(1 << 0) | (1 << 4) | (1 << 5)) == -4  # R3DG_ERR_ALLOC from `never`
    assert len(calls) == 1 and calls[0] >= 36


def test_torch_binding_rejects_bad_input():
    import relightable3dgaussian_amd as r

    one, three = torch.zeros(1, 8, 8), torch.zeros(3, 8, 8)
    maps = [one, one, three, three, three, one, one, three, one, one, three]
    w, cnt = torch.zeros(8), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        r._C.reg_loss_forward(maps, 8, 8, 255, False)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        r._C.reg_loss_backward(maps, 8, 8, 255, False, cnt, w)
    with pytest.raises(RuntimeError, match="float32"):
        r._C.reg_loss_forward([one.double()] + maps[1:], 8, 8, 255, False)
    with pytest.raises(RuntimeError, match="float32"):
        r._C.reg_loss_backward([one.half()] + maps[1:], 8, 8, 255, False, cnt, w)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        r._C.reg_loss_forward(maps, 8, 9, 255, False)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        r._C.reg_loss_forward(maps, 8, 8, 255, True)  # hwc wants [H,W,n] rendered maps
    with pytest.raises(RuntimeError, match="11 maps"):
        r._C.reg_loss_forward(maps[:5], 8, 8, 255, False)
    with pytest.raises(RuntimeError, match="terms"):
        r._C.reg_loss_forward(maps, 8, 8, 256, False)
    with pytest.raises(RuntimeError, match="no map"):
        r._C.reg_loss_forward([None] * 11, 8, 8, 255, False)


def test_python_module_argument_errors():
    from relightable3dgaussian_amd import loss

    one, three = torch.zeros(1, 8, 8), torch.zeros(3, 8, 8)
    with pytest.raises(ValueError, match="image_layout"):
        loss.regularizer_losses({"opacity": one}, {}, {"lambda_mask_entropy": 0.1}, image_layout="nhwc")
    with pytest.raises(ValueError, match="needs"):  # a map a term needs but did not get
        loss.regularizer_losses({"opacity": one}, {}, {"lambda_depth": 1.0})
    with pytest.raises(ValueError, match="needs"):
        loss.regularizer_losses({"normal": three}, {"gt_depth": one}, {"lambda_normal_mvs_depth": 0.01})
    with pytest.raises(ValueError, match="gradient"):  # a target that requires grad
        loss.regularizer_losses({"depth": one}, {"gt_depth": one.clone().requires_grad_(True)}, {"lambda_depth": 1.0})
    with pytest.raises(ValueError, match="shape mismatch"):
        loss.regularizer_losses({"depth": one}, {"gt_depth": torch.zeros(1, 8, 9)}, {"lambda_depth": 1.0})
    with pytest.raises(ValueError, match="shape mismatch"):  # hwc wants [H,W,n] rendered maps
        loss.regularizer_losses({"depth": one}, {"gt_depth": one}, {"lambda_depth": 1.0}, image_layout="hwc")
    with pytest.raises(ValueError, match="shape mismatch"):
        loss.regularizer_losses({"normal": one, "pseudo_normal": three}, {}, {"lambda_normal_render_depth": 1.0})
    with pytest.raises(ValueError, match="unknown map"):
        loss.regularizer_losses({"albedo": three}, {}, {"lambda_base_color": 1.0})
    with pytest.raises(ValueError, match="shape mismatch"):
        loss.bilateral_smooth_loss(three, torch.zeros(3, 8, 9), one)
    with pytest.raises(ValueError, match="data"):
        loss.bilateral_smooth_loss(torch.zeros(2, 8, 8), three, one)
    with pytest.raises(RuntimeError, match="GPU tensor"):  # no torch fallback
        loss.regularizer_losses({"opacity": one}, {}, {"lambda_mask_entropy": 0.1})
    with pytest.raises(RuntimeError, match="GPU tensor"):
        loss.bilateral_smooth_loss(three, three, one)
    total, stats = loss.regularizer_losses({"opacity": one}, {}, {"lambda_mask_entropy": 0.0})  # nothing enabled
    assert float(total) == 0.0 and stats == {}


# ---- GPU ---------------------------------------------------------------------------------------------------

def _cuda(a, grad=False, hwc=False):
    t = torch.from_numpy(np.array(a, np.float32)).cuda()
    if hwc:
        t = t.permute(1, 2, 0).contiguous()
    return t.requires_grad_(grad)


def hip_all(case, lambdas, layout="chw", k=None):
    """Every quantity of a case from regularizer_losses: the eight values, the loss, and the six gradient maps
    of (loss, or loss * k) brought back to [n,H,W]."""
    from relightable3dgaussian_amd import loss

    hwc = layout == "hwc"
    maps = {n: _cuda(case[n], n in REACHES, hwc) for n in RENDERED}
    targets = {n: _cuda(case[n]) for n in TARGETS}
    total, stats = loss.regularizer_losses(maps, targets, dict(zip(WEIGHTS, lambdas)), image_layout=layout)
    enabled = [t for t, l in zip(TERMS, lambdas) if l > 0]
    assert total.dim() == 0 and sorted(stats) == sorted(enabled)
    for v in stats.values():
        assert v.dim() == 0 and v.is_cuda and not v.requires_grad
    out = {t: stats[t].item() if t in stats else None for t in TERMS}
    out["loss"], out["stats"] = total.detach(), stats
    wanted = [n for n, reach in REACHES.items() if any(lambdas[i] > 0 for i in reach)]
    grads = torch.autograd.grad(total if k is None else total * k, [maps[n] for n in wanted], allow_unused=True)
    for n in REACHES:
        g = grads[wanted.index(n)] if n in wanted else None
        if g is not None:
            assert g.shape == maps[n].shape and g.is_contiguous()
            g = (g.permute(2, 0, 1) if hwc else g).contiguous().cpu().numpy()
        out["d_" + n] = g
    return out


LARGE = {"tiles_135x240": (135, 240), "rows_16x4099": (16, 4099)}
LARGE_LAMBDAS = (1.0, 0.5, 2.0, 1.5, 1.0, 0.75, 1.25, 0.5)
_LARGE_CACHE: dict = {}


def large_case(name):
    """(case, f64 restatement) of a shape too large to commit, computed once and never modified."""
    if name not in _LARGE_CACHE:
        h, w = LARGE[name]
        rng = np.random.default_rng(2025 + sorted(LARGE).index(name))
        case = {k: rng.random((n, h, w), dtype=np.float32) for k, n in {**RENDERED, **TARGETS}.items()}
        for k in ("normal", "pseudo_normal", "mvs_normal"):
            n = rng.standard_normal((3, h, w)).astype(np.float32)
            case[k] = (n / np.sqrt((n.astype(np.float64) ** 2).sum(0, keepdims=True))).astype(np.float32)
        case["image_mask"] = (rng.random((1, h, w)) > 0.3).astype(np.float32)
        case["gt_depth"] = np.where(rng.random((1, h, w)) > 0.4, case["gt_depth"] + np.float32(0.5),
                                    np.float32(0)).astype(np.float32)
        ref = restate(case, LARGE_LAMBDAS)
        for a in list(case.values()) + [ref[q] for q in GRADS]:
            a.setflags(write=False)
        _LARGE_CACHE[name] = (case, ref)
    return _LARGE_CACHE[name]


def check(name, case, got, ref, b):
    d = distances(case, got, ref)
    print(name, d)
    for q in d:
        assert d[q] <= b[q], (name, q, d[q], b[q])
    return d


def hip_distances(golden):
    """{case: {quantity: distance to f64}} over the fixtures and the two larger shapes (what DESIGN 2h tabulates
    and profiles/loss/reg_loss_distances.json records)."""
    out = {}
    for name in FIXTURE_CASES:
        case = case_of(golden, name)
        out[name] = distances(case, hip_all(case, lambdas_of(golden)), fixture64(golden, name))
    for name in LARGE:
        case, ref = large_case(name)
        out[name] = distances(case, hip_all(case, LARGE_LAMBDAS), ref)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_fixture_cases(hip_ext, golden, name, layout):
    case = case_of(golden, name)
    check(f"{name}/{layout}", case, hip_all(case, lambdas_of(golden), layout), fixture64(golden, name), bars(golden))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LARGE))
def test_larger_shapes(hip_ext, golden, name):
    """135x240: 9 x 15 tiles, partial on the lower edge; 16x4099: one row of 257 tiles, one more than the
    finishing kernel has threads, so its strided loop takes a second round."""
    case, ref = large_case(name)
    check(name, case, hip_all(case, LARGE_LAMBDAS), ref, bars(golden))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_bilateral_smooth_loss_fixtures(hip_ext, golden, name):
    """The drop-in with the reference's signature, 3-channel and 1-channel data, value and gradient."""
    from relightable3dgaussian_amd import loss

    case, ref, b, lam = case_of(golden, name), fixture64(golden, name), bars(golden), lambdas_of(golden)
    image, mask, skip = _cuda(case["gt_image"]), _cuda(case["image_mask"]), ambiguous(case)
    for data, term, i in (("metallic", "loss_metallic_smooth", 6), ("roughness", "loss_roughness_smooth", 7)):
        x = _cuda(case[data], True)
        v = loss.bilateral_smooth_loss(x, image, mask)
        g, = torch.autograd.grad(v * lam[i], x)
        d = (distance(term, v.item(), ref[term]), distance("d_" + data, g.cpu().numpy(), ref["d_" + data], skip[data]))
        print(name, data, d)
        assert d[0] <= b[term] and d[1] <= b["d_" + data], (name, data, d)
    x = _cuda(case["base_color"], True)
    v = loss.bilateral_smooth_loss(x, image, mask[0])  # an [H,W] mask
    assert v.dim() == 0 and distance("loss_base_color_smooth", v.item(), ref["loss_base_color_smooth"]) <= \
        b["loss_base_color_smooth"]
    g, = torch.autograd.grad(v, x)  # the fixture's base_color gradient holds the guide as well: against the restatement
    only = restate(case, tuple(1.0 if i == 5 else 0.0 for i in range(8)))["d_base_color"]
    assert distance("d_base_color", g.cpu().numpy(), only, skip["base_color"]) <= b["d_base_color"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["r_37x53", "r_16x33", "flat_half"])
def test_hwc_layout_is_bitwise_chw(hip_ext, golden, name):
    case, lam = case_of(golden, name), lambdas_of(golden)
    chw, hwc = hip_all(case, lam), hip_all(case, lam, layout="hwc")
    assert bits_equal(chw["loss"], hwc["loss"])
    for t in TERMS:
        assert bits_equal(chw["stats"][t], hwc["stats"][t]), t
    for q in GRADS:
        assert bits_equal(chw[q], hwc[q]), q


@pytest.mark.gpu
def test_repeatable_bit_for_bit(hip_ext, golden):
    case = large_case("tiles_135x240")[0]
    a, b = hip_all(case, LARGE_LAMBDAS), hip_all(case, LARGE_LAMBDAS)
    assert bits_equal(a["loss"], b["loss"])
    for t in TERMS:
        assert bits_equal(a["stats"][t], b["stats"][t]), t
    for q in GRADS:
        assert bits_equal(a[q], b[q]), q


@pytest.mark.gpu
def test_subset_of_terms(hip_ext, golden):
    """Depth, mask entropy and roughness smoothness alone: the other maps get no gradient, and the shared terms
    and their (unshared) gradient maps have the full run's bits."""
    case, lam = case_of(golden, "r_37x53"), lambdas_of(golden)
    full = hip_all(case, lam)
    sub = hip_all(case, tuple(l if i in (0, 1, 7) else 0.0 for i, l in enumerate(lam)))
    assert sorted(sub["stats"]) == ["loss_depth", "loss_mask_entropy", "loss_roughness_smooth"]
    for t in sub["stats"]:
        assert bits_equal(sub["stats"][t], full["stats"][t]), t
    for q in ("d_depth", "d_opacity", "d_roughness"):
        assert bits_equal(sub[q], full[q]), q
    for q in ("d_normal", "d_base_color", "d_metallic"):
        assert sub[q] is None, q
    # a single term of a shared map, against the restatement with the other weights at 0
    one = tuple(l if i == 3 else 0.0 for i, l in enumerate(lam))
    got, ref = hip_all(case, one), restate(case, one)
    assert distance("d_normal", got["d_normal"], ref["d_normal"]) <= bars(golden)["d_normal"]
    assert distance("loss_normal_mvs_depth", got["loss_normal_mvs_depth"], ref["loss_normal_mvs_depth"]) <= \
        bars(golden)["loss_normal_mvs_depth"]
    # maps that only disabled terms touch may be left out altogether, and the mask may be absent
    from relightable3dgaussian_amd import loss
    o = _cuda(case["opacity"], True)
    total, stats = loss.regularizer_losses({"opacity": o}, {}, {"lambda_mask_entropy": 0.5})
    ones = dict(case, image_mask=np.ones_like(case["image_mask"]))
    want = restate(ones, tuple(0.5 if i == 1 else 0.0 for i in range(8)))
    g, = torch.autograd.grad(total, o)
    assert list(stats) == ["loss_mask_entropy"]
    assert distance("loss_mask_entropy", stats["loss_mask_entropy"].item(), want["loss_mask_entropy"]) <= \
        bars(golden)["loss_mask_entropy"]
    assert distance("d_opacity", g.cpu().numpy(), want["d_opacity"]) <= bars(golden)["d_opacity"]


@pytest.mark.gpu
def test_upstream_scalar_multiplies_last(hip_ext, golden):
    """(loss * 3.5).backward() is fl(3.5 * gradient), bit for bit: the upstream gradient is read on the device
    and multiplies last."""
    case, lam = case_of(golden, "r_37x53"), lambdas_of(golden)
    g1, g35 = hip_all(case, lam), hip_all(case, lam, k=3.5)
    for q in GRADS:
        assert np.abs(g1[q]).max() > 0
        assert bits_equal(g35[q], (g1[q].astype(np.float64) * 3.5).astype(np.float32)), q


@pytest.mark.gpu
def test_no_depth_pixels_is_nan_with_zero_gradient(hip_ext, golden):
    got = hip_all(case_of(golden, "no_depth_pixels"), lambdas_of(golden))
    assert math.isnan(got["loss_depth"]) and math.isnan(got["loss"].item())
    assert not got["d_depth"].any()
    for t in TERMS[1:]:
        assert math.isfinite(got[t]), t
    for q in GRADS:
        assert np.isfinite(got[q]).all(), q


@pytest.mark.gpu
def test_nan_opacity_propagates_as_in_torch(hip_ext, golden):
    """torch's clamp lets a NaN through: the term is NaN, that pixel's gradient 0, the other pixels' finite and
    the other terms untouched. The f64 restatement (torch's own clamp) says the same."""
    lam = lambdas_of(golden)
    case = dict(case_of(golden, "r_5x7"))
    base = hip_all(case, lam)
    case["opacity"] = np.array(case["opacity"])
    case["opacity"][0, 2, 3] = np.nan
    got, ref = hip_all(case, lam), restate(case, lam)
    assert math.isnan(ref["loss_mask_entropy"]) and math.isnan(got["loss_mask_entropy"])
    assert ref["d_opacity"][0, 2, 3] == 0 and got["d_opacity"][0, 2, 3] == 0
    keep = np.ones((1, 5, 7), bool)
    keep[0, 2, 3] = False
    assert np.isfinite(got["d_opacity"]).all() and bits_equal(got["d_opacity"][keep], base["d_opacity"][keep])
    for t in TERMS:
        if t != "loss_mask_entropy":
            assert bits_equal(got["stats"][t], base["stats"][t]), t


@pytest.mark.gpu
def test_flat_half_gives_exact_zeros(hip_ext, golden):
    """sign(0), the exactly zero Sobel response of equal means, and the clamp: no gradient on the flat interior
    (two pixels from the image edge, whose zero padding is a step, and from the random half), at depth ==
    gt_depth, and on the opacity stripes at exactly 0 and exactly 1."""
    case = case_of(golden, "flat_half")
    got = hip_all(case, lambdas_of(golden))
    for q in ("d_base_color", "d_roughness", "d_metallic"):
        g = got[q]
        assert not g[:, 2:-2, 2:8].any(), q
        assert g[:, :, 10:].any(), q
    assert not got["d_depth"][:, :, :10].any() and got["d_depth"][:, :, 10:].any()
    assert not got["d_opacity"][:, 3].any() and not got["d_opacity"][:, 5].any() and got["d_opacity"][:, 4].all()


@pytest.mark.gpu
def test_no_grad_and_other_stream(hip_ext, golden):
    from relightable3dgaussian_amd import loss

    case, lam = case_of(golden, "r_37x53"), lambdas_of(golden)
    base = hip_all(case, lam)
    maps, targets = {n: _cuda(case[n], n in REACHES) for n in RENDERED}, {n: _cuda(case[n]) for n in TARGETS}
    with torch.no_grad():
        quiet, stats = loss.regularizer_losses(maps, targets, dict(zip(WEIGHTS, lam)))
    assert not quiet.requires_grad and bits_equal(quiet, base["loss"])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = hip_all(case, lam)
    s.synchronize()
    assert bits_equal(other["loss"], base["loss"])
    for q in GRADS:
        assert bits_equal(other[q], base[q]), q


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_raw_c_abi(hip_ext, lib, golden, name):
    """Both entry points through ctypes on device pointers (HWC strides for the rendered maps), scratch from a
    torch-backed callback, lambda times an upstream 1 in `weights` and no scale: within the bars of the f64
    fixture, and bitwise what the binding returns."""
    case, lam = case_of(golden, name), lambdas_of(golden)
    H, W = case["opacity"].shape[1:]
    dev = {k: _cuda(case[k], hwc=k in RENDERED) for k in ORDER}
    s = Inputs(struct_size=ctypes.sizeof(Inputs), H=H, W=W, terms=255)
    for k, n in RENDERED.items():
        setattr(s, k, Map(dev[k].data_ptr(), 1, W * n, n))
    for k in TARGETS:
        setattr(s, k, Map(dev[k].data_ptr(), H * W, W, 1))
    keep = []

    @ALLOC
    def torch_alloc(ctx, nbytes):
        t = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        keep.append(t)
        return t.data_ptr()

    values, count = torch.empty(8, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    weights = torch.tensor(lam, device="cuda")
    grads = {k: torch.empty_like(dev[k]) for k in REACHES}
    g = Grads(ctypes.sizeof(Grads), *[grads[k].data_ptr() for k in REACHES])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.r3dg_reg_loss_forward(ctypes.byref(s), values.data_ptr(), count.data_ptr(), torch_alloc, None, stream)
    assert rc == 0, lib.r3dg_last_error()
    rc = lib.r3dg_reg_loss_backward(ctypes.byref(s), count.data_ptr(), weights.data_ptr(), None, ctypes.byref(g), stream)
    assert rc == 0, lib.r3dg_last_error()
    torch.cuda.synchronize()
    tiles = ((H + 15) // 16) * ((W + 15) // 16)
    assert len(keep) == 1 and keep[0].numel() >= 36 * tiles
    m, gd = case["image_mask"], case["gt_depth"]
    assert int(count.item()) == int(((m != 0) == (gd > 0)).sum())  # the exact count
    got = {t: values[i].item() for i, t in enumerate(TERMS)}
    got.update({"d_" + k: grads[k].permute(2, 0, 1).contiguous().cpu().numpy() for k in REACHES})
    check(name, case, got, fixture64(golden, name), bars(golden))
    maps = [dev[k] for k in ORDER]
    v2, c2 = hip_ext.reg_loss_forward(maps, H, W, 255, True)
    g2 = hip_ext.reg_loss_backward(maps, H, W, 255, True, c2, weights)
    assert bits_equal(values, v2) and int(c2.item()) == int(count.item())
    for k, t in zip(REACHES, g2):
        assert bits_equal(grads[k], t), k


if __name__ == "__main__":
    # python tests/test_reg_loss.py [out.json]: the record of profiles/loss/reg_loss_distances.json (needs the GPU)
    import json
    import sys

    sys.path.insert(0, ROOT)
    z = np.load(GOLDEN)
    fixtures = {k: z[k] for k in z.files}
    per_case, b = hip_distances(fixtures), bars(fixtures)
    record = {"device": torch.cuda.get_device_name(0), "bars": b,
              "reference_f32_to_f64_max": {q: max(float(fixtures[f"{n}/ref32/{q}"]) for n in FIXTURE_CASES) for q in b},
              "hip_to_f64_max": {q: dict(zip(("distance", "case"), max((d[q], n) for n, d in per_case.items()))) for q in b},
              "hip_to_f64": per_case}
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "loss", "reg_loss_distances.json")
    with open(out, "w") as f:
        json.dump(record, f, indent=1)
    for q in b:
        print(q, "bar", b[q], "reference", record["reference_f32_to_f64_max"][q], "hip", record["hip_to_f64_max"][q])
