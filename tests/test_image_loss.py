"""The fused L1 + SSIM image loss (csrc/loss.hip; the reference's utils/loss_utils.py ssim and the loss of
gaussian_renderer/neilf.py:216-222) through relightable3dgaussian_amd.loss, the torch binding and the raw C
ABI, against the reference's own f64 evaluation (tests/golden/loss.npz, written by
tests/golden/make_golden_loss.py); plus the CPU checks of the boundary and of the yardstick itself.

Distances. Values (ssim, l1, psnr, loss) are compared absolutely; gradients as a fraction of
max(max |f64 gradient| of the case, 1 / number of elements). The floor is the size of one pixel's share of a mean: in
the constant-against-constant case the exact gradient is 0 (the f64 one is 1e-17), which is no unit to
measure in. BARS holds, per quantity, 4 x the largest HIP-to-f64 distance measured on an MI355X over all
cases below (fixtures and the two larger shapes), rounded up to one significant digit; the measured
figures and the reference's own f32-to-f64 distances are in DESIGN.md section 2g.
"""
from __future__ import annotations

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "r3dg_hip.h")
LIB = os.path.join(ROOT, "relightable3dgaussian_amd", "lib", "libr3dg_hip.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "loss.npz")
ALLOC = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
LAMBDA = 0.2
PARITY = 1e-4  # the project's image parity bar

#                        largest HIP-to-f64 distance measured (MI355X)   the reference's f32-to-f64
BARS = {"ssim": 3e-7,   # 6.85e-8  (c1_11x11)                           1.32e-7
        "l1": 4e-8,     # 7.63e-9  (c3_37x53)                           9.01e-9
        "psnr": 8e-6,   # 1.96e-6  (rows_16x4099), dB                   1.81e-6
        "loss": 5e-8,   # 1.21e-8  (c1_11x11)                           1.93e-8
        "dssim": 7e-6,  # 1.57e-6  (c1_11x11)                           3.41e-5 (constant)
        "dloss": 3e-6}  # 6.36e-7  (rows_16x4099)                       1.72e-5 (constant)
VALUES, GRADS = ("ssim", "l1", "psnr", "loss"), ("dssim", "dloss")


# ---- fixtures and the f64 restatement ------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def single_cases(golden):
    return [n for n in golden["names"] if n != "batch"]


def window64(channel, sigma=1.5):
    """create_window (loss_utils.py:19-28): the f32 1-D Gaussian, its f32 outer product, then double."""
    g = torch.Tensor([math.exp(-(x - 5) ** 2 / float(2 * sigma ** 2)) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float()[None, None].expand(channel, 1, 11, 11).contiguous().double()


def ssim64(x, y, sigma=1.5, replicate=False, size_average=True):
    """_ssim (loss_utils.py:42-62) on double tensors; `sigma` and `replicate` (edge-replicate instead of
    zero padding) are the two deliberately wrong variants the bars must reject."""
    c = x.size(-3)
    win = window64(c, sigma)

    def conv(t):
        t = t if t.dim() == 4 else t[None]
        if replicate:
            return F.conv2d(F.pad(t, (5, 5, 5, 5), mode="replicate"), win, groups=c)
        return F.conv2d(t, win, padding=5, groups=c)

    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu1_mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1_mu2 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def restate(img, gt, **variant):
    """Every quantity of a [C,H,W] fixture case from the restatement, in f64."""
    x = torch.from_numpy(np.array(img)).double().requires_grad_(True)
    y = torch.from_numpy(np.array(gt)).double()
    s = ssim64(x, y, **variant)
    l1 = F.l1_loss(x, y)
    loss = (1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - s)
    mse = ((x - y) ** 2).view(x.shape[0], -1).mean(1, keepdim=True)
    psnr = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()
    dssim, = torch.autograd.grad(s, x, retain_graph=True)
    dloss, = torch.autograd.grad(loss, x)
    return {"ssim": s.item(), "l1": l1.item(), "psnr": psnr.item(), "loss": loss.item(),
            "dssim": dssim.numpy(), "dloss": dloss.numpy()}


def fixture64(golden, name):
    return {q: golden[f"{name}/f64/{q}"] for q in VALUES + GRADS}


def distance(q, got, ref):
    """The measure of the module docstring; equal infinities (psnr of identical images) are at distance 0."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (q, got.shape, ref.shape)
    if q in GRADS:
        return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1.0 / ref.size))
    if np.isinf(ref).any():
        assert np.array_equal(got, ref), (q, got, ref)
        return 0.0
    return float(np.abs(got - ref).max())


def bits_equal(a, b):
    a, b = (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
            for t in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- CPU: the yardstick ----------------------------------------------------------------------------------

def test_restatement_matches_fixture_f64(golden):
    """The f64 restatement above is the reference for shapes too large to commit: it must reproduce every
    fixture's f64 value and gradient."""
    for name in single_cases(golden):
        mine, ref = restate(golden[f"{name}/img"], golden[f"{name}/gt"]), fixture64(golden, name)
        for q in VALUES + GRADS:
            assert distance(q, mine[q], ref[q]) <= 1e-12, (name, q)
    x = torch.from_numpy(np.array(golden["batch/img"])).double().requires_grad_(True)
    y = torch.from_numpy(np.array(golden["batch/gt"])).double()
    per = ssim64(x, y, size_average=False)
    assert np.abs(per.detach().numpy() - golden["batch/f64/ssim_b"]).max() <= 1e-12
    g, = torch.autograd.grad((per * torch.tensor([1.0, 2.0], dtype=torch.float64)).sum(), x)
    assert distance("dssim", g.numpy().reshape(6, 12, 18), golden["batch/f64/dssim_b"].reshape(6, 12, 18)) <= 1e-12


def test_bars_are_tight_enough_to_fail(golden):
    """Every bar is below the image parity bar, and both wrong variants (sigma 1.6; edge-replicate padding)
    miss the fixtures by more than every bar on the case where they depart most."""
    assert set(BARS) == set(VALUES + GRADS)
    assert all(0 < b < PARITY for b in BARS.values()), BARS
    for variant in ({"sigma": 1.6}, {"replicate": True}):
        worst = dict.fromkeys(("ssim", "loss") + GRADS, 0.0)  # l1 and psnr do not pass through the window
        for name in single_cases(golden):
            bad, ref = restate(golden[f"{name}/img"], golden[f"{name}/gt"], **variant), fixture64(golden, name)
            for q in worst:
                worst[q] = max(worst[q], distance(q, bad[q], ref[q]))
        print(variant, worst)
        for q, d in worst.items():
            assert d > BARS[q], (variant, q, d, BARS[q])


# ---- CPU: the boundary -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m relightable3dgaussian_amd.build")
    lib = ctypes.CDLL(LIB)
    lib.r3dg_last_error.restype = ctypes.c_char_p
    i64, vp, ci = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
    image = [ci, ci, ci, vp, i64, i64, i64, vp, i64, i64, i64]
    lib.r3dg_image_loss_forward.restype = ci
    lib.r3dg_image_loss_forward.argtypes = image + [vp, vp, ALLOC, vp, vp]
    lib.r3dg_image_loss_backward.restype = ci
    lib.r3dg_image_loss_backward.argtypes = image + [vp, vp, vp, vp, vp, vp]
    return lib


def test_header_declares_and_library_exports(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+r3dg_image_loss_forward\s*\(\s*int\s+planes\s*,\s*int\s+H\s*,\s*int\s+W\s*,", text)
    assert re.search(r"\bint\s+r3dg_image_loss_backward\s*\(\s*int\s+planes\s*,\s*int\s+H\s*,\s*int\s+W\s*,", text)
    assert hasattr(lib, "r3dg_image_loss_forward") and hasattr(lib, "r3dg_image_loss_backward")
    assert int(re.search(r"#define R3DG_ABI_VERSION (\d+)", text).group(1)) == 2  # additive: no struct changed


def test_argument_errors_need_no_device(lib):
    """R3DG_ERR_ARG (-1) with a message before any device work or allocation; a zero-sized image is R3DG_OK."""
    calls = []

    @ALLOC
    def never(ctx, nbytes):
        calls.append(nbytes)
        return None

    no_alloc = ctypes.cast(None, ALLOC)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(planes=1, H=4, W=4, img=p, gt=p, sums=p, dmaps=None, alloc=never):
        return lib.r3dg_image_loss_forward(planes, H, W, img, 16, 4, 1, gt, 16, 4, 1, sums, dmaps, alloc, None, None)

    def bwd(planes=1, H=4, W=4, img=p, gt=p, dmaps=p, ws=p, wa=p, out=p):
        return lib.r3dg_image_loss_backward(planes, H, W, img, 16, 4, 1, gt, 16, 4, 1, dmaps, ws, wa, None, out, None)

    bad = {"fwd negative planes": lambda: fwd(planes=-1), "fwd negative H": lambda: fwd(H=-1),
           "fwd negative W": lambda: fwd(W=-1), "fwd null img": lambda: fwd(img=None),
           "fwd null gt": lambda: fwd(gt=None), "fwd null sums": lambda: fwd(sums=None),
           "fwd null scratch_alloc": lambda: fwd(alloc=no_alloc),
           "fwd beyond int32": lambda: fwd(planes=3, H=65536, W=16384),
           "bwd negative planes": lambda: bwd(planes=-1), "bwd negative H": lambda: bwd(H=-1),
           "bwd negative W": lambda: bwd(W=-1), "bwd null img": lambda: bwd(img=None),
           "bwd null gt": lambda: bwd(gt=None), "bwd null dmaps": lambda: bwd(dmaps=None),
           "bwd null w_ssim": lambda: bwd(ws=None), "bwd null w_abs": lambda: bwd(wa=None),
           "bwd null dL_dimg": lambda: bwd(out=None), "bwd beyond int32": lambda: bwd(planes=3, H=65536, W=16384)}
    for what, call in bad.items():
        assert call() == -1, what
        assert len(lib.r3dg_last_error()) > 0, what
    for zero in ({"planes": 0}, {"H": 0}, {"W": 0}):
        assert fwd(**zero) == 0 and bwd(**zero) == 0, zero
        assert fwd(img=None, gt=None, sums=None, alloc=no_alloc, **zero) == 0, zero
    assert calls == []


def test_torch_binding_rejects_bad_input():
    import relightable3dgaussian_amd as r

    a = torch.zeros(3, 8, 8)
    w = torch.zeros(3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        r._C.image_loss_forward(a, a, False, True)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        r._C.image_loss_backward(a, a, False, torch.zeros(3, 3, 8, 8), w, w)
    with pytest.raises(RuntimeError, match="float32"):
        r._C.image_loss_forward(a.double(), a, False, True)
    with pytest.raises(RuntimeError, match="float32"):
        r._C.image_loss_backward(a, a.double(), False, torch.zeros(3, 3, 8, 8), w, w)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        r._C.image_loss_forward(a, torch.zeros(3, 8, 9), False, True)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        r._C.image_loss_forward(a, a, True, True)  # hwc wants [H,W,C] against [C,H,W]
    with pytest.raises(RuntimeError, match="shape mismatch"):
        r._C.image_loss_backward(torch.zeros(8, 8, 4), a, True, torch.zeros(3, 3, 8, 8), w, w)


def test_python_module_argument_errors():
    from relightable3dgaussian_amd import loss

    a = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError, match="window_size"):
        loss.ssim(a, a, window_size=7)
    with pytest.raises(ValueError, match="img2"):
        loss.ssim(a, a.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="size_average"):
        loss.ssim(a, a, size_average=False)
    with pytest.raises(ValueError, match="image_layout"):
        loss.l1_ssim_loss(a, a, LAMBDA, image_layout="nhwc")
    with pytest.raises(ValueError, match="layout"):
        loss.l1_ssim_loss(a, a, LAMBDA, image_layout="hwc")
    with pytest.raises(RuntimeError, match="GPU tensor"):  # no torch fallback
        loss.ssim(a, a)


def test_window_constants_are_the_references(golden):
    """The kernels' 11 weights are gaussian(11, 1.5) bit for bit: their f32 outer product is the reference's
    2-D window, and they are its middle row rescaled (window[5, :] / window[5, 5] * g[5]; that expression
    itself rounds, so it is compared to one f32 rounding)."""
    import relightable3dgaussian_amd as r

    k = np.array(r._C.image_loss_window(), np.float32)
    assert k.shape == (11,) and bits_equal(k, golden["gauss"])
    win = golden["window"]
    assert win.shape == (1, 1, 11, 11) and bits_equal(np.outer(k, k).astype(np.float32), win[0, 0])
    mid = win[0, 0, 5, :].astype(np.float64) / float(win[0, 0, 5, 5]) * float(k[5])
    assert np.abs(mid / k.astype(np.float64) - 1.0).max() <= 2.0 ** -23


# ---- GPU ---------------------------------------------------------------------------------------------------

def _cuda(a, grad=False):
    return torch.from_numpy(np.array(a, np.float32)).cuda().requires_grad_(grad)


def hip_single(img, gt, layout="chw"):
    """Every quantity of a [C,H,W] case from the HIP operator: loss.ssim for ssim / dssim, l1_ssim_loss
    for the rest (its own ssim statistic is checked against loss.ssim's bits)."""
    from relightable3dgaussian_amd import loss

    x, y = _cuda(img, True), _cuda(gt)
    s = loss.ssim(x, y)
    dssim, = torch.autograd.grad(s, x)
    xi = x.detach().permute(1, 2, 0).contiguous().requires_grad_(True) if layout == "hwc" else x
    total, stats = loss.l1_ssim_loss(xi, y, LAMBDA, image_layout=layout)
    dloss, = torch.autograd.grad(total, xi)
    assert total.dim() == 0 and dloss.shape == xi.shape
    for v in stats.values():
        assert v.dim() == 0 and v.is_cuda and not v.requires_grad
    assert bits_equal(stats["ssim"], s)
    return {"ssim": s.item(), "l1": stats["l1"].item(), "psnr": stats["psnr"].item(), "loss": total.item(),
            "dssim": dssim.cpu().numpy(), "dloss": dloss.cpu().numpy()}


LARGE = {"tiles_135x240": (3, 135, 240), "rows_16x4099": (3, 16, 4099)}
_LARGE_CACHE: dict = {}


def large_case(name):
    """(img, gt, f64 restatement) of a shape too large to commit, computed once and never modified."""
    if name not in _LARGE_CACHE:
        rng = np.random.default_rng(sorted(LARGE).index(name) + 7)
        img = rng.random(LARGE[name], dtype=np.float32)
        gt = np.clip(img + np.float32(0.1) * rng.standard_normal(LARGE[name], dtype=np.float32), 0, 1)
        ref = restate(img, gt)
        for a in (img, gt, ref["dssim"], ref["dloss"]):
            a.setflags(write=False)
        _LARGE_CACHE[name] = (img, gt, ref)
    return _LARGE_CACHE[name]


def hip_distances(golden):
    """{case: {quantity: distance to f64}} over every case of this file (also what DESIGN 2g tabulates)."""
    out = {}
    for name in single_cases(golden):
        got, ref = hip_single(golden[f"{name}/img"], golden[f"{name}/gt"]), fixture64(golden, name)
        out[name] = {q: distance(q, got[q], ref[q]) for q in VALUES + GRADS}
    for name in LARGE:
        img, gt, ref = large_case(name)
        got = hip_single(img, gt)
        out[name] = {q: distance(q, got[q], ref[q]) for q in VALUES + GRADS}
    out["batch"] = hip_batch(golden)
    return out


def hip_batch(golden):
    """The batched case: ssim with size_average True and False (upstream weights 1, 2 per image)."""
    from relightable3dgaussian_amd import loss

    x, y = _cuda(golden["batch/img"], True), _cuda(golden["batch/gt"])
    per = loss.ssim(x, y, size_average=False)
    assert per.shape == (2,)
    g_per, = torch.autograd.grad((per * torch.tensor([1.0, 2.0], device="cuda")).sum(), x)
    mean = loss.ssim(x, y)
    g_mean, = torch.autograd.grad(mean, x)
    flat = lambda a: np.asarray(a).reshape(6, 12, 18)
    return {"ssim": max(distance("ssim", per.detach().cpu().numpy(), golden["batch/f64/ssim_b"]),
                        distance("ssim", mean.item(), golden["batch/f64/ssim"])),
            "dssim": max(distance("dssim", flat(g_per.cpu().numpy()), flat(golden["batch/f64/dssim_b"])),
                         distance("dssim", flat(g_mean.cpu().numpy()), flat(golden["batch/f64/dssim"])))}


FIXTURE_CASES = ["c3_1x1", "c3_5x7", "c1_11x11", "c3_16x16", "c3_17x15", "c4_16x33", "c3_37x53", "c3_64x48",
                 "half_equal", "constant"]


def test_fixture_case_list_is_complete(golden):
    assert FIXTURE_CASES + ["batch"] == list(golden["names"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_fixture_cases(hip_ext, golden, name):
    got, ref = hip_single(golden[f"{name}/img"], golden[f"{name}/gt"]), fixture64(golden, name)
    d = {q: distance(q, got[q], ref[q]) for q in VALUES + GRADS}
    print(name, d)
    for q in d:
        assert d[q] <= BARS[q], (name, q, d[q], BARS[q])
    if name == "half_equal":  # sign(0) = 0: on the identical half only the SSIM term is left
        x, y = golden[f"{name}/img"], golden[f"{name}/gt"]
        assert (x[:, :, :10] == y[:, :, :10]).all()
        assert np.abs(got["dloss"][:, :, :10] - LAMBDA * -got["dssim"][:, :, :10]).max() <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LARGE))
def test_larger_shapes(hip_ext, name):
    """135x240: 9 x 15 tiles per plane, partial on the lower edge; 16x4099: one row of 257 tiles, one more
    than the finishing kernel has threads, so its strided loop takes a second round."""
    img, gt, ref = large_case(name)
    got = hip_single(img, gt)
    d = {q: distance(q, got[q], ref[q]) for q in VALUES + GRADS}
    print(name, d)
    for q in d:
        assert d[q] <= BARS[q], (name, q, d[q], BARS[q])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c3_37x53", "c4_16x33", "half_equal"])
def test_hwc_layout_is_bitwise_chw(hip_ext, golden, name):
    img, gt = golden[f"{name}/img"], golden[f"{name}/gt"]
    chw, hwc = hip_single(img, gt), hip_single(img, gt, layout="hwc")
    assert hwc["dloss"].shape == img.shape[1:] + img.shape[:1]
    for q in VALUES:
        assert np.float32(chw[q]).tobytes() == np.float32(hwc[q]).tobytes(), q
    assert bits_equal(hwc["dloss"].transpose(2, 0, 1), chw["dloss"])


@pytest.mark.gpu
def test_repeatable_bit_for_bit(hip_ext, golden):
    img, gt = large_case("tiles_135x240")[:2]
    a, b = hip_single(img, gt), hip_single(img, gt)
    for q in VALUES:
        assert np.float32(a[q]).tobytes() == np.float32(b[q]).tobytes(), q
    for q in GRADS:
        assert bits_equal(a[q], b[q]), q
    x, y = _cuda(img), _cuda(gt)
    (s1, d1), (s2, d2) = hip_ext.image_loss_forward(x, y, False, True), hip_ext.image_loss_forward(x, y, False, True)
    assert bits_equal(s1, s2) and bits_equal(d1, d2)


@pytest.mark.gpu
def test_upstream_scalar_is_read_on_the_device(hip_ext, golden):
    """(loss * 3.5).backward(): 3.5 x the gradient, within 1 ulp of each element."""
    from relightable3dgaussian_amd import loss

    y = _cuda(golden["c3_37x53/gt"])
    grads = []
    for k in (None, 3.5):
        x = _cuda(golden["c3_37x53/img"], True)
        total, _ = loss.l1_ssim_loss(x, y, LAMBDA)
        (total if k is None else total * k).backward()
        grads.append(x.grad.cpu().numpy())
        x = _cuda(golden["c3_37x53/img"], True)
        s = loss.ssim(x, y)
        (s if k is None else s * k).backward()
        grads.append(x.grad.cpu().numpy())
    for g1, g35 in ((grads[0], grads[2]), (grads[1], grads[3])):
        want = g1.astype(np.float64) * 3.5
        ulps = np.abs(g35.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        print("max ulps", ulps.max())
        assert np.abs(g1).max() > 0 and ulps.max() <= 1.0


@pytest.mark.gpu
def test_size_average_false(hip_ext, golden):
    from relightable3dgaussian_amd import loss

    d = hip_batch(golden)
    print("batch", d)
    for q in d:
        assert d[q] <= BARS[q], (q, d[q], BARS[q])
    x, y = _cuda(golden["batch/img"]), _cuda(golden["batch/gt"])
    per = loss.ssim(x, y, size_average=False)
    for b in range(2):  # the per-image values
        assert abs(loss.ssim(x[b], y[b]).item() - per[b].item()) <= BARS["ssim"]


@pytest.mark.gpu
def test_no_grad_writes_only_the_sums(hip_ext, golden):
    from relightable3dgaussian_amd import loss

    x, y = _cuda(golden["c3_37x53/img"], True), _cuda(golden["c3_37x53/gt"])
    sums, dmaps = hip_ext.image_loss_forward(x.detach(), y, False, True)
    sums0, none = hip_ext.image_loss_forward(x.detach(), y, False, False)
    assert dmaps.shape == (3, 3, 37, 53) and none.numel() == 0 and bits_equal(sums, sums0)
    with torch.no_grad():
        quiet = loss.ssim(x, y)
        total, stats = loss.l1_ssim_loss(x, y, LAMBDA)
    assert not quiet.requires_grad and not total.requires_grad
    assert bits_equal(quiet, loss.ssim(x, y)) and bits_equal(total, loss.l1_ssim_loss(x, y, LAMBDA)[0])


@pytest.mark.gpu
def test_other_stream(hip_ext, golden):
    img, gt = golden["c3_64x48/img"], golden["c3_64x48/gt"]
    base = hip_single(img, gt)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = hip_single(img, gt)
    s.synchronize()
    for q in VALUES:
        assert np.float32(base[q]).tobytes() == np.float32(other[q]).tobytes(), q
    for q in GRADS:
        assert bits_equal(base[q], other[q]), q


@pytest.mark.gpu
def test_non_contiguous_image(hip_ext, golden):
    from relightable3dgaussian_amd import loss

    img, y = golden["c3_37x53/img"], _cuda(golden["c3_37x53/gt"])
    wide = torch.zeros((3, 37, 54), device="cuda")
    wide[:, :, 1:] = _cuda(img)
    out = []
    for x in (wide[:, :, 1:], wide[:, :, 1:].contiguous()):
        x = x.detach().requires_grad_(True)
        total, stats = loss.l1_ssim_loss(x, y, LAMBDA)
        g, = torch.autograd.grad(total, x)
        out.append((total, stats["psnr"], g))
    assert not wide[:, :, 1:].is_contiguous() and out[0][2].shape == (3, 37, 53)
    for a, b in zip(*out):
        assert bits_equal(a, b)


@pytest.mark.gpu
def test_raw_c_abi(hip_ext, lib, golden):
    """Both entry points through ctypes on device pointers (HWC strides for img), scratch from a
    torch-backed callback: bitwise what the binding returns."""
    C, H, W = 3, 37, 53
    x = _cuda(golden["c3_37x53/img"]).permute(1, 2, 0).contiguous()
    y = _cuda(golden["c3_37x53/gt"])
    ws, wa, sc = (torch.full((C,), v, device="cuda") for v in (-0.25, 0.5, 3.0))
    sums_ref, dmaps_ref = hip_ext.image_loss_forward(x, y, True, True)
    grad_ref = hip_ext.image_loss_backward(x, y, True, dmaps_ref, ws, wa, sc)
    grad_ref1 = hip_ext.image_loss_backward(x, y, True, dmaps_ref, ws, wa)
    keep = []

    @ALLOC
    def torch_alloc(ctx, nbytes):
        t = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        keep.append(t)
        return t.data_ptr()

    sums, dmaps = torch.empty((C, 3), device="cuda"), torch.empty((3, C, H, W), device="cuda")
    grad, grad1 = torch.empty_like(x), torch.empty_like(x)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    image = (C, H, W, x.data_ptr(), 1, W * C, C, y.data_ptr(), H * W, W, 1)
    rc = lib.r3dg_image_loss_forward(*image, sums.data_ptr(), dmaps.data_ptr(), torch_alloc, None, stream)
    assert rc == 0, lib.r3dg_last_error()
    rc = lib.r3dg_image_loss_backward(*image, dmaps.data_ptr(), ws.data_ptr(), wa.data_ptr(), sc.data_ptr(),
                                      grad.data_ptr(), stream)
    assert rc == 0, lib.r3dg_last_error()
    rc = lib.r3dg_image_loss_backward(*image, dmaps.data_ptr(), ws.data_ptr(), wa.data_ptr(), None,
                                      grad1.data_ptr(), stream)
    assert rc == 0, lib.r3dg_last_error()
    torch.cuda.synchronize()
    assert len(keep) == 1 and keep[0].numel() >= 12 * C * 3 * 4  # 3 x 4 tiles per plane
    assert bits_equal(sums, sums_ref) and bits_equal(dmaps, dmaps_ref)
    assert bits_equal(grad, grad_ref) and bits_equal(grad1, grad_ref1)
    assert bits_equal(grad, grad1 * 3.0)  # scale multiplies last
