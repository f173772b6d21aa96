"""bench.py's plain run and `--dump-outputs`: the result line of a plain run carries the headline
figure alone (what `--full` measures is absent), `--steps` is the number of timed steps, and the
dumped arrays are what the last timed step returned -- float32, under 64 MB in all, the same from
run to run where the kernels are order-independent (the forward images). Run in process on a small
P (the frame stays 1920x1080, so the images are sampled as at M1)."""
import json
import os
import sys

import numpy as np
import pytest


def _bench(monkeypatch, capsys, *argv):
    import bench  # the repository root is on sys.path (conftest.py)

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--P", "20000", *argv])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return bench, json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_last_step_outputs(hip_ext, monkeypatch, capsys, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench, d = _bench(monkeypatch, capsys, "--steps", "3", "--warmup", "1", "--dump-outputs", a)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["dtype"] == "f32"
    assert d["unit"] == "Mpix/s" and d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert abs(d["value"] - 1920 * 1080 / d["ms_per_step"] / 1e3) < 1e-3 * d["value"]
    for k in ("roofline", "kernel_ms", "bvh_visibility", "cpu_baseline", "brdf_cpu_baseline", "exchange"):
        assert k not in d, k
    _, d2 = _bench(monkeypatch, capsys, "--steps", "1", "--warmup", "0", "--dump-outputs", b)
    assert d2["steps"] == 1 and d2["config"]["num_rendered"] == d["config"]["num_rendered"]

    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b))
    names = {f[:-4] for f in files}
    assert {"num_rendered", "n_contrib", "color", "opacity", "depth", "feature", "normal", "surface_xyz", "radii",
            "dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dfeatures", "dL_dsh", "dL_dscales",
            "dL_drotations"} <= names
    assert names <= set(bench.FWD_NAMES) | set(bench.BWD_NAMES)
    total = 0
    for f in files:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype == np.float32 and x.shape == y.shape and 0 < x.size <= bench.DUMP_CAP, f
        assert np.isfinite(x).all(), f
        total += x.nbytes
        if f[:-4] in bench.FWD_NAMES:
            # same inputs, order-independent forward: bit-identical between runs
            assert np.array_equal(x, y), f
        else:
            # the backward's atomic f32 sums run in another order each time: n terms reordered move a
            # sum by at most n * 2^-24 of the terms' magnitudes, 6e-5 at n = 1000 pixels per Gaussian
            np.testing.assert_allclose(x, y, rtol=0, atol=1e-4 * float(np.abs(x).max()), err_msg=f)
    assert total <= 64 << 20
    assert int(np.load(os.path.join(a, "num_rendered.npy"))[0]) == d["config"]["num_rendered"]
    assert np.load(os.path.join(a, "color.npy")).std() > 0 and np.abs(np.load(os.path.join(a, "dL_dsh.npy"))).max() > 0
