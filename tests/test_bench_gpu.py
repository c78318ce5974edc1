"""bench.py's output contract on a real GPU, at a small size: the driver parses exactly ONE JSON line
from stdout (native libraries' banners must not reach it), with the metric / value / unit / roofline
/ cpu_baseline fields the contract names, for the single-GPU step and the forced exchange path
(the N > 1 code path at world 1, whose RCCL initialisation prints a version banner)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--points", "20000", "--width", "320", "--height", "240", "--views", "16", "--steps", "3", "--warmup", "2",
         "--sync-loss-steps", "2", "--fwd-frames", "2", "--no-cpu-baseline"]


def _run(args):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=280, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


PARAMS = ("xyz", "features_dc", "features_rest", "opacity", "scaling")
DUMPED = {"rows", "step_info", *PARAMS, *(f"{p}_{m}" for p in PARAMS for m in ("exp_avg", "exp_avg_sq"))}


def _load(path):
    import numpy as np

    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


@pytest.mark.parametrize("extra", [[], ["--force-dist"]])
def test_bench_prints_one_json_line(extra, tmp_path):
    # started before this process touches the GPU (conftest.py runs this module first; no `gpu`
    # fixture here: torch.cuda.is_available() would initialise it, device_count() does not)
    import torch

    if torch.cuda.device_count() == 0:
        pytest.skip("no HIP device")
    line = _run(SMALL + ["--full", "--dump-outputs", str(tmp_path / "out")] + extra)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 2
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] - 1000.0) < 0.05 * 1000.0
    assert line["roofline"]["unit"] == "GB/s" and line["roofline"]["achieved"] > 0
    assert ("RCCL" in line["config"]["parallelism"]) == bool(extra)
    # the dump's two steps also run beside the --full legs and through the forced exchange path
    arrays = _load(tmp_path / "out")
    assert set(arrays) == DUMPED and arrays["xyz_exp_avg_sq"].max() > 0


def test_plain_run_prints_headline_and_dumps_outputs(tmp_path):
    """Without --full: the headline fields only.  --dump-outputs writes the results of two further
    steps from the seeded starting model (sampled parameter rows, their Adam moments, the step info)
    as float .npy files; the rows have moved from their seeded start by no more than Adam's two
    steps; and a second run with the same arguments writes the same arrays."""
    import numpy as np
    import torch

    from rain_amd import synthetic

    if torch.cuda.device_count() == 0:
        pytest.skip("no HIP device")
    line = _run(SMALL + ["--dump-outputs", str(tmp_path / "a")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup"):
        assert k in line, k
    for k in ("roofline", "cpu_baseline", "kernels", "api_iters_per_s", "forward_mpix_per_s"):
        assert k not in line, k
    assert line["steps"] == 3 and line["config"]["iterations"] == [1001, 1003]
    assert abs(line["value"] * line["ms_per_step"] - 1000.0) < 0.05 * 1000.0
    arrays = _load(tmp_path / "a")
    assert set(arrays) == DUMPED
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    n = len(arrays["rows"])
    assert n == min(arrays["step_info"][3], 16384) == 16384 and arrays["step_info"][0] == 1002
    assert arrays["xyz"].shape == (n, 3) and arrays["features_rest"].shape == (n, 15, 3)
    assert arrays["xyz_exp_avg_sq"].shape == (n, 3) and arrays["xyz_exp_avg_sq"].max() > 0
    # Adam from zero moments: step 1 moves a coordinate by lr, step 2 by lr |m^| / sqrt(v^) <= 1.001 lr
    # (Cauchy-Schwarz on m^ = (0.09 g1 + 0.1 g2) / 0.19, v^ ~ (g1^2 + g2^2) / 2); lr <= 1.6e-4 x extent 4.4
    start = synthetic.random_gaussians(20000, sh_degree=3, seed=0, bench=True)["xyz"].numpy()
    moved = np.abs(arrays["xyz"] - start[arrays["rows"].astype(np.int64)])
    print("max |xyz - start|", moved.max(), "moved rows", int((moved.max(axis=1) > 0).sum()))
    assert 0 < moved.max() <= 2.01 * 1.6e-4 * 4.4 and (moved.max(axis=1) > 0).mean() > 0.1
    # same arguments, same outputs: the steps differ between runs only in the order of the blend
    # backward's float32 atomic adds (2^-24 per add over the hundreds of pixels of a splat): relative
    # L1 1e-5 per array, which a rare sign change of a near-zero first gradient (2 lr on one element
    # of a parameter array) does not reach
    _run(SMALL + ["--dump-outputs", str(tmp_path / "b")])
    again = _load(tmp_path / "b")
    assert set(again) == DUMPED
    for k in sorted(DUMPED):
        x, y = arrays[k].astype(np.float64), again[k].astype(np.float64)
        rel = np.abs(x - y).sum() / np.abs(x).sum()
        print(f"{k}: run-to-run relative L1 {rel:.2e}")
    for k in sorted(DUMPED):
        x, y = arrays[k].astype(np.float64), again[k].astype(np.float64)
        assert x.shape == y.shape and np.abs(x - y).sum() <= 1e-5 * np.abs(x).sum(), k
