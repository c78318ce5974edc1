"""Pins the reference the depth / alpha gradient tests use (tests/depth_ref.py), on the CPU: a render
with colours [z_i, 1, 0] over a zero background carries the depth map in channel 0 and the
accumulated alpha 1 - T_final in channel 1, and the oracle's backward of that run equals float64
autograd of its own forward.  It pins the reference, not the feature."""
import numpy as np
import pytest

from oracle import torch_ref
from tests.common import make_scene, oracle_run, rel_l1
from tests.depth_ref import trick_scene

CASES = {
    "sh3": dict(P=250, W=48, H=40, sh_degree=3),
    "bg_mod": dict(P=200, W=40, H=32, sh_degree=2, bg=(1.0, 0.5, 0.25), scale_modifier=0.8),
}


@pytest.mark.parametrize("case", list(CASES))
def test_trick_run_is_depth_and_alpha_and_its_backward_equals_autograd(oracle, case):
    inp, st = make_scene(**CASES[case])
    H, W = st["image_height"], st["image_width"]
    col = oracle_run(oracle, inp, st, nthreads=1)
    internals = col["state"].internals()
    inp2, st2 = trick_scene(inp, st, internals["depths"])
    rng = np.random.default_rng(5)
    dtrick = np.zeros((3, H, W), np.float32)
    dtrick[:2] = rng.standard_normal((2, H, W)).astype(np.float32)
    tr = oracle_run(oracle, inp2, st2, dL_dpix=dtrick, nthreads=1)
    assert np.array_equal(tr["radii"], col["radii"])
    e0 = rel_l1(tr["color"][0], col["depth"][0])
    e1 = rel_l1(tr["color"][1], 1.0 - internals["final_T"])
    print(f"{case}: channel 0 vs depth {e0:.3e}, channel 1 vs 1 - final_T {e1:.3e}")
    assert e0 < 1e-5 and e1 < 1e-5
    assert np.abs(tr["color"][2]).max() == 0.0

    lists = tr["state"].blend_lists()
    stn = {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in st2.items()}
    ag = torch_ref.render_autograd(stn, {k: v.numpy() for k, v in inp2.items()}, lists, tr["radii"] > 0, dtrick)
    assert rel_l1(tr["color"], ag["image"]) < 1e-5
    vis = tr["radii"] > 0
    checked = 0
    for k in ag:
        if k == "image":
            continue
        a, b = tr["grads"][k], ag[k]
        if k == "dL_dcov3D":  # written for visible Gaussians only
            a, b = a[vis], b[vis]
        if np.abs(b).sum() == 0:
            assert np.abs(a).max() < 1e-9, k
            continue
        r = rel_l1(a, b)
        print(f"{case}: {k} oracle vs autograd {r:.3e}")
        assert r < 1e-4, f"{k}: rel L1 {r:.3e}"
        checked += 1
    assert checked >= 6
