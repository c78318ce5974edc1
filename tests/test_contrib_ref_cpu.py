"""Pins the reference the contribution-statistics tests use (tests/contrib_ref.py), on the CPU, against
the oracle alone: the numpy walk's sum_gw and sum_w equal channels 0 and 1 of the oracle's dL_dcolors for
dL_dpix = (g, 1, 0) on precomputed colours, and its total weight equals the image's accumulated alpha.
Bar: 1e-5 relative L1, the project's bar between float evaluations of the same sums.  It pins the
reference, not the feature."""
import numpy as np
import pytest

from tests.common import make_scene, rel_l1
from tests.contrib_ref import contributions_ref, oracle_sums

CASES = {
    "sh3": dict(P=250, W=48, H=40, sh_degree=3),
    "ragged_bg": dict(P=300, W=50, H=37, sh_degree=1, bg=(1.0, 0.5, 0.25), scale_modifier=0.8),
    "dense": dict(P=1200, W=40, H=32, sh_degree=0),  # pixels that saturate: n_contrib cuts the walk
}


@pytest.mark.parametrize("case", list(CASES))
def test_walk_equals_the_oracles_colour_gradient_and_alpha(oracle, case):
    inp, st = make_scene(**CASES[case])
    H, W = st["image_height"], st["image_width"]
    g = np.random.default_rng(3).standard_normal((H, W)).astype(np.float32)  # both signs
    sum_gw, sum_w, run = oracle_sums(oracle, inp, st, g, nthreads=1)
    internals = run["state"].internals()
    ref = contributions_ref(internals, W, H, g)
    e_w, e_gw = rel_l1(ref["sum_w"], sum_w), rel_l1(ref["sum_gw"], sum_gw)
    alpha_total = float((1.0 - internals["final_T"].astype(np.float64)).sum())
    e_a = abs(ref["sum_w"].sum() - alpha_total) / alpha_total
    print(f"{case}: sum_w {e_w:.3e}, sum_gw {e_gw:.3e}, total weight vs sum(1 - final_T) {e_a:.3e}")
    assert e_w < 1e-5 and e_gw < 1e-5 and e_a < 1e-5
    # no map: g == 1, sum_gw is sum_w
    one = contributions_ref(internals, W, H)
    assert np.array_equal(one["sum_gw"], one["sum_w"]) and np.array_equal(one["sum_w"], ref["sum_w"])
    # invisible Gaussians get nothing; weights and counts are consistent
    vis = run["radii"] > 0
    for k in ("sum_w", "sum_gw", "max_w", "count"):
        assert not np.any(ref[k][~vis]), k
    hit = ref["count"] > 0
    assert np.array_equal(hit, ref["sum_w"] > 0) and np.array_equal(hit, ref["max_w"] > 0)
    assert np.all(ref["max_w"] <= ref["sum_w"] * (1 + 1e-12)) and ref["max_w"].max() <= 0.99
    assert np.all(ref["sum_w"][hit] <= ref["count"][hit] * ref["max_w"][hit] * (1 + 1e-12))
