"""The float64 reference of the absolute-gradient statistics (tests/absgrad_ref.py) against the CPU oracle:
its signed sums are the oracle's dL_dmeans2D, which pins the walk whose magnitudes the GPU tests compare
against (tests/test_absgrad_gpu.py)."""
import numpy as np
import pytest

from tests import absgrad_ref as AR
from tests.common import rel_l1

_REF = {}


def _reference(oracle, name):
    if name not in _REF:
        inp, st, dpix = AR.scene(name)
        _REF[name] = AR.reference(oracle, inp, st, dpix)
    return _REF[name]


@pytest.mark.parametrize("name", ["sh3", "ragged_bg", "large"])
def test_signed_sums_are_the_oracles(oracle, name):
    ref = _reference(oracle, name)
    want = np.asarray(ref["grads"]["dL_dmeans2D"], np.float64)
    err = rel_l1(ref["signed"], want[:, :2])
    print(f"{name}: signed sums vs oracle, relative L1 {err:.3g}")
    assert err <= 1e-4
    assert np.all(want[:, 2] == 0)


@pytest.mark.parametrize("name", ["sh3", "ragged_bg", "large"])
def test_abs_bounds_signed_and_hidden_rows_are_zero(oracle, name):
    ref = _reference(oracle, name)
    s, a = ref["signed"], ref["abs"]
    assert np.all(a >= 0)
    assert np.all(a >= np.abs(s) - 1e-9 * a)  # |sum| <= sum |.|, up to the rounding of two float64 sums
    hidden = np.asarray(ref["radii"]) <= 0
    assert hidden.any() or name == "large"  # (every Gaussian of the small frame is visible)
    assert np.all(a[hidden] == 0) and np.all(s[hidden] == 0)
    got = np.abs(s).sum(axis=1) > 0
    ratio = np.linalg.norm(a[got], axis=1) / np.linalg.norm(s[got], axis=1)
    print(f"{name}: {int(got.sum())} Gaussians with gradient, median |abs| / |signed| = {np.median(ratio):.3g}")
    assert np.median(ratio) > 1.0  # the scenes do exercise cancellation


def test_single_centred_gaussian(oracle):
    """One isotropic Gaussian exactly on a pixel centre, black background, dL_dpix = 1: every pixel's pull has
    a mirror pixel with the opposite pull, so the signed sums vanish while the absolute ones do not."""
    inp, st, dpix = AR.single_gaussian()
    ref = AR.reference(oracle, inp, st, dpix)
    xy = ref["state"].internals()["xy"][0]
    assert xy[0] == (st["image_width"] - 1) / 2 and xy[1] == (st["image_height"] - 1) / 2
    assert ref["radii"][0] > 0
    s, a = ref["signed"][0], ref["abs"][0]
    print(f"single Gaussian: signed {s}, abs {a}")
    assert np.all(a > 0)
    assert np.all(np.abs(s) <= 1e-6 * a)
    # the oracle's own float32 signed sums cancel as well
    assert np.all(np.abs(np.asarray(ref["grads"]["dL_dmeans2D"])[0, :2]) <= 1e-3 * a)
