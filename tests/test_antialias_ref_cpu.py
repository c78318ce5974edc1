"""The anti-aliasing reference (tests/antialias_ref.py) on the CPU: the factor's graph against finite
differences, its exact values at low_pass = 0, its range, the clamp, and the conditions the GPU tests'
scenes must meet so that none of them can pass on nothing."""
import numpy as np
import pytest
import torch

from tests import antialias_ref as AR
from tests.common import GRAD_NAMES, oracle_run, rel_l1

_REF = {}


def _reference(oracle, name):
    """Per scene, computed once and left unchanged."""
    if name not in _REF:
        inp, st = AR.scene(name)
        H, W = st["image_height"], st["image_width"]
        dpix = np.random.default_rng(11).standard_normal((3, H, W)).astype(np.float32)
        _REF[name] = (inp, st, AR.reference(oracle, inp, st, dpix))
    return _REF[name]


def _visible_rows(oracle, inp, st, n):
    radii = oracle_run(oracle, inp, st)["radii"]
    return np.flatnonzero(radii > 0)[:n]


def test_comp_gradcheck(oracle):
    inp, st = AR.scene("small_sh3")
    rows = _visible_rows(oracle, inp, st, 50)
    assert len(rows) == 50
    m, s, q = (inp[k][rows].to(torch.float64).clone().requires_grad_(True) for k in ("means3D", "scales", "rotations"))

    def f(m, s, q):
        return AR.comp(st, dict(means3D=m, scales=s, rotations=q))[0]

    c = f(m, s, q).detach()
    assert float(c.min()) > 0.005 and float(c.max()) < 1.0  # none at the clamp: the graph is smooth here
    assert torch.autograd.gradcheck(f, (m, s, q), eps=1e-6, atol=1e-7, rtol=1e-5)
    # and through a precomputed covariance
    inp_p, st_p = AR.scene("small_precomp")
    rows = _visible_rows(oracle, inp_p, st_p, 50)
    m, cov = (inp_p[k][rows].to(torch.float64).clone().requires_grad_(True) for k in ("means3D", "cov3D_precomp"))
    assert torch.autograd.gradcheck(lambda m, cov: AR.comp(st_p, dict(means3D=m, cov3D_precomp=cov))[0], (m, cov),
                                    eps=1e-7, atol=1e-6, rtol=1e-4)


def test_comp_is_one_without_dilation(oracle):
    inp, st = AR.scene("small_sh3")
    st = dict(st, low_pass=0.0)
    rows = _visible_rows(oracle, inp, dict(st, low_pass=0.3), 500)
    leaf, withleaf = AR.leaves({k: v[rows] for k, v in inp.items()})
    c, rho = AR.comp(st, withleaf)
    assert torch.equal(c, torch.ones_like(c)) and torch.equal(rho, torch.ones_like(rho))
    for g in torch.autograd.grad(c.sum(), list(leaf.values())):
        assert float(g.abs().max()) == 0.0


@pytest.mark.parametrize("name", list(AR.SCENES) + list(AR.THIN))
def test_comp_range_and_clamp(oracle, name):
    inp, st, ref = _reference(oracle, name)
    vis = ref["radii"] > 0
    c, rho = ref["comp"][vis], ref["rho"][vis]
    assert c.min() >= 0.005 and c.max() <= 1.0 and (rho > 0).all() and (rho < 1).all()
    assert np.array_equal(c == 0.005, rho <= AR.RHO_MIN)
    # a clamped row's factor is a constant: the factor's term gives it exact zeros
    clamped = np.zeros(len(vis), bool)
    clamped[vis] = rho <= AR.RHO_MIN
    term = AR.comp_term(st, inp, np.ones(len(vis)))
    for k, v in term.items():
        assert np.abs(v[clamped]).sum() == 0.0, k
        if clamped.any() and k != "dL_drotations":
            assert np.abs(v[vis & ~clamped]).sum() > 0.0, k


@pytest.mark.parametrize("name", AR.SMALL)
def test_scene_conditions(oracle, name):
    """What the GPU tests rely on, on the reference alone."""
    inp, st, ref = _reference(oracle, name)
    vis = ref["radii"] > 0
    nz = ref["g_o"] != 0
    frac = (nz & vis).sum() / vis.sum()
    med = float(np.median(ref["comp"][vis]))
    ncon = int(ref["state"].internals()["n_contrib"].max())
    print(f"{name}: visible {vis.sum()}, non-zero g_o {(nz & vis).sum()} ({frac:.3f}), median comp {med:.3f}, "
          f"max n_contrib {ncon}")
    assert not (nz & ~vis).any()
    assert frac >= 0.6
    assert med < 0.7
    assert ncon > 64  # more than one 64-pair round
    if name in AR.THIN:
        clamped = vis & (ref["rho"] <= AR.RHO_MIN)
        print(f"{name}: clamped visible {clamped.sum()}, with non-zero g_o {(clamped & nz).sum()}")
        assert (clamped & nz).sum() >= 20
        low = AR.below_visibility(name, inp) & clamped  # o comp = 0.0025 < 1/255: radius kept, nothing blended
        assert low.sum() >= 3
        o_eff = ref["inp_comp"]["opacities"].numpy().reshape(-1)
        assert (o_eff[low] < 1.0 / 255.0).all() and (o_eff[clamped & ~low] >= 1.0 / 255.0).all()
        for k in GRAD_NAMES:
            if ref["grads"][k].size:
                assert np.abs(ref["grads"][k][low]).sum() == 0.0, k


def test_reference_is_the_plain_run_where_the_factor_is_one(oracle):
    """low_pass = 0: the anti-aliased reference is the oracle's plain run (the images bit for bit; the
    gradients up to the order of the oracle's own threaded sums)."""
    inp, st = AR.scene("small_sh3")
    st = dict(st, low_pass=0.0)
    dpix = np.random.default_rng(11).standard_normal((3, st["image_height"], st["image_width"])).astype(np.float32)
    ref = AR.reference(oracle, inp, st, dpix)
    plain = oracle_run(oracle, inp, st, dL_dpix=dpix)
    assert np.array_equal(ref["color"], plain["color"]) and np.array_equal(ref["radii"], plain["radii"])
    for k in GRAD_NAMES:
        assert rel_l1(ref["grads"][k], plain["grads"][k]) <= 1e-6, k


def test_reference_changes_the_small_scene(oracle):
    """The issue's probe: the small-splat scene's image mean drops from 0.174 to 0.110."""
    inp, st, ref = _reference(oracle, "small_sh3")
    plain = oracle_run(oracle, inp, st)
    assert abs(float(plain["color"].mean()) - 0.174) < 2e-3
    assert abs(float(ref["color"].mean()) - 0.110) < 2e-3
