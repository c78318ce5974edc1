"""The MCMC reference (tests/mcmc_ref.py) against closed forms, and rain_amd.mcmc.relocation_values (torch
float64) against the reference."""
import math

import numpy as np
import pytest
import torch

from rain_amd import mcmc
from tests import mcmc_ref as R

OPACITIES = [0.005, 0.01, 0.1, 0.3, 0.5, 0.9, 0.999, 1.0 - 1.2e-7]


def test_one_copy_is_exact():
    for o in OPACITIES:
        assert R.relocation(o, 1) == (o, o, 1.0)
    g = {"opacity": (np.array([[0.3], [-2.0], [1.0]]), None, None), "scaling": (np.zeros((3, 3)), None, None)}
    out, counts = R.relocate(g, [], [], 0.005)
    assert counts.tolist() == [0, 0, 0]
    assert np.array_equal(out["opacity"][0], g["opacity"][0]) and np.array_equal(out["scaling"][0], g["scaling"][0])


def test_two_copies_closed_form():
    for o in OPACITIES:
        on, D, coeff = R.relocation(o, 2)
        assert on == pytest.approx(1.0 - math.sqrt(1.0 - o), rel=1e-13, abs=0)
        assert D == pytest.approx(2.0 * on - on * on / math.sqrt(2.0), rel=1e-13)
        assert coeff == pytest.approx(o / D, rel=1e-15)


def test_copies_compose_to_the_source_opacity():
    for o in OPACITIES:
        for N in (2, 3, 7, 20, 51):
            on, _D, _c = R.relocation(o, N)
            assert 1.0 - (1.0 - on) ** N == pytest.approx(o, rel=1e-12)


def test_coeff_in_unit_interval_and_decreasing_in_copies():
    for o in OPACITIES:
        coeffs = [R.relocation(o, N)[2] for N in range(1, R.N_MAX + 1)]
        assert all(0.0 < c <= 1.0 for c in coeffs)
        assert all(b < a for a, b in zip(coeffs, coeffs[1:])), o


def test_counts_above_fifty_behave_as_fifty_one():
    for o in (0.01, 0.5, 0.999):
        assert R.relocation(o, 52) == R.relocation(o, 51) == R.relocation(o, 1000)
    raw = np.array([[0.4], [-6.0]])
    g = {"opacity": (raw, np.ones((2, 1)), np.ones((2, 1))), "scaling": (np.zeros((2, 3)), None, None)}
    # (the reference does not enforce the distinct-destination precondition: only the counts matter here)
    out60, c60 = R.relocate(g, [0] * 60, [1] * 60, 0.005)
    out50, c50 = R.relocate(g, [0] * 50, [1] * 50, 0.005)
    assert c60[0] == 60 and c50[0] == 50
    assert np.array_equal(out60["opacity"][0], out50["opacity"][0])
    assert np.array_equal(out60["scaling"][0], out50["scaling"][0])
    assert np.all(out60["opacity"][1] == 0.0) and np.all(out60["opacity"][2] == 0.0)  # moments cleared


def test_sum_over_rows_first_is_the_same_sum():
    """sum_{a=k+1..N} C(a-1, k) = C(N, k+1): the kernel sums D over a first (rain_amd/csrc/mcmc.hip)."""
    for o in OPACITIES:
        for N in (2, 5, 51):
            on, D, _c = R.relocation(o, N)
            D1 = sum(math.comb(N, k + 1) * (-1.0) ** k * on ** (k + 1) / math.sqrt(k + 1) for k in range(N))
            assert D1 == pytest.approx(D, rel=1e-10)


def test_clamp_and_cleared_moments_in_the_reference():
    raw = np.array([[-5.0], [3.0], [0.0], [-8.0]])  # sigmoid(-5) = 0.0067: its copies fall below min_opacity
    sc = np.arange(12, dtype=np.float64).reshape(4, 3)
    g = {"opacity": (raw, np.ones((4, 1)), np.ones((4, 1))), "scaling": (sc, np.ones((4, 3)), np.ones((4, 3))),
         "xyz": (np.arange(12, dtype=np.float64).reshape(4, 3) + 100.0, np.ones((4, 3)), np.ones((4, 3)))}
    out, counts = R.relocate(g, [0, 7, -1], [3, 2, 1], 0.005)  # the last two pairs are out of range: skipped
    assert counts.tolist() == [1, 0, 0, 0]
    lo = float(np.float32(0.005))
    assert R.sigmoid(out["opacity"][0][0, 0]) == pytest.approx(lo, rel=1e-12)  # clamped
    assert out["opacity"][0][3, 0] == out["opacity"][0][0, 0]
    _on, _D, coeff = R.relocation(R.sigmoid(-5.0), 2)
    assert np.allclose(out["scaling"][0][3], sc[0] + math.log(coeff), rtol=1e-15)
    assert np.array_equal(out["scaling"][0][3], out["scaling"][0][0])
    assert np.array_equal(out["xyz"][0][3], g["xyz"][0][0]) and np.array_equal(out["xyz"][0][0], g["xyz"][0][0])
    for k in g:
        for mom in out[k][1:]:
            assert np.all(mom[[0, 3]] == 0.0) and np.all(mom[[1, 2]] == 1.0)
        assert np.array_equal(out[k][0][[1, 2]], g[k][0][[1, 2]])  # untouched rows


def test_relocation_values_torch_agrees_with_the_reference():
    os_, Ns = [], []
    for o in OPACITIES:
        for N in (1, 2, 3, 10, 33, 51, 60):
            os_.append(o)
            Ns.append(N)
    o = torch.tensor(os_, dtype=torch.float64)
    scale = torch.tensor([[0.5, 1.0, 2.0]], dtype=torch.float64).expand(len(os_), 3)
    new_o, new_s = mcmc.relocation_values(o, scale, torch.tensor(Ns))
    assert new_o.dtype == torch.float64 and new_s.dtype == torch.float64 and new_s.shape == (len(os_), 3)
    for i, (oi, Ni) in enumerate(zip(os_, Ns)):
        on, _D, coeff = R.relocation(oi, Ni)
        assert float(new_o[i]) == pytest.approx(on, rel=1e-12), (oi, Ni)
        assert np.allclose(new_s[i].numpy(), np.array([0.5, 1.0, 2.0]) * coeff, rtol=1e-12, atol=0), (oi, Ni)
    # N = 1 exactly
    one = [i for i, n in enumerate(Ns) if n == 1]
    assert torch.equal(new_o[one], o[one]) and torch.equal(new_s[one], scale[one])


def test_step_reference_pieces():
    """The step reference against hand-evaluated values: regulariser gradients, one Adam step from zero
    moments (p - lr * sign(g)), the gate's limits and the noise through an axis-aligned covariance."""
    op = np.array([[0.0], [2.0]])
    sc = np.log(np.array([[1.0, 2.0, 3.0], [0.5, 0.5, 0.5]]))
    go, gs = R.reg_gradients(op, sc, 0.01, 0.03)
    assert go[0, 0] == pytest.approx(0.01 / 2 * 0.25) and gs[0].tolist() == pytest.approx([0.005, 0.01, 0.015])
    p, m, v = R.adam(np.array([1.0, 1.0]), np.array([0.5, -2.0]), np.zeros(2), np.zeros(2), lr=0.1, step=1)
    assert p.tolist() == pytest.approx([0.9, 1.1]) and m.tolist() == pytest.approx([0.05, -0.2])
    assert v.tolist() == pytest.approx([0.00025, 0.004])
    gate = R.noise_gate(np.array([[-20.0], [math.log(0.005 / 0.995)], [40.0]]))
    assert gate[0, 0] == pytest.approx(1.0 / (1.0 + math.exp(-0.5)), rel=1e-6) and gate[1, 0] == pytest.approx(0.5)
    assert 0.0 <= gate[2, 0] < 1e-40  # 1 / (1 + e^99.5): nothing in fp32, where the exponential overflows
    d = R.noise_delta(np.array([[-20.0]]), np.log(np.array([[1.0, 2.0, 3.0]])), np.array([[2.0, 0, 0, 0]]),
                      np.array([[1.0, 1.0, 1.0]]), 0.1)
    assert d[0].tolist() == pytest.approx([0.1 * gate[0, 0] * s for s in (1.0, 4.0, 9.0)])
    # a quarter turn about z maps the x axis onto y: Sigma = diag(s1^2, s0^2, s2^2)
    q = np.array([[math.cos(math.pi / 4), 0, 0, math.sin(math.pi / 4)]])
    d = R.noise_delta(np.array([[-20.0]]), np.log(np.array([[1.0, 2.0, 3.0]])), q, np.array([[1.0, 0.0, 0.0]]), 1.0)
    assert d[0].tolist() == pytest.approx([4.0 * gate[0, 0], 0.0, 0.0], abs=1e-12)
