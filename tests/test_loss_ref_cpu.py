"""Pins tests/loss_maps_ref.py (the explicit statement of the fused L1+SSIM kernels' workspace maps
and backward) to autograd over oracle/loss_ref.py in float64, per pixel."""
import pytest
import torch
import torch.nn.functional as F

from oracle.loss_ref import ssim, window_2d
from tests.loss_maps_ref import KINDS, autograd_reference, loss_maps, make_inputs

SHAPES = [(3, 1, 1), (3, 1, 133), (3, 5, 6), (3, 37, 10), (3, 33, 65), (1, 11, 11), (4, 12, 70)]
TOL = 1e-12  # of the largest gradient; float64 has 1.1e-16 and the sums have 121 terms


@pytest.mark.parametrize("C,H,W", SHAPES)
@pytest.mark.parametrize("lam", [0.2, 1.0, 0.0])
def test_dimg_and_loss_match_autograd(C, H, W, lam):
    img, gt = make_inputs("random", C, H, W)
    ref_loss, ref_grad = autograd_reference(img, gt, lam)
    r = loss_maps(img.double(), gt.double(), lam)
    assert abs(float(r["loss"]) - float(ref_loss)) <= 1e-14
    assert float((r["dimg"] - ref_grad).abs().max()) <= TOL * float(ref_grad.abs().max())


@pytest.mark.parametrize("C,H,W", SHAPES)
def test_maps_match_autograd(C, H, W):
    """G1, G11, G12 are -λ/(CHW) times the gradient of sum(S) with respect to the blurred moments:
    autograd through the oracle's SSIM expression with the moments as leaves."""
    lam = 0.2
    img, gt = make_inputs("random", C, H, W)
    x, y = img.double(), gt.double()
    w = window_2d(11, C, x)

    def blur(t):
        return F.conv2d(t.unsqueeze(0), w, padding=5, groups=C).squeeze(0)

    m1, e11, e12 = (blur(t).requires_grad_(True) for t in (x, x * x, x * y))
    m2, e22 = blur(y), blur(y * y)
    m12 = m1 * m2
    num = (2 * m12 + 0.01 ** 2) * (2 * (e12 - m12) + 0.03 ** 2)
    den = (m1.pow(2) + m2.pow(2) + 0.01 ** 2) * ((e11 - m1.pow(2)) + (e22 - m2.pow(2)) + 0.03 ** 2)
    smap = num / den
    assert abs(float(smap.detach().mean()) - float(ssim(x, y))) <= 1e-14
    (-lam / (C * H * W) * smap.sum()).backward()
    r = loss_maps(x, y, lam)
    assert float((r["S"] - smap.detach()).abs().max()) <= 1e-14
    for i, leaf in enumerate((m1, e11, e12)):
        ref = leaf.grad
        assert float((r["maps"][i] - ref).abs().max()) <= TOL * float(ref.abs().max()), i


@pytest.mark.parametrize("kind", [k for k in KINDS if k not in ("equal", "both_black")] + ["impulse@32,64"])
def test_kinds_match_autograd_and_fp32_reference_is_usable(kind):
    """Every input kind with a non-zero gradient: the float64 statement agrees with autograd, and
    the same statement in float32 (the GPU tests' error yardstick) stays within 1e-4 of the
    gradient's maximum, so a bound of a few times its error still resolves single pixels."""
    C, H, W = 3, 37, 70
    img, gt = make_inputs(kind, C, H, W)
    _, ref_grad = autograd_reference(img, gt, 0.2)
    r64 = loss_maps(img.double(), gt.double(), 0.2)
    gmax = float(ref_grad.abs().max())
    assert gmax > 0
    assert float((r64["dimg"] - ref_grad).abs().max()) <= TOL * gmax
    r32 = loss_maps(img, gt, 0.2)
    assert r32["dimg"].dtype == torch.float32
    assert float((r32["dimg"].double() - r64["dimg"]).abs().max()) <= 1e-4 * gmax


@pytest.mark.parametrize("kind", ["equal", "both_black"])
def test_zero_gradient_kinds(kind):
    img, gt = make_inputs(kind, 3, 37, 70)
    r = loss_maps(img.double(), gt.double(), 0.2)
    rnd = loss_maps(*[t.double() for t in make_inputs("random", 3, 37, 70)], 0.2)
    assert abs(float(r["loss"])) <= 1e-12 and abs(float(r["ssim"]) - 1.0) <= 1e-12
    assert float(r["dimg"].abs().max()) <= 1e-9 * float(rnd["dimg"].abs().max())
