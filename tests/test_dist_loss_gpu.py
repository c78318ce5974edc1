"""GPU tests of the fused depth-distortion loss (rain_amd/csrc/geom_loss.hip rl_dist_*,
rain_amd.loss.fused_distortion_loss): L = lambda mean(A M2 - M1^2) against the float64 formula on the
same fp32 maps, the gradients against their closed forms, the accumulate_alpha flag, and the
bitwise promises of the one-call form and of repeated calls.

Sizes: 37x29 (HW = 1073, no multiple of 4: one pixel per thread), 64x48 (four per thread), and a
16-byte-misaligned view of 64x48 maps (one per thread again).

Loss bar: 1e-5 * lambda * mean(A M2 + M1^2).  Per pixel the fp32 products and their difference err by
at most ~2 ulp of A M2 + M1^2 (2^-23 each); the sum runs in double.  That is ~2.4e-7 of the summed
magnitudes, so the bar leaves about 40x margin.  Gradient bar: 1e-6 relative (two fp32 roundings)."""
import pytest
import torch

from rain_amd.loss import (distortion_loss_backward, distortion_loss_forward, distortion_loss_forward_backward,
                           fused_distortion_loss)

pytestmark = pytest.mark.gpu
LAM = 0.37
CASES = {"37x29": (29, 37, False), "64x48": (48, 64, False), "64x48_misaligned": (48, 64, True)}


def _maps(H, W, misaligned, seed=3):
    """fp32 device maps shaped like a render's: alpha in [0, 1], M1 ~ A m, M2 >= M1^2 / A."""
    g = torch.Generator().manual_seed(seed)
    A = torch.rand((1, H, W), generator=g)
    m = 2.0 + 3.0 * torch.rand((1, H, W), generator=g)
    var = torch.rand((1, H, W), generator=g)
    M = torch.cat([A * m, A * (m * m + var)], 0)
    if not misaligned:
        return A.cuda().contiguous(), M.cuda().contiguous()
    # contiguous views that start 4 bytes past a 16-byte boundary
    bufA = torch.zeros(H * W + 1, device="cuda")
    bufM = torch.zeros(2 * H * W + 1, device="cuda")
    bufA[1:].copy_(A.reshape(-1))
    bufM[1:].copy_(M.reshape(-1))
    a, mm = bufA[1:].view(1, H, W), bufM[1:].view(2, H, W)
    assert a.data_ptr() % 16 == 4 and mm.data_ptr() % 16 == 4 and a.is_contiguous() and mm.is_contiguous()
    return a, mm


@pytest.fixture(scope="module")
def refs():
    """Per case, computed once: the maps and the float64 loss and closed-form gradients on them."""
    out = {}
    for name, (H, W, mis) in CASES.items():
        A, M = _maps(H, W, mis)
        a, m1, m2 = A.double(), M[0:1].double(), M[1:2].double()
        n = H * W
        out[name] = dict(A=A, M=M, mean=float((a * m2 - m1 * m1).sum() / n), mag=float((a * m2 + m1 * m1).sum() / n),
                         dA=LAM / n * m2, dM=torch.cat([-2.0 * LAM / n * m1, LAM / n * a], 0))
    return out


def _rel(x, y):
    return float((x.double() - y).abs().max() / y.abs().max())


@pytest.mark.parametrize("case", list(CASES))
def test_loss_and_gradients(gpu, refs, case):
    r = refs[case]
    # (detached views of the shared maps: a clone of the misaligned views would be aligned)
    A, M = r["A"].detach().requires_grad_(), r["M"].detach().requires_grad_()
    assert A.data_ptr() == r["A"].data_ptr() and M.data_ptr() == r["M"].data_ptr()
    loss, parts = fused_distortion_loss(A, M, LAM)
    assert not parts.requires_grad and parts.shape == (2,)
    loss.backward()
    err = abs(float(loss) - LAM * r["mean"])
    bar = 1e-5 * LAM * r["mag"]
    print(f"\n{case}: loss {float(loss):.9g} float64 {LAM * r['mean']:.9g} |diff| {err:.3e} bar {bar:.3e}")
    assert err <= bar
    assert float(parts[0]) == float(loss)
    assert abs(float(parts[1]) - r["mean"]) <= 1e-5 * r["mag"]
    ea, em = _rel(A.grad, r["dA"]), _rel(M.grad, r["dM"])
    print(f"{case}: dA rel {ea:.3e}, dM rel {em:.3e}")
    assert ea <= 1e-6 and em <= 1e-6
    # per element too (every pixel is written, none is off by more than the two roundings)
    assert torch.allclose(A.grad.double(), r["dA"], rtol=1e-6, atol=0.0)
    assert torch.allclose(M.grad.double(), r["dM"], rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("case", list(CASES))
def test_one_call_form_and_repeats_are_bitwise(gpu, refs, case):
    r = refs[case]
    A, M = r["A"], r["M"]
    loss, parts = distortion_loss_forward(A, M, LAM)
    dA, dM = distortion_loss_backward(A, M, LAM)
    l2, p2, dA2, dM2 = distortion_loss_forward_backward(A, M, LAM)
    assert torch.equal(loss, l2) and torch.equal(parts, p2) and torch.equal(dA, dA2) and torch.equal(dM, dM2)
    for _ in range(3):
        l3, p3, dA3, dM3 = distortion_loss_forward_backward(A, M, LAM)
        assert torch.equal(l2, l3) and torch.equal(p2, p3) and torch.equal(dA2, dA3) and torch.equal(dM2, dM3)
    # the autograd wrapper returns the same numbers
    a, m = A.detach().requires_grad_(), M.detach().requires_grad_()
    l4, p4 = fused_distortion_loss(a, m, LAM)
    l4.backward()
    assert torch.equal(l4.detach(), loss) and torch.equal(p4, parts)
    assert torch.equal(a.grad, dA) and torch.equal(m.grad, dM)


@pytest.mark.parametrize("case", list(CASES))
def test_accumulate_alpha_adds_exactly(gpu, refs, case):
    r = refs[case]
    A, M = r["A"], r["M"]
    H, W = A.shape[-2:]
    dA, dM = distortion_loss_backward(A, M, LAM)
    old = torch.randn((1, H, W), device="cuda", generator=torch.Generator("cuda").manual_seed(4)) * float(dA.abs().mean())
    for fn in (lambda buf: distortion_loss_backward(A, M, LAM, d_alpha=buf),
               lambda buf: distortion_loss_forward_backward(A, M, LAM, d_alpha=buf)[2:]):
        buf = old.clone()
        got, gm = fn(buf)
        assert got.data_ptr() == buf.data_ptr()  # added in place, no extra tensor
        assert torch.equal(got, old + dA)  # one fp32 add of the rounded gradient
        assert torch.equal(gm, dM)  # the moment gradients are overwritten as before
    # a misaligned accumulator takes the one-pixel path and adds the same
    flat = torch.zeros(H * W + 1, device="cuda")
    flat[1:].copy_(old.reshape(-1))
    view = flat[1:].view(1, H, W)
    got, _ = distortion_loss_backward(A, M, LAM, d_alpha=view)
    assert torch.equal(got, old + dA) and float(flat[0]) == 0.0


def test_gradient_scale_and_lambda(gpu, refs):
    r = refs["37x29"]
    A, M = r["A"], r["M"]
    base = distortion_loss_backward(A, M, LAM)
    three = distortion_loss_backward(A, M, LAM, grad_loss=torch.tensor(3.0, device="cuda"))
    for a, b in zip(base, three):
        assert float(a.abs().sum()) > 0 and torch.allclose(b, 3.0 * a, rtol=1e-6, atol=0.0)
    l0, p0 = distortion_loss_forward(A, M, 0.0)
    assert float(l0) == 0.0 and abs(float(p0[1]) - r["mean"]) <= 1e-5 * r["mag"]
