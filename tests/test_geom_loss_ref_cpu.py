"""Pins the reference of the geometry loss tests (tests/geom_loss_ref.py) on the CPU by known
answers, and checks the conditions its generated inputs must meet so that the GPU tests' bars
measure the kernels and not the inputs."""
import math

import pytest
import torch

from tests.geom_loss_ref import SHAPES, TANFOV, depth_normal, geometry_loss_ref, make_inputs, rays, reference, rel_l1

f64 = torch.float64


def _plane_maps(H, W, n, d, tanfovx, tanfovy):
    """D, A, N of the plane n . X = d seen through the pixel-centre rays, with N = A n."""
    r = rays(H, W, tanfovx, tanfovy, f64, "cpu")
    z = d / (n[:, None, None] * r).sum(0)
    A = 0.3 + 0.6 * torch.rand((H, W), dtype=f64, generator=torch.Generator().manual_seed(1))
    return (z * A)[None], A[None], n[:, None, None] * A[None], z


def test_tilted_plane_is_consistent():
    H, W = 23, 31
    n = torch.tensor([0.3, -0.2, -1.0], dtype=f64)
    n = n / n.norm()
    D, A, N, z = _plane_maps(H, W, n, -3.0 * float(n.norm()) * 1.0, *TANFOV)
    assert float(z.min()) > 0
    n_d, valid, P, _ok = depth_normal(D, A, *TANFOV)
    assert bool(valid.all()) and valid.shape == (H - 2, W - 2)
    assert float((n_d - n[:, None, None]).abs().max()) < 1e-12
    assert float((n_d * P[:, 1:-1, 1:-1]).sum(0).max()) < 0  # facing the camera
    loss, L_n, L_d, nv = geometry_loss_ref(D, A, N, *TANFOV, 1.0)
    assert nv == (H - 2) * (W - 2)
    assert abs(float(L_n)) <= 1e-12 and float(L_d) == 0.0 and float(loss) == float(L_n)


def test_fronto_parallel_plane_faces_the_camera_exactly():
    H, W = 9, 12
    A = torch.full((1, H, W), 0.75, dtype=f64)
    D = 2.0 * A
    n_d, valid, _P, _ok = depth_normal(D, A, *TANFOV)
    assert bool(valid.all())
    assert torch.equal(n_d, torch.tensor([0.0, 0.0, -1.0], dtype=f64)[:, None, None].expand(3, H - 2, W - 2))
    N = torch.tensor([0.0, 0.0, -1.0], dtype=f64)[:, None, None] * A
    assert float(geometry_loss_ref(D, A, N, *TANFOV, 1.0)[1]) == 0.0


@pytest.mark.parametrize("H,W", [(2, 9), (9, 2), (1, 1), (2, 2)])
def test_no_interior_no_normal_term(H, W):
    D, A, N, gt = make_inputs(H, W)
    loss, L_n, L_d, nv = geometry_loss_ref(D, A, N, *TANFOV, 1.0, 0.5, gt)
    assert float(L_n) == 0.0 and nv == 0 and float(L_d) > 0 and float(loss) == 0.5 * float(L_d)


def test_masks_and_depth_term():
    D, A, N, gt = make_inputs(5, 7)
    A = A.clone()
    A[0, 2, 3] = 0.05  # below alpha_min: the centre and its four neighbours lose their normal
    _n, valid, _P, ok = depth_normal(D, A, *TANFOV)
    assert not bool(ok[2, 3])
    expect = torch.ones(3, 5, dtype=torch.bool)
    for y, x in ((2, 3), (1, 3), (3, 3), (2, 2), (2, 4)):
        expect[y - 1, x - 1] = False
    assert torch.equal(valid, expect)
    z = D[0] / A[0]
    m = ok & (gt[0] > 0)
    L_d = geometry_loss_ref(D, A, None, *TANFOV, 0.0, 1.0, gt)[2]
    assert math.isclose(float(L_d), float((z - gt[0]).abs()[m].sum() / 35), rel_tol=1e-14)
    # gradients flow to D, A and N and the loss is linear in N
    D.requires_grad_(), A.requires_grad_(), N.requires_grad_()
    geometry_loss_ref(D, A, N, *TANFOV, 1.0, 0.5, gt)[0].backward()
    assert float(D.grad.abs().sum()) > 0 and float(A.grad.abs().sum()) > 0 and float(N.grad.abs().sum()) > 0
    assert float(D.grad[0, 2, 3]) == 0.0 and float(A.grad[0, 2, 3]) == 0.0


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("kind", ["smooth", "holes"])
def test_input_conditions(H, W, kind):
    """At every GPU-test shape: fp32 picks the float64 masks, its gradients are within 5e-5 relative
    L1 of float64 (the GPU bar is 1e-4), smooth inputs have every interior pixel valid and holes
    inputs between 50 % and 95 %."""
    r64 = reference(H, W, kind, 1.0, 0.5)
    r32 = reference(H, W, kind, 1.0, 0.5, dtype=torch.float32)
    assert r64["valid"] == r32["valid"]
    interior = max(H - 2, 0) * max(W - 2, 0)
    if kind == "smooth":
        assert r64["valid"] == interior
    elif interior > 1:
        assert 0.5 * interior <= r64["valid"] <= 0.95 * interior, (r64["valid"], interior)
    for k in ("dD", "dA", "dN"):
        if float(r64[k].abs().sum()) > 0:
            assert rel_l1(r32[k], r64[k]) < 5e-5, (k, rel_l1(r32[k], r64[k]))
        else:
            assert float(r32[k].abs().sum()) == 0.0
    assert abs(float(r32["loss"]) - float(r64["loss"])) <= 2e-6 * abs(float(r64["loss"])) + 1e-7
