"""GPU tests of the fused depth-normal consistency + depth loss (rain_amd/csrc/geom_loss.hip,
rain_amd.loss.fused_geometry_loss, Trainer's lambda_normal) against the float64 torch reference
tests/geom_loss_ref.py (pinned by tests/test_geom_loss_ref_cpu.py)."""
import math

import pytest
import torch

from rain_amd import cameras, synthetic
from rain_amd.gaussian_model import GaussianModel, OptimizationParams
from rain_amd.loss import (fused_geometry_loss, geometry_loss_backward, geometry_loss_forward,
                           geometry_loss_forward_backward)
from rain_amd.renderer import PipelineParams, render
from rain_amd.train import TrainConfig, Trainer
from tests.geom_loss_ref import SHAPES, TANFOV, geometry_loss_ref, make_inputs, reference

pytestmark = pytest.mark.gpu
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
TERMS = {"normal": (1.0, 0.0), "depth": (0.0, 0.7), "both": (1.0, 0.7)}  # (lambda_normal, lambda_depth)


def rel_l1(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().sum() / b.abs().sum())


def _device_inputs(H, W, kind, terms):
    """fp32 device maps; a term's map is given only when the term is on (exercises the NULL forms)."""
    ln, ld = TERMS[terms]
    D, A, N, gt = (t.float().cuda() for t in make_inputs(H, W, kind))
    return D, A, (N if ln else None), (gt if ld else None), ln, ld


@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("kind", ["smooth", "holes"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_parity_with_float64_reference(gpu, H, W, kind, terms):
    D, A, N, gt, ln, ld = _device_inputs(H, W, kind, terms)
    ref = reference(H, W, kind, ln, ld)
    D.requires_grad_(), A.requires_grad_()
    if N is not None:
        N.requires_grad_()
    loss, parts = fused_geometry_loss(D, A, N, TANFOV[0], TANFOV[1], lambda_normal=ln, lambda_depth=ld, gt_depth=gt)
    assert not parts.requires_grad
    loss.backward()
    p = parts.cpu()
    loss = loss.detach()
    print(f"\n{H}x{W} {kind} {terms}: loss {float(loss):.9g} ref {float(ref['loss']):.9g} valid {int(p[3])}")
    assert abs(float(loss) - float(ref["loss"])) <= 2e-6 * abs(float(ref["loss"])) + 1e-7
    assert float(p[0]) == float(loss)
    assert abs(float(p[1]) - float(ref["L_n"])) <= 2e-6 * abs(float(ref["L_n"])) + 1e-7
    assert abs(float(p[2]) - float(ref["L_d"])) <= 2e-6 * abs(float(ref["L_d"])) + 1e-7
    assert int(p[3]) == ref["valid"]
    for name, got in (("dD", D.grad), ("dA", A.grad), ("dN", N.grad if N is not None else None)):
        want = ref[name]
        if got is None:
            assert float(want.abs().sum()) == 0.0
            continue
        assert got.shape == want.shape
        if float(want.abs().sum()) == 0.0:  # e.g. 2x9 without the depth term, 3x3 with a hole
            assert float(got.abs().sum()) == 0.0, name
        else:
            e = rel_l1(got, want)
            print(f"  {name} rel L1 {e:.3g}")
            assert e < 1e-4, (name, e)


@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("H,W", SHAPES)
def test_every_gradient_pixel_is_written(gpu, H, W, terms):
    D, A, N, gt, ln, ld = _device_inputs(H, W, "holes", terms)
    nan = float("nan")

    def buffers():
        return (torch.full_like(D, nan), torch.full_like(A, nan), torch.full_like(N, nan) if N is not None else None)

    _loss, _parts, ws = geometry_loss_forward(D, A, N, *TANFOV, ln, ld, gt)
    out = buffers()
    geometry_loss_backward(D, A, N, *TANFOV, ln, ld, gt, 0.1, ws, out=out)
    out2 = buffers()
    geometry_loss_forward_backward(D, A, N, *TANFOV, ln, ld, gt, out=out2)
    for t in (*out, *out2):
        if t is not None:
            assert not bool(torch.isnan(t).any())


@pytest.mark.parametrize("scale", [None, 0.37])
@pytest.mark.parametrize("H,W", SHAPES)
def test_forward_backward_matches_separate_calls_bitwise(gpu, H, W, scale):
    D, A, N, gt, ln, ld = _device_inputs(H, W, "holes", "both")
    gl = None if scale is None else torch.tensor([scale], device="cuda")

    def separate():
        loss, parts, ws = geometry_loss_forward(D, A, N, *TANFOV, ln, ld, gt)
        return (loss, parts) + geometry_loss_backward(D, A, N, *TANFOV, ln, ld, gt, 0.1, ws, gl)

    def fused():
        return geometry_loss_forward_backward(D, A, N, *TANFOV, ln, ld, gt, grad_loss=gl)

    s1, s2, f1, f2 = separate(), separate(), fused(), fused()
    for a, b, c, d in zip(s1, s2, f1, f2):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(c, d)
    if scale is not None and float(s1[2].abs().sum()) > 0:
        plain = geometry_loss_forward_backward(D, A, N, *TANFOV, ln, ld, gt)
        for a, b in zip(f1[2:], plain[2:]):
            assert torch.allclose(a, scale * b, rtol=1e-6, atol=0.0)


def test_gradient_scale(gpu):
    H, W = 37, 53
    grads = []
    for k in (1.0, 3.0):
        D, A, N, gt, ln, ld = _device_inputs(H, W, "holes", "both")
        for t in (D, A, N):
            t.requires_grad_()
        loss, parts = fused_geometry_loss(D, A, N, *TANFOV, lambda_normal=ln, lambda_depth=ld, gt_depth=gt)
        (k * loss).backward()
        grads.append((D.grad, A.grad, N.grad))
    for a, b in zip(*grads):
        assert float(a.abs().sum()) > 0
        assert torch.allclose(b, 3.0 * a, rtol=1e-6, atol=0.0)


def _model(P, seed, sh_degree=1):
    g = GaussianModel(sh_degree, divide_ratio=0.8, device="cuda")
    p = synthetic.random_gaussians(P, sh_degree=sh_degree, seed=seed, bench=True)
    p["rotation"] = p["rotation"] * 1.7
    # anisotropic scales, so the normals (shortest axes) and the rotations matter
    p["scaling"] = p["scaling"] + 0.4 * torch.randn(p["scaling"].shape, generator=torch.Generator().manual_seed(seed))
    g.set_params(p)
    g.active_sh_degree = sh_degree
    g.spatial_lr_scale = 4.4
    return g


def _params(g):
    return dict(zip(NAMES, (g._xyz, g._features_dc, g._features_rest, g._opacity, g._scaling, g._rotation)))


def test_end_to_end_parameter_gradients(gpu):
    """fused_geometry_loss and the torch reference (fp32, on the device) on the same rendered maps,
    both backpropagated through the same rasterizer: the six raw parameter gradients agree."""
    P, W, H = 2000, 96, 64
    cam = cameras.fibonacci_cameras(8, W, H)[3].to("cuda")
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    bg = torch.zeros(3, device="cuda")
    g = _model(P, seed=5)
    for p in g.params():
        p.requires_grad_(True)
    out = {}
    for which in ("hip", "ref"):
        for p in g.params():
            p.grad = None
        pkg = render(cam, g, PipelineParams(), bg, normal_grad=True)
        D, A, Nm = pkg["depth"], pkg["alpha"], pkg["normal"]
        gt = (D / A.clamp_min(0.1)).detach() + 0.2  # a depth prior off the kink
        if which == "hip":
            loss, parts = fused_geometry_loss(D, A, Nm, tx, ty, lambda_normal=1.0, lambda_depth=0.5, gt_depth=gt)
            nvalid = int(parts[3])
        else:
            loss, _ln, _ld, nv = geometry_loss_ref(D, A, Nm, tx, ty, 1.0, 0.5, gt)
            assert nv == nvalid and nv > 0.2 * H * W, (nv, nvalid)
        loss.backward()
        out[which] = (float(loss.detach()), {k: v.grad.clone() if v.grad is not None else torch.zeros_like(v)
                                    for k, v in _params(g).items()})
    (la, ga), (lb, gb) = out["hip"], out["ref"]
    assert abs(la - lb) <= 1e-5 * abs(lb)
    for k in NAMES:
        if float(gb[k].abs().sum()) == 0.0:  # colours do not see the geometry loss
            assert float(ga[k].abs().sum()) == 0.0, k
            continue
        e = rel_l1(ga[k], gb[k])
        print(f"\n  {k}: rel L1 {e:.3g}")
        assert e < 1e-4, (k, e)
    assert float(ga["rotation"].abs().sum()) > 0


def _trainer(use_fused, lam, P=20_000, W=160, H=120, V=6, steps=6):
    cams = [c.to("cuda") for c in cameras.fibonacci_cameras(V, W, H)]
    gts = [torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(10 + i)) for i in range(V)]
    g = _model(P, seed=2, sh_degree=3)
    # no densify / prune or opacity reset inside the window
    opt = OptimizationParams(densify_from_iter=500, lambda_normal=lam, lambda_normal_from_iter=1)
    g.training_setup(opt)
    t = Trainer(g, cams, gts, opt, cfg=TrainConfig(c2f=False, seed=3), scene_extent=4.4, fused=use_fused)
    assert t.fused == use_fused
    losses = [t.step(it, sync_loss=True).loss for it in range(1, steps + 1)]
    return g, losses, t


def test_trainer_fused_matches_autograd_with_lambda_normal(gpu):
    (ga, la, _ta), (gb, lb, _tb) = _trainer(False, 0.05), _trainer(True, 0.05)
    for x, y in zip(la, lb):
        assert abs(x - y) <= 1e-5 * abs(y), (la, lb)
    for k, x in _params(ga).items():
        y = _params(gb)[k]
        e = rel_l1(x, y)
        assert e < 1e-5, (k, e)
    # the term is in the loss and reaches the rotations
    g0, l0, _t0 = _trainer(True, 0.0)
    assert all(a != b for a, b in zip(lb, l0))
    assert not torch.equal(gb._rotation, g0._rotation)
    assert rel_l1(gb._rotation, g0._rotation) > 1e-6


def test_trainer_refuses_lambda_normal_on_sharded_paths(gpu):
    g, _l, t = _trainer(True, 0.05, steps=0)
    t.sharded = True  # what world > 1 (or a forced exchange) sets; no ranks are started
    with pytest.raises(ValueError, match="lambda_normal > 0 needs the single-GPU step"):
        t.step(1)
    g2, _l2, t2 = _trainer(False, 0.05, steps=0)
    t2.sharded = True
    with pytest.raises(ValueError, match="lambda_normal > 0 needs the single-GPU step"):
        t2.step(1)
