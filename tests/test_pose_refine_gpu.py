"""Pose refinement against a frozen model (rain_amd.pose.refine_pose) on the GPU: from a camera whose
pose is off by at least half a pixel on average, Adam on the six CameraPose numbers lowers both the
photometric L1 and the distance to the true pose."""
import numpy as np
import pytest
import torch

from rain_amd import cameras, synthetic
from rain_amd.gaussian_model import GaussianModel
from rain_amd.pose import refine_pose
from rain_amd.renderer import PipelineParams, render

pytestmark = pytest.mark.gpu

# the perturbation (rot_delta, trans_delta), and the optimiser's settings
DELTA = (0.006, -0.005, 0.004, 0.02, -0.015, 0.01)
ITERS, LR = 100, 1e-3


def _pixels(cam, xyz):
    """Pixel positions [n,2] of the points under a camera's full projection."""
    ph = torch.cat([xyz, torch.ones_like(xyz[:, :1])], 1) @ cam.full_proj_transform
    ndc = ph[:, :2] / (ph[:, 3:4] + 1e-7)
    return torch.stack([((ndc[:, 0] + 1.0) * cam.image_width - 1.0) * 0.5,
                        ((ndc[:, 1] + 1.0) * cam.image_height - 1.0) * 0.5], 1)


def test_refine_pose_recovers_a_perturbed_camera(gpu):
    P, W, H = 3000, 128, 96
    g = GaussianModel(3, divide_ratio=0.8, device="cuda")
    g.set_params(synthetic.random_gaussians(P, sh_degree=3, seed=2, bench=True))
    g.active_sh_degree = 3
    cam = cameras.fibonacci_cameras(8, W, H)[3].to("cuda")
    bg = torch.zeros(3, device=gpu)
    pipe = PipelineParams()
    with torch.no_grad():
        true = render(cam, g, pipe, bg, depth_grad=True)
        target = true["render"].clone()
        seen = true["alpha"] > 0
        target_depth = torch.where(seen, true["depth"] / torch.where(seen, true["alpha"], torch.ones_like(true["alpha"])),
                                   torch.zeros_like(true["depth"]))
    start = cameras.CameraPose(cam)
    with torch.no_grad():
        start.rot_delta.copy_(torch.tensor(DELTA[:3], device=gpu))
        start.trans_delta.copy_(torch.tensor(DELTA[3:], device=gpu))
        vis = true["visibility_filter"]
        assert int(vis.sum()) > P // 2
        shift = (_pixels(start, g.get_xyz[vis]) - _pixels(cam, g.get_xyz[vis])).norm(dim=1).mean()
    print(f"perturbation: {float(shift):.3f} px on average over {int(vis.sum())} visible means")
    assert float(shift) >= 0.5  # a condition on the start, computed here
    norm0 = float(np.linalg.norm(DELTA))
    before = {k: v.grad for k, v in zip("abcdef", g.params())}
    pose, losses = refine_pose(start, g, pipe, bg, target, ITERS, LR, target_depth=target_depth)
    assert pose is start and len(losses) == ITERS and all(np.isfinite(losses))
    # the Gaussians are detached: nothing was accumulated in their .grad
    for (k, b), p in zip(before.items(), g.params()):
        assert p.grad is b, k
    with torch.no_grad():
        l1_first = float((render(cameras.CameraPose(cam).requires_grad_(False), g, pipe, bg)["render"] - target).abs().mean())
        first = cameras.CameraPose(cam)
        first.rot_delta.copy_(torch.tensor(DELTA[:3], device=gpu))
        first.trans_delta.copy_(torch.tensor(DELTA[3:], device=gpu))
        l1_start = float((render(first, g, pipe, bg)["render"] - target).abs().mean())
        l1_final = float((render(pose, g, pipe, bg)["render"] - target).abs().mean())
        norm1 = float(torch.cat([pose.rot_delta, pose.trans_delta]).norm())
    print(f"refine_pose: lr {LR}, {ITERS} iterations, perturbation {DELTA}: photometric L1 {l1_start:.4e} -> "
          f"{l1_final:.4e} (ratio {l1_final / l1_start:.3f}; at the true pose {l1_first:.1e}), |delta| {norm0:.4e} -> "
          f"{norm1:.4e} (ratio {norm1 / norm0:.3f}); loss {losses[0]:.4e} -> {losses[-1]:.4e}")
    assert l1_final < l1_start
    assert norm1 < norm0
