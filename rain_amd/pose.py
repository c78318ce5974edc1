"""Camera-pose refinement against a frozen scene (noisy COLMAP / SLAM poses, tracking).

refine_pose() renders with render(pose_grad=True), whose backward returns the gradients of the three
camera arrays (include/rain_raster.h rr_backward_camera), chains them through
rain_amd.cameras.CameraPose into its six numbers and steps those with Adam.  The Gaussians receive
no gradient.
"""
from __future__ import annotations

import torch

from .cameras import CameraPose
from .renderer import render


def refine_pose(camera, pc, pipe, bg, target_image, iters, lr, target_depth=None, low_pass=0.3):
    """Refine the pose of `camera` (a Camera, or a CameraPose to continue from) so that the render of
    `pc` matches `target_image` [3,H,W]: Adam (`lr`, `iters` steps) on CameraPose's rot_delta and
    trans_delta.  The loss is the mean L1 on colour, plus the mean L1 between depth / alpha and
    `target_depth` [1,H,W] where that is given (pixels with alpha > 0).  Returns (pose, losses): the
    CameraPose and the loss of every iteration (floats, evaluated before that iteration's step).
    pipe.antialiasing raises a ValueError: camera gradients of an anti-aliased frame are a follow-up."""
    if bool(getattr(pipe, "antialiasing", False)):
        raise ValueError("refine_pose does not combine with pipe.antialiasing yet (follow-up: camera-pose gradients "
                         "of an anti-aliased frame)")
    pose = camera if isinstance(camera, CameraPose) else CameraPose(camera)
    params = [pose.rot_delta, pose.trans_delta]
    opt = torch.optim.Adam(params, lr=lr)
    losses = []
    for _ in range(int(iters)):
        pkg = render(pose, pc, pipe, bg, low_pass=low_pass, pose_grad=True)
        loss = (pkg["render"] - target_image).abs().mean()
        if target_depth is not None:
            alpha = pkg["alpha"]
            seen = alpha > 0
            expected = pkg["depth"] / torch.where(seen, alpha, torch.ones_like(alpha))
            loss = loss + (torch.where(seen, expected - target_depth, torch.zeros_like(alpha))).abs().mean()
        # the pose's gradients only: the Gaussians stay detached (nothing accumulates in their .grad)
        grads = torch.autograd.grad(loss, params, allow_unused=True)
        for p, g in zip(params, grads):
            p.grad = g if g is not None else torch.zeros_like(p)
        opt.step()
        losses.append(float(loss.detach()))
    return pose, losses
