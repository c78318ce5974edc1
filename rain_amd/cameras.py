"""Camera matrices in the reference's conventions.

Restates, in numpy/torch, the helpers the reference uses to build the rasterizer's
``viewmatrix`` / ``projmatrix`` / ``campos`` inputs:

* ``getWorld2View2``      utils/graphics_utils.py:27-38
* ``getProjectionMatrix`` utils/graphics_utils.py:40-60
* ``fov2focal/focal2fov`` utils/graphics_utils.py:62-66
* ``Camera`` matrices     scene/cameras.py:102-111  (world_view_transform is W2C^T, i.e. the
  column-major memory layout the kernels read; full_proj_transform = (P·W2C)^T)

plus the synthetic camera rig of SURVEY §8(d): N views on a Fibonacci sphere looking at the
origin (up = +z), NeRF-synthetic FoV.  Pinned against the reference's own functions by
tests/golden (make_golden.py imports them in the dev container).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch


def getWorld2View2(R, t, translate=np.array([0.0, 0.0, 0.0]), scale=1.0):
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = R.transpose()
    Rt[:3, 3] = t
    Rt[3, 3] = 1.0
    C2W = np.linalg.inv(Rt)
    cam_center = (C2W[:3, 3] + translate) * scale
    C2W[:3, 3] = cam_center
    return np.float32(np.linalg.inv(C2W))


def getProjectionMatrix(znear, zfar, fovX, fovY):
    tan_half_y = math.tan(fovY / 2)
    tan_half_x = math.tan(fovX / 2)
    top = tan_half_y * znear
    bottom = -top
    right = tan_half_x * znear
    left = -right
    P = torch.zeros(4, 4)
    z_sign = 1.0
    P[0, 0] = 2.0 * znear / (right - left)
    P[1, 1] = 2.0 * znear / (top - bottom)
    P[0, 2] = (right + left) / (right - left)
    P[1, 2] = (top + bottom) / (top - bottom)
    P[3, 2] = z_sign
    P[2, 2] = z_sign * zfar / (zfar - znear)
    P[2, 3] = -(zfar * znear) / (zfar - znear)
    return P


def fov2focal(fov, pixels):
    return pixels / (2 * math.tan(fov / 2))


def focal2fov(focal, pixels):
    return 2 * math.atan(pixels / (2 * focal))


@dataclass
class Camera:
    """Matrix part of scene/cameras.py:Camera (no image).  All tensors on ``device``."""
    R: np.ndarray
    T: np.ndarray
    FoVx: float
    FoVy: float
    image_width: int
    image_height: int
    uid: int = 0
    znear: float = 0.01
    zfar: float = 100.0
    device: str = "cpu"

    def __post_init__(self):
        # transposed then made contiguous once: the kernels read the column-major W2C, and a strided
        # view would cost a copy kernel in every render
        self.world_view_transform = torch.tensor(getWorld2View2(self.R, self.T)).transpose(0, 1).contiguous().to(
            self.device)
        self.projection_matrix = getProjectionMatrix(self.znear, self.zfar, self.FoVx, self.FoVy).transpose(0, 1).to(
            self.device)
        self.full_proj_transform = (self.world_view_transform.unsqueeze(0).bmm(
            self.projection_matrix.unsqueeze(0))).squeeze(0)
        self.camera_center = self.world_view_transform.inverse()[3, :3].contiguous()

    def to(self, device):
        return Camera(self.R, self.T, self.FoVx, self.FoVy, self.image_width, self.image_height, self.uid,
                      self.znear, self.zfar, str(device))


def skew(w: torch.Tensor) -> torch.Tensor:
    """[3] -> the 3x3 cross-product matrix [w]x."""
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


class _KeepBase(torch.autograd.Function):
    """The value of `base`, the gradient of `computed` (CameraPose at zero deltas: E = I reproduces the
    base matrix's values, but a product with I turns a -0 entry into +0; selecting the base keeps the
    matrix bitwise, and the gradient still reaches the deltas)."""

    @staticmethod
    def forward(ctx, computed, base):
        return base.clone()

    @staticmethod
    def backward(ctx, grad):
        return grad, None


class CameraPose(torch.nn.Module):
    """A Camera with a learnable pose correction (pose refinement, tracking; render(pose_grad=True)).

    With the base world-to-view rotation R and translation t of `camera`, the parameters
    rot_delta [3] (an axis-angle vector, left-multiplied) and trans_delta [3], both zero-initialised, and
    E = matrix_exp(skew(rot_delta)) (whose gradient is finite at 0): R' = E R, t' = E t + trans_delta.
    It exposes, differentiably, what render() reads of a Camera: world_view_transform ([R' t'; 0 1]^T,
    contiguous), full_proj_transform (world_view_transform @ projection_matrix), camera_center
    (-R'^T t', closed form), and FoVx / FoVy / image_width / image_height.  At zero deltas the two
    matrices equal the base camera's.  `dtype`: the parameters' and matrices' type (float64 for
    reference computations; the rasterizer takes float32)."""

    def __init__(self, camera: Camera, dtype=torch.float32):
        super().__init__()
        self.FoVx, self.FoVy = camera.FoVx, camera.FoVy
        self.image_width, self.image_height = camera.image_width, camera.image_height
        self.uid = camera.uid
        w2c = camera.world_view_transform.detach().to(dtype).transpose(0, 1)
        self.register_buffer("base_wvt", camera.world_view_transform.detach().to(dtype).contiguous())
        self.register_buffer("base_fpt", camera.full_proj_transform.detach().to(dtype).contiguous())
        self.register_buffer("base_R", w2c[:3, :3].contiguous())
        self.register_buffer("base_t", w2c[:3, 3].contiguous())
        self.register_buffer("projection_matrix", camera.projection_matrix.detach().to(dtype).contiguous())
        dev = camera.world_view_transform.device
        self.rot_delta = torch.nn.Parameter(torch.zeros(3, dtype=dtype, device=dev))
        self.trans_delta = torch.nn.Parameter(torch.zeros(3, dtype=dtype, device=dev))

    def rotation_translation(self):
        """(R' [3,3], t' [3]) of the corrected world-to-view transform."""
        E = torch.linalg.matrix_exp(skew(self.rot_delta))
        return E @ self.base_R, E @ self.base_t + self.trans_delta

    @property
    def world_view_transform(self):
        R, t = self.rotation_translation()
        bottom = torch.zeros((3, 1), dtype=R.dtype, device=R.device)
        one = torch.ones((1, 1), dtype=R.dtype, device=R.device)
        # rows of the transpose: [R'^T 0], [t'^T 1]
        wvt = torch.cat([torch.cat([R.transpose(0, 1), bottom], 1), torch.cat([t.view(1, 3), one], 1)], 0).contiguous()
        if not bool(torch.cat([self.rot_delta.detach(), self.trans_delta.detach()]).any()):
            wvt = _KeepBase.apply(wvt, self.base_wvt)  # zero deltas: the base camera's matrix, bitwise
        return wvt

    @property
    def full_proj_transform(self):
        fpt = self.world_view_transform.unsqueeze(0).bmm(self.projection_matrix.unsqueeze(0)).squeeze(0)
        if not bool(torch.cat([self.rot_delta.detach(), self.trans_delta.detach()]).any()):
            fpt = _KeepBase.apply(fpt, self.base_fpt)  # (the base's product may come from another device)
        return fpt

    @property
    def camera_center(self):
        R, t = self.rotation_translation()
        return -(R.transpose(0, 1) @ t)


def look_at_R_T(eye: np.ndarray, target=np.zeros(3), up=np.array([0.0, 0.0, 1.0])):
    """COLMAP-style (R, T) for a camera at ``eye`` looking at ``target``: x right, y down, z forward.

    The reference stores R as camera-to-world rotation and T as the world-to-camera translation
    (scene/dataset_readers.py:246-252: R = transpose(w2c[:3,:3]), T = w2c[:3,3])."""
    fwd = target - eye
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    if np.linalg.norm(right) < 1e-6:
        right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, down, fwd, eye
    w2c = np.linalg.inv(c2w)
    return np.transpose(w2c[:3, :3]), w2c[:3, 3]


def fibonacci_cameras(n: int, width: int, height: int, radius: float = 4.0, fovx: float = 0.6911112,
                      device: str = "cpu"):
    """``n`` views on a Fibonacci sphere of ``radius`` looking at the origin."""
    fovy = focal2fov(fov2focal(fovx, width), height)
    cams = []
    golden = math.pi * (3.0 - math.sqrt(5.0))
    for i in range(n):
        z = 1.0 - 2.0 * (i + 0.5) / n
        r = math.sqrt(max(0.0, 1.0 - z * z))
        th = golden * i
        eye = radius * np.array([r * math.cos(th), r * math.sin(th), z])
        R, T = look_at_R_T(eye)
        cams.append(Camera(R, T, fovx, fovy, width, height, uid=i, device=device))
    return cams
