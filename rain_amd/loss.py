"""Training loss (utils/loss_utils.py:6-53): loss = (1-λ)·L1 + λ·(1-SSIM), 11x11 Gaussian window σ=1.5.

The reference's own ``ssim`` (depthwise 11x11 conv2d) is restated as test infrastructure in
oracle/loss_ref.py.  ``fused_l1_ssim_loss`` is what the train step uses: the whole loss and its gradient in two HIP
kernels (rain_amd/csrc/loss.hip) — the window is an outer product of the 1-D Gaussian
(loss_utils.py:15-19), so it is applied as two 11-tap passes over an LDS tile.  ``ssim_separable``
is the same factorisation in torch (a CPU-testable statement of what the kernel computes).  All are
pinned to the reference's ssim values by tests/golden/loss.npz.

``fused_geometry_loss`` (opt-in, no reference counterpart) is the depth-normal consistency + depth
loss on the rasterizer's depth / alpha / normal maps (rain_amd/csrc/geom_loss.hip; definition in
include/rain_loss.h), pinned to tests/geom_loss_ref.py.
"""
from __future__ import annotations

import ctypes
from functools import lru_cache
from math import exp

import torch
import torch.nn.functional as F


def window_1d(window_size: int = 11, sigma: float = 1.5) -> torch.Tensor:
    """The loss's 1-D Gaussian window (utils/loss_utils.py:15-17): exp(-(x - size//2)² / 2σ²)
    evaluated in double, stored as fp32 and normalised by its fp32 sum — the same fp32 weights the
    reference convolves with (pinned by tests/golden/loss.npz)."""
    c = window_size // 2
    w = torch.tensor([exp(-((i - c) ** 2) / (2.0 * sigma * sigma)) for i in range(window_size)],
                     dtype=torch.float32)
    return w / w.sum()


_WINDOW = None


def _window_host():
    """The reference's 1-D window gaussian(11, 1.5) (fp32 exp values normalised in fp32)."""
    global _WINDOW
    if _WINDOW is None:
        g = window_1d(11, 1.5)
        _WINDOW = (ctypes.c_float * 11)(*[float(v) for v in g])
    return _WINDOW


_ONES = {}


def _ones(device):
    """A cached device scalar 1.0 (the default grad_loss; read-only for the kernels)."""
    t = _ONES.get(device)
    if t is None:
        t = _ONES[device] = torch.ones((1,), dtype=torch.float32, device=device)
    return t


def _l1_ssim_args(who, img, gt, exact_dims=False, ws=None, with_ws=False):
    """The argument check every L1+SSIM entry point shares: float32 img / gt of one [.., C, H, W]
    shape on one HIP device (and a workspace of rl_workspace_bytes for the backward).  Dtype, shape
    and workspace size are judged before the device.  Returns C, H, W."""
    for name, t in (("img", img), ("gt", gt)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise RuntimeError(f"{who}: {name} must be a float32 tensor, got "
                               f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
    if img.dim() != 3 if exact_dims else img.dim() < 3:
        raise RuntimeError(f"{who}: img must be a [C,H,W] tensor, got {tuple(img.shape)}")
    C, H, W = img.shape[-3:]
    if img.numel() != C * H * W or img.numel() == 0:
        raise RuntimeError(f"{who}: img must be one non-empty [C,H,W] image, got {tuple(img.shape)}")
    if gt.shape != img.shape:
        raise RuntimeError(f"{who}: gt must have img's shape {tuple(img.shape)}, got {tuple(gt.shape)}")
    if with_ws:
        from . import _native as N

        need = N.loss_lib().rl_workspace_bytes(C, H, W)
        if not isinstance(ws, torch.Tensor) or not ws.is_contiguous() or ws.numel() * ws.element_size() < need:
            raise RuntimeError(f"{who}: ws must be a contiguous workspace of at least {need} bytes "
                               f"(l1_ssim_forward's for the same shape)")
    if img.device.type != "cuda":
        raise RuntimeError(f"{who}: img must be on a HIP device (no CPU fallback)")
    if gt.device != img.device:
        raise RuntimeError(f"{who}: gt must be on img's device {img.device}, got {gt.device}")
    if with_ws and ws.device != img.device:
        raise RuntimeError(f"{who}: ws must be on img's device {img.device}, got {ws.device}")
    return C, H, W


def l1_ssim_forward(img, gt, lambda_dssim):
    """Fused forward (include/rain_loss.h).  Returns (loss scalar, parts [3], workspace); the
    workspace carries the per-pixel SSIM derivative maps the backward needs."""
    from . import _native as N

    L = N.loss_lib()
    C, H, W = _l1_ssim_args("l1_ssim_forward", img, gt)
    img = img.contiguous()
    gt = gt.contiguous()
    ws = torch.empty((L.rl_workspace_bytes(C, H, W),), dtype=torch.uint8, device=img.device)
    loss = torch.empty((), dtype=torch.float32, device=img.device)
    parts = torch.empty((3,), dtype=torch.float32, device=img.device)
    rc = L.rl_l1_ssim_forward(img.data_ptr(), gt.data_ptr(), C, H, W, float(lambda_dssim), _window_host(),
                              ws.data_ptr(), ws.numel(), loss.data_ptr(), parts.data_ptr(), N.stream_of(img))
    if rc:
        raise RuntimeError(L.rl_last_error().decode())
    return loss, parts, ws


def l1_ssim_backward(img, gt, lambda_dssim, ws, grad_loss=None):
    """dLoss/dimg scaled by grad_loss (a device scalar; None = 1)."""
    from . import _native as N

    L = N.loss_lib()
    C, H, W = _l1_ssim_args("l1_ssim_backward", img, gt, ws=ws, with_ws=True)
    img = img.contiguous()
    gt = gt.contiguous()
    dimg = torch.empty_like(img)
    if grad_loss is None:
        grad_loss = _ones(img.device)
    g = grad_loss.reshape(1).contiguous().float()
    rc = L.rl_l1_ssim_backward(img.data_ptr(), gt.data_ptr(), C, H, W, float(lambda_dssim), _window_host(),
                               ws.data_ptr(), g.data_ptr(), dimg.data_ptr(), N.stream_of(img))
    if rc:
        raise RuntimeError(L.rl_last_error().decode())
    return dimg


def l1_ssim_forward_backward(img, gt, lambda_dssim, grad_loss=None):
    """Forward and backward at once (the training step's form): (loss, parts, dimg), bitwise
    l1_ssim_forward's loss / parts and l1_ssim_backward's dimg, in two launches instead of three."""
    from . import _native as N

    L = N.loss_lib()
    C, H, W = _l1_ssim_args("l1_ssim_forward_backward", img, gt)
    img = img.contiguous()
    gt = gt.contiguous()
    ws = torch.empty((L.rl_workspace_bytes(C, H, W),), dtype=torch.uint8, device=img.device)
    loss = torch.empty((), dtype=torch.float32, device=img.device)
    parts = torch.empty((3,), dtype=torch.float32, device=img.device)
    dimg = torch.empty_like(img)
    if grad_loss is None:
        grad_loss = _ones(img.device)
    g = grad_loss.reshape(1).contiguous().float()
    rc = L.rl_l1_ssim_forward_backward(img.data_ptr(), gt.data_ptr(), C, H, W, float(lambda_dssim), _window_host(),
                                       ws.data_ptr(), ws.numel(), loss.data_ptr(), parts.data_ptr(), g.data_ptr(),
                                       dimg.data_ptr(), N.stream_of(img))
    if rc:
        raise RuntimeError(L.rl_last_error().decode())
    return loss, parts, dimg


class _FusedL1SSIM(torch.autograd.Function):
    """(1-λ)·L1 + λ·(1-SSIM) in two HIP kernels (rain_amd/csrc/loss.hip, include/rain_loss.h)."""

    @staticmethod
    def forward(ctx, img, gt, lambda_dssim):
        img = img.contiguous()
        gt = gt.contiguous()
        loss, parts, ws = l1_ssim_forward(img, gt, lambda_dssim)
        ctx.save_for_backward(img, gt, ws)
        ctx.lam = float(lambda_dssim)
        ctx.mark_non_differentiable(parts)
        ctx.set_materialize_grads(False)  # no zero-filled gradient for `parts` (a fill per step)
        return loss, parts

    @staticmethod
    def backward(ctx, grad_loss, _grad_parts):
        if grad_loss is None:  # the loss itself not in the differentiated graph: zero gradient
            return None, None, None
        img, gt, ws = ctx.saved_tensors
        return l1_ssim_backward(img, gt, ctx.lam, ws, grad_loss), None, None


def fused_l1_ssim_loss(img, gt, lambda_dssim=0.2):
    """Returns (loss, parts) where parts = [loss, L1, SSIM] (device, no sync)."""
    _l1_ssim_args("fused_l1_ssim_loss", img, gt, exact_dims=True)
    return _FusedL1SSIM.apply(img, gt, lambda_dssim)


def _geom_args(depth, alpha, normal, gt_depth, tanfovx, tanfovy, alpha_min, lambda_normal, lambda_depth):
    """The maps made contiguous and the leading arguments every rl_geom_* call shares."""
    if depth.device.type != "cuda":
        raise RuntimeError("geometry loss: tensors must be on a HIP device (no CPU fallback)")
    H, W = depth.shape[-2:]
    maps = []
    for name, t, c in (("depth", depth, 1), ("alpha", alpha, 1), ("normal", normal, 3), ("gt_depth", gt_depth, 1)):
        if t is None:
            maps.append(None)
            continue
        if t.dtype != torch.float32 or t.numel() != c * H * W or t.device != depth.device:
            raise RuntimeError(f"geometry loss: {name} must be a float32 [{c}, {H}, {W}] tensor on the depth's device")
        maps.append(t.contiguous())
    ptr = [ctypes.c_void_p(t.data_ptr()) if t is not None else None for t in maps]
    head = ptr + [H, W, float(tanfovx), float(tanfovy), float(alpha_min), float(lambda_normal), float(lambda_depth)]
    return maps, head, H, W


def geometry_loss_forward(depth, alpha, normal, tanfovx, tanfovy, lambda_normal, lambda_depth=0.0, gt_depth=None,
                          alpha_min=0.1):
    """Depth-normal consistency + depth loss, forward (include/rain_loss.h rl_geom_forward).  Returns
    (loss scalar, parts [4] = {loss, L_n, L_d, valid pixels}, workspace for geometry_loss_backward)."""
    from . import _native as N

    L = N.loss_lib()
    maps, head, H, W = _geom_args(depth, alpha, normal, gt_depth, tanfovx, tanfovy, alpha_min, lambda_normal,
                                  lambda_depth)
    dev = depth.device
    ws = torch.empty((L.rl_geom_workspace_bytes(H, W),), dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    parts = torch.empty((4,), dtype=torch.float32, device=dev)
    rc = L.rl_geom_forward(*head, ws.data_ptr(), ws.numel(), loss.data_ptr(), parts.data_ptr(), N.stream_of(depth))
    if rc:
        raise RuntimeError(L.rl_last_error().decode())
    return loss, parts, ws


def _geom_grad_buffers(depth, alpha, normal, out):
    """(dD, dA, dN) to write: the caller's `out` triple or fresh uninitialised tensors."""
    if out is not None:
        return out
    return (torch.empty_like(depth, memory_format=torch.contiguous_format),
            torch.empty_like(alpha, memory_format=torch.contiguous_format),
            torch.empty_like(normal, memory_format=torch.contiguous_format) if normal is not None else None)


def geometry_loss_backward(depth, alpha, normal, tanfovx, tanfovy, lambda_normal, lambda_depth, gt_depth, alpha_min,
                           ws, grad_loss=None, out=None):
    """(dL/ddepth, dL/dalpha, dL/dnormal) scaled by grad_loss (a device scalar; None = 1); dnormal
    is None without a normal map.  `out`: a (dD, dA, dN) triple of contiguous tensors to write into."""
    from . import _native as N

    L = N.loss_lib()
    maps, head, H, W = _geom_args(depth, alpha, normal, gt_depth, tanfovx, tanfovy, alpha_min, lambda_normal,
                                  lambda_depth)
    dD, dA, dN = _geom_grad_buffers(maps[0], maps[1], maps[2], out)
    if grad_loss is None:
        grad_loss = _ones(depth.device)
    g = grad_loss.reshape(1).contiguous().float()
    rc = L.rl_geom_backward(*head, ws.data_ptr(), g.data_ptr(), dD.data_ptr(), dA.data_ptr(),
                            dN.data_ptr() if dN is not None else None, N.stream_of(depth))
    if rc:
        raise RuntimeError(L.rl_last_error().decode())
    return dD, dA, dN


def geometry_loss_forward_backward(depth, alpha, normal, tanfovx, tanfovy, lambda_normal, lambda_depth=0.0,
                                   gt_depth=None, alpha_min=0.1, grad_loss=None, out=None):
    """Forward and backward at once (the training step's form): (loss, parts, dD, dA, dN), bitwise
    geometry_loss_forward's loss / parts and geometry_loss_backward's gradients, in two launches."""
    from . import _native as N

    L = N.loss_lib()
    maps, head, H, W = _geom_args(depth, alpha, normal, gt_depth, tanfovx, tanfovy, alpha_min, lambda_normal,
                                  lambda_depth)
    dev = depth.device
    ws = torch.empty((L.rl_geom_workspace_bytes(H, W),), dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    parts = torch.empty((4,), dtype=torch.float32, device=dev)
    dD, dA, dN = _geom_grad_buffers(maps[0], maps[1], maps[2], out)
    if grad_loss is None:
        grad_loss = _ones(dev)
    g = grad_loss.reshape(1).contiguous().float()
    rc = L.rl_geom_forward_backward(*head, ws.data_ptr(), ws.numel(), loss.data_ptr(), parts.data_ptr(), g.data_ptr(),
                                    dD.data_ptr(), dA.data_ptr(), dN.data_ptr() if dN is not None else None,
                                    N.stream_of(depth))
    if rc:
        raise RuntimeError(L.rl_last_error().decode())
    return loss, parts, dD, dA, dN


class _FusedGeometryLoss(torch.autograd.Function):
    """lambda_normal·L_n + lambda_depth·L_d in two HIP kernels (rain_amd/csrc/geom_loss.hip)."""

    @staticmethod
    def forward(ctx, depth, alpha, normal, gt_depth, tanfovx, tanfovy, lambda_normal, lambda_depth, alpha_min):
        depth = depth.contiguous()
        alpha = alpha.contiguous()
        normal = normal.contiguous() if normal is not None else None
        gt_depth = gt_depth.contiguous() if gt_depth is not None else None
        ctx.cfg = (float(tanfovx), float(tanfovy), float(lambda_normal), float(lambda_depth), float(alpha_min))
        loss, parts, ws = geometry_loss_forward(depth, alpha, normal, ctx.cfg[0], ctx.cfg[1], ctx.cfg[2], ctx.cfg[3],
                                                gt_depth, ctx.cfg[4])
        ctx.has = (normal is not None, gt_depth is not None)
        ctx.save_for_backward(*[t for t in (depth, alpha, normal, gt_depth, ws) if t is not None])
        ctx.mark_non_differentiable(parts)
        ctx.set_materialize_grads(False)
        return loss, parts

    @staticmethod
    def backward(ctx, grad_loss, _grad_parts):
        if grad_loss is None:  # the loss itself not in the differentiated graph
            return (None,) * 9
        saved = list(ctx.saved_tensors)
        depth, alpha = saved[0], saved[1]
        normal = saved[2] if ctx.has[0] else None
        gt_depth = saved[2 + ctx.has[0]] if ctx.has[1] else None
        ws = saved[-1]
        tx, ty, ln, ld, amin = ctx.cfg
        dD, dA, dN = geometry_loss_backward(depth, alpha, normal, tx, ty, ln, ld, gt_depth, amin, ws, grad_loss)
        return (dD, dA, dN) + (None,) * 6


def fused_geometry_loss(depth, alpha, normal, tanfovx, tanfovy, lambda_normal=0.05, lambda_depth=0.0, gt_depth=None,
                        alpha_min=0.1):
    """Depth-normal consistency (2DGS / GOF / PGSR style) with an optional metric depth prior, on
    the maps render(normal_grad=True) returns: depth [1,H,W] = Σ α T z, alpha [1,H,W] = Σ α T, normal
    [3,H,W] = Σ α T n (include/rain_loss.h has the definition).  Returns (loss, parts) with parts =
    [loss, L_n, L_d, valid pixels] (device, no sync, not differentiable); gradients reach depth,
    alpha and normal.  `normal` may be None with lambda_normal = 0."""
    if depth.dim() != 3 or depth.device.type != "cuda":
        raise RuntimeError("fused_geometry_loss expects [1,H,W] / [3,H,W] tensors on a HIP device")
    return _FusedGeometryLoss.apply(depth, alpha, normal, gt_depth, tanfovx, tanfovy, lambda_normal, lambda_depth,
                                    alpha_min)


def _dist_args(alpha, moments, lambda_dist):
    """Checked, contiguous (alpha, moments) and the shared head of the rl_dist_* argument lists."""
    if alpha.device.type != "cuda":
        raise RuntimeError("distortion loss: tensors must be on a HIP device (no CPU fallback)")
    H, W = alpha.shape[-2:]
    for name, t, c in (("alpha", alpha, 1), ("moments", moments, 2)):
        if t.dtype != torch.float32 or t.numel() != c * H * W or t.device != alpha.device:
            raise RuntimeError(f"distortion loss: {name} must be a float32 [{c}, {H}, {W}] tensor on the alpha's device")
    alpha, moments = alpha.contiguous(), moments.contiguous()
    return alpha, moments, [alpha.data_ptr(), moments.data_ptr(), H, W, float(lambda_dist)], H, W


def _dist_grad_buffers(alpha, moments, d_alpha):
    if d_alpha is not None and (not d_alpha.is_contiguous() or d_alpha.dtype != torch.float32 or
                                d_alpha.numel() != alpha.numel() or d_alpha.device != alpha.device):
        raise RuntimeError("distortion loss: d_alpha must be a contiguous float32 tensor of alpha's size and device")
    dA = d_alpha if d_alpha is not None else torch.empty_like(alpha)
    return dA, torch.empty_like(moments)


def distortion_loss_forward(alpha, moments, lambda_dist):
    """Depth-distortion loss lambda_dist * mean(A M2 - M1^2), forward (include/rain_loss.h
    rl_dist_forward).  Returns (loss scalar, parts [2] = {loss, unweighted mean})."""
    from . import _native as N

    L = N.loss_lib()
    alpha, moments, head, H, W = _dist_args(alpha, moments, lambda_dist)
    dev = alpha.device
    ws = torch.empty((L.rl_dist_workspace_bytes(H, W),), dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    parts = torch.empty((2,), dtype=torch.float32, device=dev)
    rc = L.rl_dist_forward(*head, ws.data_ptr(), ws.numel(), loss.data_ptr(), parts.data_ptr(), N.stream_of(alpha))
    if rc:
        raise RuntimeError(L.rl_last_error().decode())
    return loss, parts


def distortion_loss_backward(alpha, moments, lambda_dist, grad_loss=None, d_alpha=None):
    """(dL/dalpha, dL/dmoments) scaled by grad_loss (a device scalar; None = 1).  With `d_alpha` (a
    contiguous float32 tensor of alpha's size) the alpha gradient is ADDED into it and it is returned;
    otherwise a fresh tensor is written."""
    from . import _native as N

    L = N.loss_lib()
    alpha, moments, head, H, W = _dist_args(alpha, moments, lambda_dist)
    dA, dM = _dist_grad_buffers(alpha, moments, d_alpha)
    if grad_loss is None:
        grad_loss = _ones(alpha.device)
    g = grad_loss.reshape(1).contiguous().float()
    rc = L.rl_dist_backward(*head, g.data_ptr(), dA.data_ptr(), dM.data_ptr(), int(d_alpha is not None),
                            N.stream_of(alpha))
    if rc:
        raise RuntimeError(L.rl_last_error().decode())
    return dA, dM


def distortion_loss_forward_backward(alpha, moments, lambda_dist, d_alpha=None, grad_loss=None):
    """Forward and backward at once (the training step's form): (loss, parts, dA, dM), bitwise
    distortion_loss_forward's loss / parts and distortion_loss_backward's gradients, in two launches.
    `d_alpha`: an existing alpha gradient (e.g. geometry_loss_forward_backward's) to add into."""
    from . import _native as N

    L = N.loss_lib()
    alpha, moments, head, H, W = _dist_args(alpha, moments, lambda_dist)
    dev = alpha.device
    ws = torch.empty((L.rl_dist_workspace_bytes(H, W),), dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    parts = torch.empty((2,), dtype=torch.float32, device=dev)
    dA, dM = _dist_grad_buffers(alpha, moments, d_alpha)
    if grad_loss is None:
        grad_loss = _ones(dev)
    g = grad_loss.reshape(1).contiguous().float()
    rc = L.rl_dist_forward_backward(*head, ws.data_ptr(), ws.numel(), loss.data_ptr(), parts.data_ptr(), g.data_ptr(),
                                    dA.data_ptr(), dM.data_ptr(), int(d_alpha is not None), N.stream_of(alpha))
    if rc:
        raise RuntimeError(L.rl_last_error().decode())
    return loss, parts, dA, dM


class _FusedDistortionLoss(torch.autograd.Function):
    """lambda_dist * mean(A M2 - M1^2) in HIP kernels (rain_amd/csrc/geom_loss.hip, rl_dist_*)."""

    @staticmethod
    def forward(ctx, alpha, moments, lambda_dist):
        alpha, moments = alpha.contiguous(), moments.contiguous()
        ctx.lam = float(lambda_dist)
        loss, parts = distortion_loss_forward(alpha, moments, ctx.lam)
        ctx.save_for_backward(alpha, moments)
        ctx.mark_non_differentiable(parts)
        ctx.set_materialize_grads(False)
        return loss, parts

    @staticmethod
    def backward(ctx, grad_loss, _grad_parts):
        if grad_loss is None:
            return None, None, None
        alpha, moments = ctx.saved_tensors
        dA, dM = distortion_loss_backward(alpha, moments, ctx.lam, grad_loss)
        return dA, dM, None


def fused_distortion_loss(alpha, moments, lambda_dist):
    """Depth-distortion loss (Mip-NeRF 360 / 2DGS) on the maps render(dist_grad=True) returns: alpha
    [1,H,W] = Σ α T and depth_moments [2,H,W] = (Σ α T m, Σ α T m²): lambda_dist · mean(A·M2 − M1²), which
    is the mean over pixels of Σ_{i>j} w_i w_j (m_i − m_j)².  Returns (loss, parts) with parts =
    [loss, unweighted mean] (device, no sync, not differentiable); gradients reach alpha and moments."""
    if alpha.dim() != 3 or alpha.device.type != "cuda":
        raise RuntimeError("fused_distortion_loss expects [1,H,W] / [2,H,W] tensors on a HIP device")
    return _FusedDistortionLoss.apply(alpha, moments, lambda_dist)


@lru_cache(maxsize=8)
def _sep_windows(window_size, channels, device, dtype):
    g = window_1d(window_size, 1.5).to(device=device, dtype=dtype)
    return (g.view(1, 1, 1, window_size).expand(channels, 1, 1, window_size).contiguous(),
            g.view(1, 1, window_size, 1).expand(channels, 1, window_size, 1).contiguous())


def ssim_separable(img1, img2, window_size=11):
    """Mean SSIM with the separable form of the same window; all five filtered maps in one batch."""
    C = img1.size(-3)
    x = torch.stack([img1, img2, img1 * img1, img2 * img2, img1 * img2], 0).reshape(1, 5 * C, *img1.shape[-2:])
    wh, wv = _sep_windows(window_size, 5 * C, img1.device, img1.dtype)
    p = window_size // 2
    y = F.conv2d(F.conv2d(x, wh, padding=(0, p), groups=5 * C), wv, padding=(p, 0), groups=5 * C)
    mu1, mu2, e11, e22, e12 = y.view(5, C, *img1.shape[-2:]).unbind(0)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sigma1_sq, sigma2_sq, sigma12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu1_mu2
    C1 = 0.01 ** 2
    C2 = 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean()
