"""Operator surface of the reference rasterizer over the MI355X ``_C``.

Interface only (the computation is in ``_C`` -> include/rain_raster.h -> rain_amd/csrc): the public
names, field order, argument meaning, error messages, debug-snapshot behaviour and autograd
contract are those of the reference's
submodules/diff_gaussian_rasterization/diff_gaussian_rasterization/__init__.py (Inria
Gaussian-Splatting licence, LICENSE.md there) — ``rasterize_gaussians`` (:10-31),
``_RasterizeGaussians`` (:33-146), ``GaussianRasterizationSettings`` (:148-161),
``GaussianRasterizer`` (:163-212) — so ``gaussian_renderer.render`` (gaussian_renderer/__init__.py:
9-79) runs against it unchanged.  The code is organised differently: argument packing and the
debug snapshot are shared helpers.
"""
import contextlib
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C

_MSG_COLOR = 'Please provide excatly one of either SHs or precomputed colors!'  # reference text, typo included
_MSG_COV = 'Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!'
_MSG_DIST = 'forward_distortion needs 0 < dist_near < dist_far, or both 0 (metric depth)'
_MSG_AA_CAMERA = ('forward_camera does not combine with antialiasing yet (follow-up: camera-pose gradients of an '
                  'anti-aliased frame, RR_FLAG_ANTIALIAS)')
_MSG_ABS = ('{} does not combine with absgrad yet (follow-up: absolute-gradient statistics together with {}, '
            'RR_FLAG_ABSGRAD)')
_MSG_NORMAL = 'render_depth_normal needs the scale/rotation pair (normals come from the scale axes)'


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    low_pass: float


def _antialiased(on):
    """_C.antialiased(on): the calls inside the block serve anti-aliased frames.  A stand-in `_C` without the
    switch (a CPU oracle bound in its place) serves plain frames only."""
    if hasattr(_C, "antialiased"):
        return _C.antialiased(on)
    if on:
        raise RuntimeError("antialiasing needs the rasterizer's own _C (this one has no antialiased() switch)")
    return contextlib.nullcontext()


def _antialiasing_on():
    fn = getattr(_C, "antialiasing_on", None)
    return bool(fn is not None and fn())


def _absgrad(on):
    """_C.absgrad(on): the backward calls inside the block also sum the absolute mean2D gradients.  A stand-in
    `_C` without the switch serves the signed gradients only."""
    if hasattr(_C, "absgrad"):
        return _C.absgrad(on)
    if on:
        raise RuntimeError("absgrad needs the rasterizer's own _C (this one has no absgrad() switch)")
    return contextlib.nullcontext()


def _absgrad_on():
    fn = getattr(_C, "absgrad_on", None)
    return bool(fn is not None and fn())


def _host_copy(values):
    """CPU clones of every tensor argument (what the reference dumps when a debug call fails)."""
    return tuple(v.cpu().clone() if isinstance(v, torch.Tensor) else v for v in values)


def _invoke(fn, args, debug: bool, dump: str, message: str):
    """Call a ``_C`` entry point; in debug mode a failing call leaves ``dump`` (torch.save of the
    arguments on the CPU) in the working directory before the exception propagates
    (__init__.py:73-80,123-130)."""
    if not debug:
        return fn(*args)
    snapshot = _host_copy(args)
    try:
        return fn(*args)
    except Exception:
        torch.save(snapshot, dump)
        print(message)
        raise


def _forward_args(s: GaussianRasterizationSettings, means3D, colors, opacities, scales, rotations, cov3D, sh):
    """Argument tuple of _C.rasterize_gaussians (rasterize_points.cu:24-44)."""
    return (s.bg, means3D, colors, opacities, scales, rotations, s.scale_modifier, cov3D, s.viewmatrix,
            s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width, sh, s.sh_degree, s.campos,
            s.prefiltered, s.debug, s.low_pass)


def _backward_args(s: GaussianRasterizationSettings, saved, num_rendered, grad_color):
    """Argument tuple of _C.rasterize_gaussians_backward (rasterize_points.cu:110-133)."""
    colors, means3D, scales, rotations, cov3D, radii, sh, geom, binning, img = saved
    return (s.bg, means3D, radii, colors, scales, rotations, s.scale_modifier, cov3D, s.viewmatrix, s.projmatrix,
            s.tanfovx, s.tanfovy, grad_color, sh, s.sh_degree, s.campos, geom, num_rendered, binning, img, s.debug,
            s.low_pass)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings):
        s = raster_settings
        args = _forward_args(s, means3D, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, sh)
        num_rendered, color, radii, depth, geom, binning, img = _invoke(
            _C.rasterize_gaussians, args, s.debug, "snapshot_fw.dump",
            "\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
        ctx.raster_settings = s
        ctx.num_rendered = num_rendered
        ctx.antialiasing = _antialiasing_on()  # the frame's switch (_C.antialiased), for its backward
        ctx.absgrad = _absgrad_on()  # (_C.absgrad) the backward then leaves means2D.absgrad, gsplat's convention
        ctx.means2D = means2D if ctx.absgrad else None  # a plain reference: the attribute goes on this object
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning,
                              img)
        return color, radii, depth

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_depth):
        # depth receives no gradient: grad_depth is accepted and dropped (__init__.py:91-120)
        s = ctx.raster_settings
        args = _backward_args(s, ctx.saved_tensors, ctx.num_rendered, grad_out_color)
        with _antialiased(ctx.antialiasing), _absgrad(ctx.absgrad):
            d_means2D, d_colors, d_opacities, d_means3D, d_cov3D, d_sh, d_scales, d_rotations, *d_abs = _invoke(
                _C.rasterize_gaussians_backward_abs if ctx.absgrad else _C.rasterize_gaussians_backward, args,
                s.debug, "snapshot_bw.dump",
                "\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
        if ctx.absgrad:  # [P,3], the absolute sums beside the signed .grad
            ctx.means2D.absgrad = d_abs[0]
        # order of forward()'s inputs; raster_settings gets None
        return d_means3D, d_means2D, d_sh, d_colors, d_opacities, d_scales, d_rotations, d_cov3D, None


def _aux_forward(ctx, inputs, raster_settings, normal=False, dist=None, camera=None):
    """The forward of the four aux classes: (color, radii, depth, alpha), then the normal map with
    `normal` (None without it, in a dist frame), then the moment maps with `dist` = (near, far).  `camera` =
    (viewmatrix, projmatrix, campos) replaces the settings' arrays by these differentiable inputs."""
    means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp = inputs
    s = raster_settings
    if camera is not None:
        # the kernels read contiguous fp32 arrays; the gradients come back in that layout
        viewmatrix, projmatrix, campos = (t.detach().to(torch.float32).contiguous() for t in camera)
        ctx.cam_shapes = (viewmatrix.shape, projmatrix.shape, campos.shape)
        s = s._replace(viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos)
    args = _forward_args(s, means3D, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, sh)
    fn = _C.rasterize_gaussians_aux if normal else _C.rasterize_gaussians
    if dist is not None:
        fn, args = _C.rasterize_gaussians_dist, args + dist + (normal,)
    num_rendered, color, radii, depth, *maps, geom, binning, img = _invoke(
        fn, args, s.debug, "snapshot_fw.dump",
        "\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
    alpha = _C.accumulated_alpha(img, s.image_height, s.image_width)
    ctx.raster_settings = s
    ctx.num_rendered = num_rendered
    ctx.dist = dist or ()
    ctx.antialiasing = _antialiasing_on()  # the frame's switch (_C.antialiased), for its backward
    ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning,
                          img)
    ctx.mark_non_differentiable(radii)
    ctx.set_materialize_grads(False)  # an output the loss does not use costs no zero fill and no work
    return (color, radii, depth, alpha, *maps)


def _aux_backward(ctx, fn, grads, n_inputs, camera=False):
    """The backward of the four aux classes: `grads` = (colour, depth, alpha[, normal[, moments]]) as `fn`,
    the class's _C entry, takes them after the reference's arguments; one gradient per forward input
    (`n_inputs`; raster_settings and the plain values get None).  With `camera` the three inputs after
    raster_settings receive rasterize_gaussians_backward_camera's gradients when one of them needs any."""
    if all(g is None for g in grads):
        return (None,) * n_inputs
    s = ctx.raster_settings
    grads = _absent_as_empty(*grads)  # "absent" (a NULL pointer in the library)
    args = _backward_args(s, ctx.saved_tensors, ctx.num_rendered, grads[0]) + grads[1:] + ctx.dist
    camera = camera and any(ctx.needs_input_grad[9:12])  # a fixed camera: the plain depth backward
    with _antialiased(ctx.antialiasing):
        d_means2D, d_colors, d_opacities, d_means3D, d_cov3D, d_sh, d_scales, d_rotations, *d_cam = _invoke(
            _C.rasterize_gaussians_backward_camera if camera else fn, args, s.debug, "snapshot_bw.dump",
            "\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
    # (in the inputs' own shapes: a flat [16] matrix gets a flat gradient)
    d_cam = tuple(g.view(shape) for g, shape in zip(d_cam, ctx.cam_shapes)) if camera else ()
    res = (d_means3D, d_means2D, d_sh, d_colors, d_opacities, d_scales, d_rotations, d_cov3D, None) + d_cam
    return res + (None,) * (n_inputs - len(res))


class _RasterizeGaussiansDepth(torch.autograd.Function):
    """_RasterizeGaussians with differentiable depth and accumulated-alpha outputs (no reference
    counterpart; GaussianRasterizer.forward_depth): returns (color, radii, depth, alpha) with
    depth D = sum alpha_i T_i z_i and alpha A = 1 - T_final = sum alpha_i T_i, both [1,H,W]."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings):
        return _aux_forward(ctx, (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp),
                            raster_settings)

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_depth, grad_alpha):
        return _aux_backward(ctx, _C.rasterize_gaussians_backward_depth, (grad_out_color, grad_depth, grad_alpha), 9)


class _RasterizeGaussiansCamera(torch.autograd.Function):
    """_RasterizeGaussiansDepth with the camera as a differentiable input (no reference counterpart;
    GaussianRasterizer.forward_camera): viewmatrix, projmatrix and campos of the settings are also passed
    as tensor inputs, three independent ones, and receive the gradients of
    _C.rasterize_gaussians_backward_camera.  Returns (color, radii, depth, alpha)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, viewmatrix, projmatrix, campos):
        return _aux_forward(ctx, (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp),
                            raster_settings, camera=(viewmatrix, projmatrix, campos))

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_depth, grad_alpha):
        return _aux_backward(ctx, _C.rasterize_gaussians_backward_depth, (grad_out_color, grad_depth, grad_alpha), 12,
                             camera=True)


class _RasterizeGaussiansNormal(torch.autograd.Function):
    """_RasterizeGaussiansDepth plus a differentiable aux normal map (no reference counterpart;
    GaussianRasterizer.forward_normal): returns (color, radii, depth, alpha, normal) with
    normal N = sum alpha_i T_i n_i [3,H,W] (render_depth_normal's map)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings):
        return _aux_forward(ctx, (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp),
                            raster_settings, normal=True)

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_depth, grad_alpha, grad_normal):
        return _aux_backward(ctx, _C.rasterize_gaussians_backward_normal,
                             (grad_out_color, grad_depth, grad_alpha, grad_normal), 9)


class _RasterizeGaussiansDist(torch.autograd.Function):
    """_RasterizeGaussiansNormal plus the differentiable depth-moment maps of the distortion loss (no
    reference counterpart; GaussianRasterizer.forward_distortion): returns (color, radii, depth, alpha,
    normal or None, moments) with moments [2,H,W] = (sum alpha_i T_i m_i, sum alpha_i T_i m_i^2)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, dist_near, dist_far, normal):
        return _aux_forward(ctx, (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp),
                            raster_settings, normal=bool(normal), dist=(float(dist_near), float(dist_far)))

    @staticmethod
    def backward(ctx, grad_out_color, grad_radii, grad_depth, grad_alpha, grad_normal, grad_moments):
        return _aux_backward(ctx, _C.rasterize_gaussians_backward_dist,
                             (grad_out_color, grad_depth, grad_alpha, grad_normal, grad_moments), 12)


def _check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp):
    """The reference's two argument checks (__init__.py:177-187)."""
    if (shs is None) == (colors_precomp is None):
        raise Exception(_MSG_COLOR)
    have_pair = scales is not None and rotations is not None
    have_any = scales is not None or rotations is not None
    if (cov3D_precomp is None and not have_pair) or (cov3D_precomp is not None and have_any):
        raise Exception(_MSG_COV)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings):
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings)


def _absent_as_empty(*tensors):
    """None -> torch.Tensor([]) (a CPU numel-0 tensor, which _C reads as 'absent', __init__.py:189-199)."""
    return tuple(torch.Tensor([]) if t is None else t for t in tensors)


def _checked_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp, normal=False):
    """The preamble of every GaussianRasterizer.forward*: the reference's checks (and, for a frame with the
    aux normal map, the scale/rotation pair), then the five optional inputs with None as 'absent'."""
    _check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp)
    if normal and cov3D_precomp is not None:
        raise Exception(_MSG_NORMAL)
    return _absent_as_empty(shs, colors_precomp, scales, rotations, cov3D_precomp)


class GaussianRasterizer(nn.Module):
    # Absolute-gradient densification statistics (AbsGS, gsplat's absgrad; include/rain_raster.h
    # RR_FLAG_ABSGRAD): set on the instance after construction (r.absgrad = True).  forward()'s backward then
    # leaves means2D.absgrad [P,3], the per-pixel absolute dL/dmeans2D sums, beside means2D.grad (unchanged).
    # Left False, forward() follows the thread's `_C.absgrad()` switch instead.
    # The other forward_* methods and render_depth_normal refuse it (follow-ups).
    absgrad = False

    def __init__(self, raster_settings, antialiasing=False):
        """antialiasing (upstream 3DGS's name; it travels beside the 13 settings fields): every splat's
        opacity is scaled by sqrt(max(0.000025, det(cov2D) / det(cov2D + low_pass I))), the opacity
        compensation of the 2D dilation, and the factor's gradient reaches the covariance
        (include/rain_raster.h RR_FLAG_ANTIALIAS).  Every forward* below and its backward honour it, as do
        contributions() and render_depth_normal(); forward_camera refuses it."""
        super().__init__()
        self.raster_settings = raster_settings
        self.antialiasing = bool(antialiasing)

    def markVisible(self, positions):
        s = self.raster_settings
        with torch.no_grad():
            return _C.mark_visible(positions, s.viewmatrix, s.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        shs, colors_precomp, scales, rotations, cov3D_precomp = _checked_inputs(shs, colors_precomp, scales,
                                                                                rotations, cov3D_precomp)
        # .absgrad only ever turns the switch on: a caller's own `with _C.absgrad():` block around this call stands
        with _antialiased(self.antialiasing), (_absgrad(True) if self.absgrad else contextlib.nullcontext()):
            return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                       cov3D_precomp, self.raster_settings)

    def forward_depth(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                      cov3D_precomp=None):
        """forward() with differentiable depth and accumulated alpha (opt-in; forward()'s depth gets
        no gradient): returns (color [3,H,W], radii [P], depth [1,H,W], alpha [1,H,W]).  depth is
        sum alpha_i T_i z_i (no background term, not normalised), alpha is 1 - T_final =
        sum alpha_i T_i; expected depth is depth / alpha.  Gradient conventions are the colour
        path's (no mask for the 0.99 alpha clamp, dL/dmeans2D in NDC units)."""
        if self.absgrad:
            raise ValueError(_MSG_ABS.format("forward_depth", "depth / alpha gradients"))
        shs, colors_precomp, scales, rotations, cov3D_precomp = _checked_inputs(shs, colors_precomp, scales,
                                                                                rotations, cov3D_precomp)
        with _antialiased(self.antialiasing):
            return _RasterizeGaussiansDepth.apply(means3D, means2D, shs, colors_precomp, opacities, scales,
                                                  rotations, cov3D_precomp, self.raster_settings)

    def forward_camera(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                       cov3D_precomp=None):
        """forward_depth() with a differentiable camera (opt-in; pose refinement, tracking): the same
        (color [3,H,W], radii [P], depth [1,H,W], alpha [1,H,W]), and autograd delivers the gradients of
        raster_settings.viewmatrix / projmatrix / campos — three independent inputs, each in its memory
        layout — to whatever produced those tensors (rain_amd.cameras.CameraPose).  The view matrix is
        reached through the EWA Jacobian, its 3x3 block and the view depth of the depth map; the
        projection through means2D only (its z row gets 0); campos through the SH view direction (0
        with colors_precomp).  Culling, radii and the depth order are discrete and contribute nothing.
        A rasterizer built with antialiasing=True raises a ValueError (a follow-up)."""
        if self.antialiasing:
            raise ValueError(_MSG_AA_CAMERA)
        if self.absgrad:
            raise ValueError(_MSG_ABS.format("forward_camera", "camera-pose gradients"))
        shs, colors_precomp, scales, rotations, cov3D_precomp = _checked_inputs(shs, colors_precomp, scales,
                                                                                rotations, cov3D_precomp)
        s = self.raster_settings
        return _RasterizeGaussiansCamera.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                               cov3D_precomp, s, s.viewmatrix, s.projmatrix, s.campos)

    def forward_normal(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                       cov3D_precomp=None):
        """forward_depth() plus a differentiable aux normal map (opt-in): returns (color [3,H,W],
        radii [P], depth [1,H,W], alpha [1,H,W], normal [3,H,W]).  normal is render_depth_normal's map,
        sum alpha_i T_i n_i with n_i the view-space unit normal (the smallest-scale axis, facing the
        camera; no background term).  Its gradient reaches the rotations directly (the axis choice
        and the flip are constants) and opacity, position and covariance through alpha_i.  Needs the
        scale/rotation pair (cov3D_precomp is refused)."""
        if self.absgrad:
            raise ValueError(_MSG_ABS.format("forward_normal", "a normal-map gradient"))
        shs, colors_precomp, scales, rotations, cov3D_precomp = _checked_inputs(
            shs, colors_precomp, scales, rotations, cov3D_precomp, normal=True)
        with _antialiased(self.antialiasing):
            return _RasterizeGaussiansNormal.apply(means3D, means2D, shs, colors_precomp, opacities, scales,
                                                   rotations, cov3D_precomp, self.raster_settings)

    def forward_distortion(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                           rotations=None, cov3D_precomp=None, dist_near=0.2, dist_far=100.0, normal=False):
        """forward_depth() plus the differentiable depth-moment maps of the depth-distortion loss
        (opt-in): returns (color [3,H,W], radii [P], depth [1,H,W], alpha [1,H,W], normal [3,H,W] or None,
        moments [2,H,W]).  moments = (M1, M2) = (sum w_i m_i, sum w_i m_i^2) with w_i = alpha_i T_i and m_i
        the mapped view depth: the NDC depth far/(far-near) (1 - near/z) for 0 < dist_near < dist_far, z
        itself for dist_near = dist_far = 0.  The per-pixel distortion sum_{i>j} w_i w_j (m_i - m_j)^2 is
        alpha * M2 - M1^2 (rain_amd.loss.fused_distortion_loss).  With `normal` the aux normal map of
        forward_normal() is rendered and differentiated too (needs the scale/rotation pair)."""
        if self.absgrad:
            raise ValueError(_MSG_ABS.format("forward_distortion", "depth-moment gradients"))
        shs, colors_precomp, scales, rotations, cov3D_precomp = _checked_inputs(
            shs, colors_precomp, scales, rotations, cov3D_precomp, normal=normal)
        near, far = float(dist_near), float(dist_far)
        if not ((near == 0.0 and far == 0.0) or (0.0 < near < far < float("inf"))):
            raise Exception(_MSG_DIST)
        with _antialiased(self.antialiasing):
            return _RasterizeGaussiansDist.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                                 cov3D_precomp, self.raster_settings, near, far, bool(normal))

    @torch.no_grad()
    def contributions(self, means3D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                      cov3D_precomp=None, pixel_weight=None, out=None):
        """Forward only, then the per-Gaussian blend-contribution statistics of that frame (opt-in; what
        importance pruning reads, rain_amd.importance): returns (color [3,H,W], radii [P], stats) with
        stats = (sum_w, sum_gw, max_w, count) of _C.gaussian_contributions: over the pixels p Gaussian i
        was blended into, sum_p w_i, sum_p g(p) w_i with g = pixel_weight [H,W] (1 when None), max_p w_i
        and the pixel count, w_i = alpha_i T_i.  `out` [P,4] accumulates views into one buffer."""
        shs, colors_precomp, scales, rotations, cov3D = _checked_inputs(shs, colors_precomp, scales, rotations,
                                                                        cov3D_precomp)
        s = self.raster_settings
        args = _forward_args(s, means3D, colors_precomp, opacities, scales, rotations, cov3D, shs)
        with _antialiased(self.antialiasing):
            num_rendered, color, radii, _depth, geom, binning, img = _C.rasterize_gaussians(*args)
        stats = _C.gaussian_contributions(radii, geom, binning, img, num_rendered, means3D.size(0), s.image_width,
                                          s.image_height, pixel_weight=pixel_weight, out=out)
        return color, radii, stats

    @torch.no_grad()
    def render_depth_normal(self, means3D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None):
        """Forward only, with the auxiliary outputs of BASELINE configs[4]: returns (color [3,H,W],
        radii [P], depth [1,H,W], normal [3,H,W]).  The normal map (no reference counterpart) blends
        each Gaussian's view-space smallest-scale axis, facing the camera, like depth: sum of
        alpha*T*n, no background (include/rain_raster.h RR_FLAG_AUX_NORMAL).  Needs scales/rotations."""
        if self.absgrad:
            raise ValueError(_MSG_ABS.format("render_depth_normal", "the aux normal frame"))
        if (shs is None) == (colors_precomp is None):
            raise Exception(_MSG_COLOR)
        if scales is None or rotations is None:
            raise Exception(_MSG_NORMAL)
        shs, colors_precomp, cov3D = _absent_as_empty(shs, colors_precomp, None)
        args = _forward_args(self.raster_settings, means3D, colors_precomp, opacities, scales, rotations, cov3D, shs)
        with _antialiased(self.antialiasing):
            out = _C.rasterize_gaussians_aux(*args)
        return out[1], out[2], out[3], out[4]


__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "_RasterizeGaussians",
           "_RasterizeGaussiansDepth", "_RasterizeGaussiansCamera", "_RasterizeGaussiansNormal", "_RasterizeGaussiansDist", "_C"]
