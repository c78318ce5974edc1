"""MI355X ``_C`` module: same functions, argument orders and return tuples as the reference's
pybind extension (submodules/diff_gaussian_rasterization/ext.cpp:4-7, rasterize_points.cu:24-212),
implemented over the C ABI in include/rain_raster.h.

* ``rasterize_gaussians``           ≙ RasterizeGaussiansCUDA          (rasterize_points.cu:24-108)
* ``rasterize_gaussians_backward``  ≙ RasterizeGaussiansBackwardCUDA  (rasterize_points.cu:110-191)
* ``mark_visible``                  ≙ markVisible                     (rasterize_points.cu:193-212)

Beyond the reference (opt-in): ``rasterize_gaussians_backward_depth`` also takes gradients of the
depth map and of the accumulated alpha, and ``accumulated_alpha`` returns that alpha map
(include/rain_raster.h rr_backward_aux, rr_render_alpha); ``rasterize_gaussians_backward_normal``
takes a gradient of the aux normal map of ``rasterize_gaussians_aux`` as well (rr_backward_aux_normal);
``rasterize_gaussians_dist`` also renders the depth-moment maps of the distortion loss and
``rasterize_gaussians_backward_dist`` takes their gradient (rr_forward_render_dist, rr_backward_aux_dist);
``rasterize_gaussians_backward_camera`` is ``rasterize_gaussians_backward_depth`` that also returns the
gradients of the camera arrays (viewmatrix, projmatrix, campos; rr_backward_camera).
``antialiased()`` makes the calls inside its block render and differentiate anti-aliased frames
(RR_FLAG_ANTIALIAS: the opacity compensation of the 2D dilation).
``absgrad()`` makes the backward calls inside its block also sum the absolute per-pixel mean2D gradients
(RR_FLAG_ABSGRAD; AbsGS, gsplat's ``absgrad``), and ``rasterize_gaussians_backward_abs`` returns them.

Differences that are deliberate and invisible to callers: scratch buffers are sized by the C
ABI's *_bytes() queries instead of grown through std::function callbacks; outputs the kernels
write completely are allocated with torch.empty (the reference zero-fills them first); scratch and
outputs live on ``means3D.device`` and kernels run on torch's current stream of that device (the
reference uses the current device and the legacy default stream).

This module holds the reference signatures, the dtype / device checks, the output allocation, the P == 0
results and the thread switches; the native call sequences (the counted two-stage forward, the choice of
backward entry point) are rain_amd/_raster_driver.py's.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import threading

import torch

from .. import _native as N
from .. import _raster_driver as driver
from .._raster_driver import ptr as _ptr  # (tests and tools import it from here under this name)

NUM_CHANNELS = 3

# Exact tile culling (include/rain_raster.h RR_FLAG_NO_TILE_CULLING): identical outputs, fewer
# (tile, Gaussian) pairs.  RAIN_TILE_CULLING=0 restores the reference's bounding-square binning.
TILE_CULLING = os.environ.get("RAIN_TILE_CULLING", "1") != "0"
# Early-stop binning (include/rain_raster.h RR_FLAG_FULL_BINNING): identical outputs, tile lists
# cut past saturation.  False (or RAIN_EARLY_STOP=0) bins every pair (full per-tile lists).
EARLY_STOP = os.environ.get("RAIN_EARLY_STOP", "1") != "0"


def frame_flags():
    return (0 if TILE_CULLING else N.RR_FLAG_NO_TILE_CULLING) | (0 if EARLY_STOP else N.RR_FLAG_FULL_BINNING)


def _dev_f32(t, device, name):
    if t is None or t.numel() == 0:
        return None
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be a float32 tensor (got {t.dtype})")
    if t.device != device:
        raise RuntimeError(f"{name} must be on {device} (got {t.device})")
    return t.contiguous()


def _require_device(means3D):
    if means3D.device.type != "cuda":
        raise RuntimeError("rain_amd rasterizer: tensors must be on a HIP device (no CPU fallback)")
    return means3D.device


# Anti-aliased rendering (include/rain_raster.h RR_FLAG_ANTIALIAS).  The functions below keep the
# reference's argument lists, so the switch travels beside them: inside `with antialiased():` every
# rasterize_gaussians* call of this thread, forward or backward, builds its frame with the flag.  A
# frame's backward must run under the value its forward ran under (the autograd classes record it).
_SWITCH = threading.local()


def antialiasing_on() -> bool:
    return bool(getattr(_SWITCH, "antialiasing", False))


@contextlib.contextmanager
def antialiased(on=True):
    prev = antialiasing_on()
    _SWITCH.antialiasing = bool(on)
    try:
        yield
    finally:
        _SWITCH.antialiasing = prev


# Absolute-gradient densification statistics (include/rain_raster.h RR_FLAG_ABSGRAD): the same kind of
# switch.  It is a flag of the backward's frame; the forward calls accept and ignore it.
def absgrad_on() -> bool:
    return bool(getattr(_SWITCH, "absgrad", False))


@contextlib.contextmanager
def absgrad(on=True):
    prev = absgrad_on()
    _SWITCH.absgrad = bool(on)
    try:
        yield
    finally:
        _SWITCH.absgrad = prev


def _frame(P, degree, M, W, H, tan_fovx, tan_fovy, scale_modifier, low_pass, prefiltered, debug):
    flags = frame_flags() | (N.RR_FLAG_ANTIALIAS if antialiasing_on() else 0) | \
        (N.RR_FLAG_ABSGRAD if absgrad_on() else 0)
    return N.RRFrame(int(P), int(degree), int(M), int(W), int(H), float(tan_fovx), float(tan_fovy),
                     float(scale_modifier), float(low_pass), int(bool(prefiltered)), int(bool(debug)), flags)


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                        prefiltered, debug, low_pass):
    out = _rasterize(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                     viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                     prefiltered, debug, low_pass, False)
    return out[:4] + out[5:]


def rasterize_gaussians_aux(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                            viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                            prefiltered, debug, low_pass):
    """rasterize_gaussians plus the aux normal map (include/rain_raster.h RR_FLAG_AUX_NORMAL; no
    reference counterpart): returns (num_rendered, color, radii, depth, normal [3,H,W], geomBuffer,
    binningBuffer, imgBuffer).  The buffers are valid for rasterize_gaussians_backward."""
    return _rasterize(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                      viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                      prefiltered, debug, low_pass, True)


def rasterize_gaussians_dist(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                             viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                             prefiltered, debug, low_pass, dist_near, dist_far, normal=False):
    """rasterize_gaussians plus the depth-moment maps moments [2,H,W] = (sum w m, sum w m^2), w = alpha T,
    m the mapped depth (include/rain_raster.h rr_forward_render_dist: NDC depth for 0 < dist_near <
    dist_far, metric depth for 0, 0), and with `normal` the aux normal map: returns (num_rendered, color,
    radii, depth, normal [3,H,W] or None, moments, geomBuffer, binningBuffer, imgBuffer).  The buffers are
    valid for rasterize_gaussians_backward_dist."""
    out = _rasterize(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                     viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                     prefiltered, debug, low_pass, bool(normal), (float(dist_near), float(dist_far)))
    return out[:5] + (out[8],) + out[5:8]


def _rasterize(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
               viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
               prefiltered, debug, low_pass, normal, dist=None):
    """(num_rendered, color, radii, depth, normal, geom, binning, img) and, with dist = (near, far), the
    moment maps as a ninth entry."""
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    P = means3D.size(0)
    H, W = int(image_height), int(image_width)
    device = _require_device(means3D)
    fopts = dict(dtype=torch.float32, device=device)
    u8 = dict(dtype=torch.uint8, device=device)
    if P == 0:
        return (0, torch.zeros((NUM_CHANNELS, H, W), **fopts), torch.zeros((0,), dtype=torch.int32, device=device),
                torch.zeros((1, H, W), **fopts), torch.zeros((3, H, W), **fopts) if normal else None,
                torch.empty((0,), **u8), torch.empty((0,), **u8), torch.empty((0,), **u8)) + \
            ((torch.zeros((2, H, W), **fopts),) if dist is not None else ())
    L = N.raster()
    M = sh.size(1) if sh.size(0) != 0 else 0
    keep = dict(
        bg=_dev_f32(background, device, "bg"), means3D=_dev_f32(means3D, device, "means3D"),
        colors=_dev_f32(colors, device, "colors_precomp"), opacity=_dev_f32(opacity, device, "opacities"),
        scales=_dev_f32(scales, device, "scales"), rotations=_dev_f32(rotations, device, "rotations"),
        cov3D=_dev_f32(cov3D_precomp, device, "cov3D_precomp"), view=_dev_f32(viewmatrix, device, "viewmatrix"),
        proj=_dev_f32(projmatrix, device, "projmatrix"), sh=_dev_f32(sh, device, "sh"),
        campos=_dev_f32(campos, device, "campos"))
    frame = _frame(P, degree, M, W, H, tan_fovx, tan_fovy, scale_modifier, low_pass, prefiltered, debug)
    if normal:
        frame.flags |= N.RR_FLAG_AUX_NORMAL
    _cam_keep, cam = driver.camera_block(keep["bg"], keep["view"], keep["proj"], keep["campos"])
    gs = N.RRGaussians(_ptr(keep["means3D"]), _ptr(keep["sh"]), _ptr(keep["colors"]), _ptr(keep["opacity"]),
                       _ptr(keep["scales"]), _ptr(keep["rotations"]), _ptr(keep["cov3D"]))
    out_color = torch.empty((NUM_CHANNELS, H, W), **fopts)
    out_depth = torch.empty((1, H, W), **fopts)
    out_normal = torch.empty((3, H, W), **fopts) if normal else None
    moments = torch.empty((2, H, W), **fopts) if dist is not None else None
    radii = torch.empty((P,), dtype=torch.int32, device=device)
    geom = torch.empty((L.rr_geometry_bytes(P),), **u8)
    img = torch.empty((L.rr_image_bytes(W, H),), **u8)
    # num_rendered is the reference's value (sum of bounding-square tile counts)
    binning, num_rendered = driver.render_counted(
        L, frame, cam, gs, radii, geom, img, None, out_color, out_depth, out_normal, moments, dist,
        N.stream_of(means3D), "rasterize_gaussians" if dist is None else "rasterize_gaussians_dist")
    return (num_rendered, out_color, radii, out_depth, out_normal, geom, binning, img) + \
        ((moments,) if dist is not None else ())


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree,
                                 campos, geomBuffer, R, binningBuffer, imageBuffer, debug, low_pass):
    return _backward("rasterize_gaussians_backward", background, means3D, radii, colors, scales,
                     rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                     dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, low_pass)


def rasterize_gaussians_backward_abs(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                     cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh,
                                     degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, low_pass):
    """rasterize_gaussians_backward with RR_FLAG_ABSGRAD: its 8 tensors (unchanged) plus dL_dmeans2D_abs
    [P,3], the sums over a Gaussian's pixels of the absolute per-pixel dL/dmeans2D terms (z stays 0;
    no reference counterpart).  A 9-tuple."""
    with absgrad(True):
        return _backward("rasterize_gaussians_backward_abs", background, means3D, radii, colors, scales,
                         rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                         dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, low_pass,
                         want_abs=True)


def rasterize_gaussians_backward_depth(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                       cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh,
                                       degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, low_pass,
                                       dL_dout_depth, dL_dout_alpha):
    """rasterize_gaussians_backward with gradients of the depth map D = sum alpha_i T_i z_i
    (dL_dout_depth [1,H,W]) and of the accumulated alpha A = 1 - T_final (dL_dout_alpha [1,H,W])
    added to the colour's (no reference counterpart; rr_backward_aux).  Any of the three output
    gradients may be an empty tensor ("absent": zero), but not all of them.  Same 8-tuple."""
    return _backward("rasterize_gaussians_backward_depth", background, means3D, radii, colors, scales,
                     rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                     dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, low_pass,
                     dL_dout_depth, dL_dout_alpha)


def rasterize_gaussians_backward_camera(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                        cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh,
                                        degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, low_pass,
                                        dL_dout_depth, dL_dout_alpha):
    """rasterize_gaussians_backward_depth plus the gradients of the camera arrays (rr_backward_camera):
    returns its 8 tensors and (d_viewmatrix [4,4], d_projmatrix [4,4], d_campos [3]), the gradients of
    `viewmatrix`, `projmatrix` and `campos` as three independent inputs, in their memory layout.  The
    view matrix is reached through the EWA Jacobian, its 3x3 block and the view depth of the depth map;
    the projection through means2D (its z row gets 0); campos through the SH view direction (0 with
    precomputed colours).  The depth and alpha gradients may both be empty (a colour-only loss).
    Raises inside antialiased(): camera gradients of an anti-aliased frame are a follow-up."""
    if antialiasing_on():
        raise RuntimeError("rasterize_gaussians_backward_camera: camera gradients do not combine with "
                           "antialiasing yet (RR_FLAG_ANTIALIAS)")
    return _backward("rasterize_gaussians_backward_camera", background, means3D, radii, colors, scales,
                     rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                     dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, low_pass,
                     dL_dout_depth, dL_dout_alpha, camera=True)


def rasterize_gaussians_backward_normal(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                        cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh,
                                        degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, low_pass,
                                        dL_dout_depth, dL_dout_alpha, dL_dout_normal):
    """rasterize_gaussians_backward_depth plus a gradient of the aux normal map N = sum alpha_i T_i n_i
    (dL_dout_normal [3,H,W]; rr_backward_aux_normal).  The buffers must come from
    rasterize_gaussians_aux (its geomBuffer holds the per-Gaussian normals).  Any of the four output
    gradients may be an empty tensor ("absent": zero), but not all of them; with dL_dout_normal
    absent this is rasterize_gaussians_backward_depth.  The normal reaches dL_drotations directly and
    every geometric gradient through alpha_i; scales, means3D and the camera get nothing from n_i
    itself (the axis choice and the flip towards the camera are constants).  Same 8-tuple."""
    return _backward("rasterize_gaussians_backward_normal", background, means3D, radii, colors, scales,
                     rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                     dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, low_pass,
                     dL_dout_depth, dL_dout_alpha, dL_dout_normal)


def rasterize_gaussians_backward_dist(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                      cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh,
                                      degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, low_pass,
                                      dL_dout_depth, dL_dout_alpha, dL_dout_normal, dL_dout_moments, dist_near,
                                      dist_far):
    """rasterize_gaussians_backward_normal plus a gradient of the depth-moment maps (dL_dout_moments
    [2,H,W] = dL/dM1, dL/dM2; rr_backward_aux_dist) of a frame rendered by rasterize_gaussians_dist with
    the same dist_near / dist_far (and, for a normal gradient, normal=True).  Any of the five output
    gradients may be an empty tensor ("absent": zero), but not all of them; with dL_dout_moments absent
    this is rasterize_gaussians_backward_normal.  The moments reach dL_dmeans3D through the view depth
    and every geometric gradient through alpha_i.  Same 8-tuple."""
    return _backward("rasterize_gaussians_backward_dist", background, means3D, radii, colors, scales,
                     rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                     dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug, low_pass,
                     dL_dout_depth, dL_dout_alpha, dL_dout_normal, dL_dout_moments, (float(dist_near), float(dist_far)))


def _present(t):
    return t is not None and t.numel() != 0


def _backward(label, background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
              projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer,
              imageBuffer, debug, low_pass, dL_dout_depth=None, dL_dout_alpha=None, dL_dout_normal=None,
              dL_dout_moments=None, dist=(0.0, 0.0), camera=False, want_abs=False):
    """Every rasterize_gaussians_backward* above (`label`: its name, for error messages).  An absent map
    goes to the library as NULL, and the library picks the kernel variants from which maps are there."""
    P = means3D.size(0)
    nrm = _present(dL_dout_normal)
    maps = (("dL_dout_color", dL_dout_color, NUM_CHANNELS), ("dL_dout_depth", dL_dout_depth, 1),
            ("dL_dout_alpha", dL_dout_alpha, 1), ("dL_dout_normal", dL_dout_normal, 3),
            ("dL_dout_moments", dL_dout_moments, 2))
    aux = any(_present(t) for _, t, _ in maps[1:])
    if aux:  # the frame's size from whichever output gradient is there
        ref = next(t for _, t, _ in maps if _present(t))
        H, W = ref.size(-2), ref.size(-1)
        for name, t, c in maps:
            if _present(t) and t.numel() != c * H * W:
                raise RuntimeError(f"{name} must have {c} x {H} x {W} elements (got {tuple(t.shape)})")
    else:
        H, W = dL_dout_color.size(1), dL_dout_color.size(2)
    M = sh.size(1) if sh.size(0) != 0 else 0
    device = _require_device(means3D)
    fopts = dict(dtype=torch.float32, device=device)
    if P == 0:
        z = lambda *s: torch.zeros(s, **fopts)  # noqa: E731
        return (z(0, 3), z(0, NUM_CHANNELS), z(0, 1), z(0, 3), z(0, 6), z(0, M, 3), z(0, 3), z(0, 4)) + \
            ((z(4, 4), z(4, 4), z(3)) if camera else ()) + ((z(0, 3),) if want_abs else ())
    L = N.raster()
    keep = dict(
        bg=_dev_f32(background, device, "bg"), means3D=_dev_f32(means3D, device, "means3D"),
        colors=_dev_f32(colors, device, "colors_precomp"), scales=_dev_f32(scales, device, "scales"),
        rotations=_dev_f32(rotations, device, "rotations"), cov3D=_dev_f32(cov3D_precomp, device, "cov3D_precomp"),
        view=_dev_f32(viewmatrix, device, "viewmatrix"), proj=_dev_f32(projmatrix, device, "projmatrix"),
        sh=_dev_f32(sh, device, "sh"), campos=_dev_f32(campos, device, "campos"), radii=radii.contiguous())
    dpix, ddepth, dalpha, dnormal, dmoments = (_dev_f32(t, device, name) for name, t, _ in maps)
    # opacities are not needed by the backward (the reference does not pass them either; an anti-aliased
    # frame's backward reads the compensated opacity back from the geometry buffer)
    frame = _frame(P, degree, M, W, H, tan_fovx, tan_fovy, scale_modifier, low_pass, False, debug)
    if nrm:  # the forward was rasterize_gaussians_aux
        frame.flags |= N.RR_FLAG_AUX_NORMAL
    _cam_keep, cam = driver.camera_block(keep["bg"], keep["view"], keep["proj"], keep["campos"])
    gs = N.RRGaussians(_ptr(keep["means3D"]), _ptr(keep["sh"]), _ptr(keep["colors"]), None,
                       _ptr(keep["scales"]), _ptr(keep["rotations"]), _ptr(keep["cov3D"]))
    # dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations
    res = tuple(torch.empty(shape, **fopts)
                for shape in ((P, 3), (P, NUM_CHANNELS), (P, 1), (P, 3), (P, 6), (P, M, 3), (P, 3), (P, 4)))
    grads = N.RRGrads(*[_ptr(t) for t in res])
    if want_abs:
        res = res + (torch.empty((P, 3), **fopts),)
        grads.dL_dmeans2D_abs = _ptr(res[8])
    ws = torch.empty((L.rr_backward_workspace_bytes(P),), dtype=torch.uint8, device=device)
    cam_res = None
    if camera:
        if nrm or _present(dL_dout_moments):
            raise RuntimeError("camera gradients do not combine with dL_dout_normal / dL_dout_moments yet")
        cam_res = (torch.empty((4, 4), **fopts), torch.empty((4, 4), **fopts), torch.empty((3,), **fopts))
    driver.backward(L, frame, cam, gs, keep["radii"], geomBuffer, imageBuffer, binningBuffer, R, dpix, ddepth, dalpha,
                    dnormal, dmoments, dist, ws, grads, cam_res, N.stream_of(means3D), label)
    return res + cam_res if camera else res


def accumulated_alpha(imageBuffer, H, W):
    """Accumulated alpha A = 1 - T_final = sum alpha_i T_i [1,H,W] of the frame last rendered into
    `imageBuffer` (rasterize_gaussians' imgBuffer); zeros for the empty buffer of a P == 0 frame."""
    H, W = int(H), int(W)
    device = _require_device(imageBuffer)
    out = torch.zeros((1, H, W), dtype=torch.float32, device=device)
    if imageBuffer.numel() == 0:
        return out
    frame = _frame(1, 0, 0, W, H, 1.0, 1.0, 1.0, 0.3, False, False)
    L = N.raster()
    if imageBuffer.numel() < L.rr_image_bytes(W, H):
        raise RuntimeError("accumulated_alpha: imageBuffer is smaller than a frame of this size")
    N.check(L.rr_render_alpha(ctypes.byref(frame), _ptr(imageBuffer), _ptr(out), N.stream_of(imageBuffer)),
            "accumulated_alpha")
    return out


def gaussian_contributions(radii, geomBuffer, binningBuffer, imageBuffer, num_rendered, P, W, H, pixel_weight=None,
                           out=None):
    """Per-Gaussian blend-contribution statistics of the frame last rendered into the buffers
    (rasterize_gaussians' radii, geomBuffer, binningBuffer, imgBuffer and num_rendered;
    include/rain_raster.h rr_contributions).  With w_i(p) = alpha_i(p) T_i(p) over the pixels the forward
    blended Gaussian i into, returns (sum_w [P], sum_gw [P], max_w [P], count [P] int32): sum_p w, sum_p g w
    with g = pixel_weight [H,W] (either sign; 1 everywhere when None), max_p w, and the number of pixels.
    The four are views of one [P,4] float32 buffer (count through its bits; it wraps past 2^32 hits).
    Passing `out`, such a [P,4] buffer, accumulates this frame into it (sums add, max_w takes the max,
    counts add) and returns views of it.  No gradient flows; no CPU fallback."""
    P, W, H = int(P), int(W), int(H)
    device = _require_device(radii)
    if out is None:
        buf = torch.empty((P, 4), dtype=torch.float32, device=device)  # written completely
    else:
        buf = out
        if buf.dtype != torch.float32 or tuple(buf.shape) != (P, 4) or not buf.is_contiguous() or buf.device != device:
            raise RuntimeError(f"out must be a contiguous float32 [{P}, 4] tensor on {device}")
    views = (buf[:, 0], buf[:, 1], buf[:, 2], buf.view(torch.int32)[:, 3])
    if P == 0:
        return views
    g = _dev_f32(pixel_weight, device, "pixel_weight")
    if g is not None and g.numel() != H * W:
        raise RuntimeError(f"pixel_weight must have {H} x {W} elements (got {tuple(g.shape)})")
    L = N.raster()
    if radii.numel() != P or geomBuffer.numel() < L.rr_geometry_bytes(P) or \
            imageBuffer.numel() < L.rr_image_bytes(W, H):
        raise RuntimeError("gaussian_contributions: radii / buffers are not those of a P-Gaussian frame of this size")
    radii = radii.contiguous()
    frame = _frame(P, 0, 0, W, H, 1.0, 1.0, 1.0, 0.3, False, False)
    N.check(L.rr_contributions(ctypes.byref(frame), _ptr(radii), _ptr(geomBuffer), _ptr(imageBuffer),
                                        _ptr(binningBuffer), int(num_rendered), _ptr(g), 0 if out is None else 1,
                                        _ptr(buf), N.stream_of(radii)),
            "gaussian_contributions")
    return views


def mark_visible(means3D, viewmatrix, projmatrix):
    P = means3D.size(0)
    device = _require_device(means3D)
    present = torch.zeros((P,), dtype=torch.bool, device=device)
    if P != 0:
        m = _dev_f32(means3D, device, "means3D")
        v = _dev_f32(viewmatrix, device, "viewmatrix")
        p = _dev_f32(projmatrix, device, "projmatrix")
        N.check(N.raster().rr_mark_visible(P, _ptr(m), _ptr(v), _ptr(p), _ptr(present), N.stream_of(means3D)),
                "mark_visible")
    return present


def debug_views(geomBuffer, binningBuffer, imageBuffer, num_rendered, P, W, H):
    """Copies of the forward's private binning/image state (tests only): point_list [8 num_pairs]
    (4 slots per pair in the phase-A region [0, 4L) and the phase-B region [4L, 8L); tile t's list
    is point_list[ranges[t, 0]:ranges[t, 1]]),
    ranges [T,2], tile_max [T], final_T [H,W], n_contrib [H,W], splats [P,12]."""
    f = _frame(P, 0, 0, W, H, 1.0, 1.0, 1.0, 0.3, False, False)
    num_rendered = frame_stats(geomBuffer, imageBuffer, P, W, H)["num_pairs"]
    v = N.RRDebugViews()
    N.check(N.raster().rr_debug_get_views(ctypes.byref(f), _ptr(geomBuffer), _ptr(imageBuffer), _ptr(binningBuffer),
                                          int(num_rendered), ctypes.byref(v)), "debug_views")
    dev = geomBuffer.device
    gx, gy = (W + 15) // 16, (H + 15) // 16
    T = gx * gy

    def grab(ptr, n, dtype, src):
        out = torch.empty((n,), dtype=dtype, device=dev)
        if n:
            base = src.data_ptr()
            off = ptr - base
            nbytes = n * out.element_size()
            assert 0 <= off and off + nbytes <= src.numel(), "debug view outside its buffer"
            out.view(torch.uint8).copy_(src[off:off + nbytes])
        return out

    return dict(
        # per-tile lists live at the ranges' absolute positions: 4 slots per (bin, Gaussian) pair
        # (phase A's region [0, 4L) and phase B's [4L, 8L); clamped to the buffer)
        point_list=grab(v.point_list, min(8 * num_rendered, (binningBuffer.numel() - (v.point_list -
                                          binningBuffer.data_ptr())) // 4), torch.int32, binningBuffer)
        if num_rendered else torch.empty((0,), dtype=torch.int32, device=dev),
        ranges=grab(v.ranges, 2 * T, torch.int32, imageBuffer).view(T, 2),
        tile_max=grab(v.tile_max, T, torch.int32, imageBuffer),
        final_T=grab(v.final_T, H * W, torch.float32, imageBuffer).view(H, W),
        n_contrib=grab(v.n_contrib, H * W, torch.int32, imageBuffer).view(H, W),
        splats=grab(v.splats, 12 * P, torch.float32, geomBuffer).view(P, 12))


def frame_stats(geomBuffer, imageBuffer, P, W, H):
    """(L, visible count V, L_eff = sum of per-tile max n_contrib, T) of the last forward — bench/tests."""
    f = _frame(P, 0, 0, W, H, 1.0, 1.0, 1.0, 0.3, False, False)
    st = N.RRFrameStats()
    N.check(N.raster().rr_read_frame_stats(ctypes.byref(f), _ptr(geomBuffer), _ptr(imageBuffer), ctypes.byref(st),
                                           N.stream_of(geomBuffer)), "frame_stats")
    return dict(num_rendered=st.num_rendered, num_visible=st.num_visible, l_eff=st.l_eff, tiles=st.tiles,
                num_pairs=st.num_pairs, num_binned=st.num_binned, phase_b_pairs=st.phase_b_pairs,
                phase_b_slots=st.phase_b_slots)
