"""Training-step rasterizer over GaussianModel's raw parameters (include/rain_raster.h
RR_FLAG_RAW_PARAMS).

The reference's iteration (train.py:109-134) goes: getters (exp / normalize / sigmoid / cat,
gaussian_model.py:85-105) -> render() -> rasterizer -> autograd back through the getters into six
leaf gradients, plus masked scatters for the densification statistics.  Here the getters run
inside the rasterizer's preprocess, the chain rule through them runs inside its per-Gaussian
backward kernel, which writes the six raw-parameter gradients straight into their (flat) .grad
buffers and folds in the densification statistics — no SH concatenation, no autograd graph, no
[P,3] means2D tensor.  The arithmetic is the same as the reference-API path (rain_amd.renderer /
diff_gaussian_rasterization) on the activated tensors; tests/test_fused_gpu.py compares the two.

This module holds RawFrame / NextFrame, the raw rr_grads packing, the argument checks and the autograd
classes; the native call sequences (the one-call forward with its retry, the counted two-stage forward, the
workspace registration, the choice of backward entry point) are rain_amd/_raster_driver.py's.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import torch

from . import _native as N
from . import _raster_driver as driver
# names tests, tools and bench.py use from this module; forward_params / forward_next look
# _register_workspace up here at call time (tests replace it)
from ._raster_driver import BinningCache, ptr as _p, register_workspace as _register_workspace
from .diff_gaussian_rasterization import _C


@dataclass
class RawFrame:
    """State a forward hands to its backward (the reference's saved tensors, __init__.py:85-87)."""
    frame: N.RRFrame
    cam: N.RRCamera
    gs: N.RRGaussians
    keep: tuple
    radii: torch.Tensor
    geom: torch.Tensor
    img: torch.Tensor
    binning: torch.Tensor
    num_rendered: int
    P: int
    M: int
    # the backward's accumulator workspace, zero-filled by the forward render
    # (rr_set_forward_workspace); the first backward uses it, a second one allocates its own
    ws: torch.Tensor | None = None
    # the aux normal map [3,H,W] of a frame rendered with normal=True (RR_FLAG_AUX_NORMAL), else None
    normal: torch.Tensor | None = None
    # the depth-moment maps [2,H,W] of a frame rendered with dist=(near, far), else None, and that pair
    moments: torch.Tensor | None = None
    dist: tuple | None = None


def forward(model, camera, bg: torch.Tensor, low_pass: float, scale_modifier: float = 1.0,
            cache: BinningCache | None = None, normal: bool = False, dist: tuple | None = None,
            antialiasing: bool = False):
    """Render `camera` from `model` (a GaussianModel) in raw-parameter mode.
    Returns (color [3,H,W], radii [P] int32, depth [1,H,W], RawFrame).  With `cache` the binning
    buffer is reused (see BinningCache) and must not be needed by an earlier frame's pending
    backward.  With `normal` the frame also renders the aux normal map (RR_FLAG_AUX_NORMAL), left in
    the RawFrame's `normal` field ([3,H,W]); backward(dL_dnormal=...) differentiates it.  Such a
    frame always runs its own preprocess (it cannot be the `next_frame` of an earlier backward).
    With `dist` = (dist_near, dist_far) the frame also renders the depth-moment maps of the distortion
    loss (rr_forward_render_dist), left in the RawFrame's `moments` field ([2,H,W]);
    backward(dL_dmoments=...) differentiates them.  It runs its own preprocess as well.
    With `antialiasing` the frame carries RR_FLAG_ANTIALIAS (the opacity compensation of the 2D
    dilation, include/rain_raster.h); its backward reads the flag from the RawFrame."""
    params = (model._xyz, model._features_dc, model._features_rest, model._opacity, model._scaling,
              model._rotation)
    return forward_params(params, model.active_sh_degree, int(camera.image_width), int(camera.image_height),
                          math.tan(camera.FoVx * 0.5), math.tan(camera.FoVy * 0.5), camera.world_view_transform,
                          camera.full_proj_transform, camera.camera_center, bg, low_pass, scale_modifier, cache,
                          normal, dist, antialiasing)


def forward_params(params, sh_degree: int, W: int, H: int, tanfovx: float, tanfovy: float, viewmatrix, projmatrix,
                   campos, bg: torch.Tensor, low_pass: float, scale_modifier: float = 1.0,
                   cache: BinningCache | None = None, normal: bool = False, dist: tuple | None = None,
                   antialiasing: bool = False):
    """forward() on explicit raw parameters (xyz, f_dc, f_rest, opacity, scaling, rotation) — the
    GaussianModel attributes before activation — and camera values as render() puts them in
    GaussianRasterizationSettings.  `normal`, `dist`, `antialiasing`: see forward()."""
    xyz = params[0]
    dev = xyz.device
    if dev.type != "cuda":
        raise RuntimeError("rain_amd.fused: tensors must be on a HIP device (no CPU fallback)")
    P = xyz.shape[0]
    H, W = int(H), int(W)
    f_dc, f_rest = params[1], params[2]
    M = 1 + f_rest.shape[1]
    D = int(sh_degree)
    L = N.raster()
    flags = N.RR_FLAG_RAW_PARAMS | _C.frame_flags() | (N.RR_FLAG_AUX_NORMAL if normal else 0) | \
        (N.RR_FLAG_ANTIALIAS if antialiasing else 0)
    frame = N.RRFrame(P, D, M, W, H, float(tanfovx), float(tanfovy), float(scale_modifier), float(low_pass), 0, 0,
                      flags)
    keep, cam = driver.camera_block(bg, viewmatrix, projmatrix, campos)
    # kernel argument order: xyz, f_dc, opacity, scaling, rotation, f_rest
    params = tuple(t.detach() for t in (xyz, f_dc, params[3], params[4], params[5], f_rest))
    for t in params:
        if not t.is_contiguous() or t.dtype != torch.float32:
            raise RuntimeError("rain_amd.fused: parameters must be contiguous float32")
    gs = driver.raw_gaussians(*params)
    fo = dict(dtype=torch.float32, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    color = torch.empty((3, H, W), **fo)
    depth = torch.empty((1, H, W), **fo)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    geom = torch.empty((L.rr_geometry_bytes(P),), **u8)
    img = torch.empty((L.rr_image_bytes(W, H),), **u8)
    stream = N.stream_of(xyz)
    ws = _register_workspace(L, P, dev)
    # the aux normal frame goes through the two-stage calls (rr_forward renders no normal map)
    nmap = torch.empty((3, H, W), **fo) if normal else None
    if dist is not None:
        dist = (float(dist[0]), float(dist[1]))
    mom = torch.empty((2, H, W), **fo) if dist is not None else None
    if P > 0 and cache is not None and not normal and dist is None:
        binning, num_rendered, _ = driver.render_one_call(L, frame, cam, gs, radii, geom, img, cache, color, depth,
                                                          stream, "fused forward")
        st = RawFrame(frame, cam, gs, (keep, params), radii, geom, img, binning, num_rendered, P, M, ws)
        return color, radii, depth, st
    if P > 0:
        binning, num_rendered = driver.render_counted(L, frame, cam, gs, radii, geom, img, cache, color, depth, nmap,
                                                      mom, dist, stream, "fused forward")
    else:
        binning, num_rendered = torch.empty((0,), **u8), 0
        color.copy_(bg.view(3, 1, 1).expand(3, H, W))
        depth.zero_()
        if normal:
            nmap.zero_()
        if mom is not None:
            mom.zero_()
    st = RawFrame(frame, cam, gs, (keep, params), radii, geom, img, binning, num_rendered, P, M, ws, nmap, mom, dist)
    return color, radii, depth, st


@dataclass
class NextFrame:
    """A frame whose preprocess the previous step's backward runs on the parameters it has just
    stepped (include/rain_raster.h rr_next_frame); forward_next() then renders it from the filled
    geometry buffer.  Built by prepare_next() before that backward."""
    frame: N.RRFrame
    cam: N.RRCamera
    keep: tuple
    radii: torch.Tensor
    geom: torch.Tensor
    P: int
    M: int
    W: int
    H: int
    desc: N.RRNextFrame = None

    def __post_init__(self):
        self.desc = N.RRNextFrame(ctypes.pointer(self.frame), ctypes.pointer(self.cam), _p(self.radii), _p(self.geom),
                                  self.geom.numel())


def prepare_next(model, camera, bg: torch.Tensor, low_pass: float, scale_modifier: float = 1.0,
                 antialiasing: bool = False) -> NextFrame:
    """The next frame's descriptor and output buffers (geometry buffer, radii) for `camera` at the
    model's current P, M and SH degree.  `antialiasing` is the next frame's own RR_FLAG_ANTIALIAS,
    independent of the flag of the frame whose backward runs this preprocess."""
    xyz = model._xyz
    dev = xyz.device
    P = xyz.shape[0]
    H, W = int(camera.image_height), int(camera.image_width)
    M = 1 + model._features_rest.shape[1]
    L = N.raster()
    frame = N.RRFrame(P, int(model.active_sh_degree), M, W, H, math.tan(camera.FoVx * 0.5),
                      math.tan(camera.FoVy * 0.5), float(scale_modifier), float(low_pass), 0, 0,
                      N.RR_FLAG_RAW_PARAMS | _C.frame_flags() | (N.RR_FLAG_ANTIALIAS if antialiasing else 0))
    keep, cam = driver.camera_block(bg, camera.world_view_transform, camera.full_proj_transform, camera.camera_center)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    geom = torch.empty((L.rr_geometry_bytes(P),), dtype=torch.uint8, device=dev)
    return NextFrame(frame, cam, keep, radii, geom, P, M, W, H)


def forward_next(nxt: NextFrame, model, cache: BinningCache | None = None):
    """forward() of a frame whose geometry the previous backward filled (rr_forward_from_geometry):
    the same outputs and RawFrame, without the preprocess launch."""
    L = N.raster()
    dev = nxt.geom.device
    P, W, H = nxt.P, nxt.W, nxt.H
    params = tuple(t.detach() for t in (model._xyz, model._features_dc, model._opacity, model._scaling,
                                        model._rotation, model._features_rest))
    gs = driver.raw_gaussians(*params)
    color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    depth = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    img = torch.empty((L.rr_image_bytes(W, H),), dtype=torch.uint8, device=dev)
    ws = _register_workspace(L, P, dev)
    binning, num_rendered, _ = driver.render_one_call(L, nxt.frame, nxt.cam, None, nxt.radii, nxt.geom, img, cache,
                                                      color, depth, N.stream_of(nxt.geom),
                                                      "fused forward (precomputed geometry)")
    st = RawFrame(nxt.frame, nxt.cam, gs, (nxt.keep, params), nxt.radii, nxt.geom, img, binning, num_rendered, P,
                  nxt.M, ws)
    return color, nxt.radii, depth, st


def backward(st: RawFrame, dL_dpix: torch.Tensor, grads: dict | None, stats: tuple | None = None,
             adam: "N.RRAdam | None" = None, dmeans2D: torch.Tensor | None = None, next_frame: NextFrame | None = None,
             dL_ddepth: torch.Tensor | None = None, dL_dalpha: torch.Tensor | None = None,
             dL_dnormal: torch.Tensor | None = None, dL_dmoments: torch.Tensor | None = None,
             cam_grads: tuple | None = None, absgrad: bool = False, dmeans2D_abs: torch.Tensor | None = None):
    """Write dLoss/d(raw parameter) into grads['xyz'|'f_dc'|'f_rest'|'opacity'|'scaling'|'rotation']
    (contiguous fp32 tensors of the parameter shapes, fully overwritten) and, if `stats` =
    (grad_accum [P,1], denom [P,1], max_radii2D [P]) is given, update the densification statistics
    in place for every Gaussian with radii > 0.  With `adam` (rain_amd.optim.FusedAdam.fused_step)
    the optimizer step is applied to the parameters in the same pass and `grads` may be None; with
    `next_frame` (prepare_next, needs `adam`) the same pass runs that frame's preprocess on the
    stepped parameters.
    `dmeans2D` ([P,3] contiguous fp32, optional) receives the screen-space (NDC) mean gradient —
    what the reference leaves in viewspace_points.grad — with z = 0.
    `dL_ddepth` / `dL_dalpha` ([1,H,W] or [H,W] fp32, optional): gradients of the depth map and of the
    accumulated alpha (accumulated_alpha()), added to the colour's in every output above, the
    statistics, the fused step and the next frame included (rr_backward_aux); `dL_dpix` may then
    be None.
    `dL_dnormal` ([3,H,W] fp32, optional): gradient of the aux normal map of a frame rendered with
    forward(normal=True), added likewise (rr_backward_aux_normal): it reaches the rotation directly
    and everything else through alpha_i.
    `dL_dmoments` ([2,H,W] fp32, optional): gradient of the depth-moment maps of a frame rendered with
    forward(dist=(near, far)), added likewise (rr_backward_aux_dist, with the frame's near / far): it
    reaches xyz through the view depth and everything else through alpha_i.
    `cam_grads` = (d_viewmatrix [4,4], d_projmatrix [4,4], d_campos [3]) (contiguous fp32, optional): they
    receive the gradients of the frame's three camera arrays (rr_backward_camera), fully overwritten.
    Colour, depth and alpha gradients only, and no `adam` / `next_frame`, and not on a frame rendered with
    antialiasing (a follow-up).
    `absgrad` (RR_FLAG_ABSGRAD; AbsGS, gsplat's absgrad): the blend backward also sums the absolute per-pixel
    mean-gradient terms; `stats` then accumulates the norm of those sums instead of the signed gradient's, and
    `dmeans2D_abs` ([P,3] contiguous fp32, optional) receives them (z = 0).  Every other output is unchanged.
    Colour gradient only: no aux map and no `cam_grads` (follow-ups)."""
    if absgrad:
        if dL_ddepth is not None or dL_dalpha is not None or dL_dnormal is not None or dL_dmoments is not None:
            raise RuntimeError("rain_amd.fused.backward: absgrad does not combine with depth / alpha / normal / "
                               "moments gradients yet (RR_FLAG_ABSGRAD)")
        if cam_grads is not None:
            raise RuntimeError("rain_amd.fused.backward: absgrad does not combine with camera gradients yet "
                               "(RR_FLAG_ABSGRAD)")
    elif dmeans2D_abs is not None:
        raise RuntimeError("rain_amd.fused.backward: dmeans2D_abs needs absgrad=True")
    if dmeans2D_abs is not None and (dmeans2D_abs.dtype != torch.float32 or not dmeans2D_abs.is_contiguous() or
                                     st is None or tuple(dmeans2D_abs.shape) != (st.P, 3)):
        raise RuntimeError("rain_amd.fused: dmeans2D_abs must be a contiguous float32 [P, 3] tensor")
    if cam_grads is not None:
        if st is not None and st.frame.flags & N.RR_FLAG_ANTIALIAS:
            raise RuntimeError("rain_amd.fused.backward: camera gradients do not combine with antialiasing yet "
                               "(RR_FLAG_ANTIALIAS)")
        if dL_dnormal is not None or dL_dmoments is not None:
            raise RuntimeError("rain_amd.fused.backward: camera gradients do not combine with dL_dnormal / "
                               "dL_dmoments yet")
        if adam is not None or next_frame is not None:
            raise RuntimeError("rain_amd.fused.backward: camera gradients do not combine with the fused optimizer "
                               "step / the next frame")
        for t, shape in zip(cam_grads, ((4, 4), (4, 4), (3,))):
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
                raise RuntimeError("rain_amd.fused: cam_grads must be contiguous float32 [4,4], [4,4], [3] tensors")
    if st.P == 0:
        if cam_grads is not None:
            for t in cam_grads:
                t.zero_()
        return
    L = N.raster()
    aux = dL_ddepth is not None or dL_dalpha is not None or dL_dnormal is not None or dL_dmoments is not None
    if dL_dmoments is not None and st.dist is None:
        raise RuntimeError("rain_amd.fused.backward: dL_dmoments needs a frame rendered with forward(dist=(near, far))")
    if dL_dpix is None and not aux:
        raise RuntimeError("rain_amd.fused.backward: no output gradient given")
    npix = st.frame.width * st.frame.height
    maps = [None, None, None, None]
    if aux:
        for i, (name, t, c) in enumerate((("dL_ddepth", dL_ddepth, 1), ("dL_dalpha", dL_dalpha, 1),
                                          ("dL_dnormal", dL_dnormal, 3), ("dL_dmoments", dL_dmoments, 2))):
            if t is not None:
                if t.dtype != torch.float32 or t.numel() != c * npix:
                    raise RuntimeError(f"rain_amd.fused: {name} must be a float32 [{c}, H, W] tensor")
                maps[i] = t.contiguous()
    dpix = dL_dpix.contiguous() if dL_dpix is not None else next(m for m in maps if m is not None)
    names = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
    if grads is None:
        if adam is None:
            raise RuntimeError("rain_amd.fused.backward: nothing to do (no gradients requested, no optimizer step)")
        grads = dict.fromkeys(names)
    for k in names:
        if grads[k] is not None and not grads[k].is_contiguous():
            raise RuntimeError(f"rain_amd.fused: grads[{k!r}] must be contiguous")
    acc, den, mr = stats if stats is not None else (None, None, None)
    if dmeans2D is not None and (not dmeans2D.is_contiguous() or tuple(dmeans2D.shape) != (st.P, 3)):
        raise RuntimeError("rain_amd.fused: dmeans2D must be a contiguous [P, 3] tensor")
    out = N.RRGrads(_p(dmeans2D), None, _p(grads["opacity"]), _p(grads["xyz"]), None, _p(grads["f_dc"]),
                    _p(grads["scaling"]), _p(grads["rotation"]), _p(grads["f_rest"]), _p(acc), _p(den), _p(mr),
                    ctypes.pointer(adam) if adam is not None else None,
                    ctypes.pointer(next_frame.desc) if next_frame is not None else None, _p(dmeans2D_abs))
    # the workspace the forward's render zero-filled serves this backward (which then skips its clear); absgrad
    # is a flag of this backward too: both go on a copy of the frame
    ws, st.ws = st.ws, None
    frame = driver.backward_frame(st.frame, ws is not None, N.RR_FLAG_ABSGRAD if absgrad else 0)
    if ws is None:
        ws = torch.empty((L.rr_backward_workspace_bytes(st.P),), dtype=torch.uint8, device=dpix.device)
    what = " (camera)" if cam_grads is not None else " (distortion)" if maps[3] is not None else \
        " (normal)" if maps[2] is not None else " (depth)" if aux else ""
    driver.backward(L, frame, st.cam, st.gs, st.radii, st.geom, st.img, st.binning, st.num_rendered,
                    dpix if dL_dpix is not None else None, maps[0], maps[1], maps[2], maps[3], st.dist, ws, out,
                    cam_grads, N.stream_of(dpix), "fused backward" + what)


def accumulated_alpha(st: RawFrame) -> torch.Tensor:
    """A = 1 - T_final = sum alpha_i T_i [1,H,W] of the frame `st` was rendered from."""
    H, W = st.frame.height, st.frame.width
    if st.P == 0:
        return torch.zeros((1, H, W), dtype=torch.float32, device=st.radii.device)
    return _C.accumulated_alpha(st.img, H, W)


_RAW_INPUTS = 18  # forward inputs of the raw-parameter classes (RasterizeRawParamsDist: three more)


def _raw_forward(ctx, inputs, aux=True, normal=False, dist=None, camera=False):
    """The forward of the five classes below on their 18 common `inputs`: (color, radii, depth), with `aux`
    the accumulated alpha as well (depth then carries gradients), then the aux normal map with `normal`
    (None without it, in a dist frame), then the moment maps with `dist` = (near, far).  `camera`: the three
    camera arrays are differentiable inputs.  Inside `with _C.antialiased():` (the classes keep their 18
    inputs, so the switch travels beside them) the frame, and with it its backward, carries RR_FLAG_ANTIALIAS."""
    antialiasing = _C.antialiasing_on()
    ctx.absgrad = _C.absgrad_on()  # (_C.absgrad) the backward then leaves means2D.absgrad
    if ctx.absgrad and (aux or camera):
        raise ValueError("render(absgrad=True) does not combine with depth_grad / normal_grad / dist_grad / "
                         "pose_grad yet (follow-up: absolute-gradient statistics with those gradients)")
    ctx.means2D = inputs[6] if ctx.absgrad else None  # a plain reference: the attribute goes on this object
    if camera and antialiasing:
        raise ValueError("render(pose_grad=True) does not combine with antialiasing yet (follow-up: camera-pose "
                         "gradients of an anti-aliased frame)")
    (xyz, f_dc, f_rest, opacity, scaling, rotation, _means2D, sh_degree, W, H, tanfovx, tanfovy, viewmatrix,
     projmatrix, campos, bg, low_pass, scale_modifier) = inputs
    if camera:
        viewmatrix, projmatrix, campos = (t.detach().to(torch.float32).contiguous()
                                          for t in (viewmatrix, projmatrix, campos))
        ctx.cam_shapes = (viewmatrix.shape, projmatrix.shape, campos.shape)
    color, radii, depth, st = forward_params((xyz, f_dc, f_rest, opacity, scaling, rotation), sh_degree, W, H,
                                             tanfovx, tanfovy, viewmatrix, projmatrix, campos, bg, low_pass,
                                             scale_modifier, normal=normal, dist=dist,
                                             antialiasing=bool(antialiasing))
    # the parameters as saved tensors (the reference saves its inputs, __init__.py:85-87): autograd's
    # version check then rejects a backward after they were modified in place.  The scratch
    # buffers and camera tensors are saved too, so that autograd frees them after a backward
    # that does not retain the graph; ctx keeps only the descriptors (plain structs).
    keep, _p6 = st.keep
    ctx.save_for_backward(xyz, f_dc, f_rest, opacity, scaling, rotation, st.radii, st.geom, st.img, st.binning,
                          st.ws, *keep)
    ctx.desc = (st.frame, st.cam, st.gs, st.num_rendered, st.P, st.M, st.dist)
    ctx.set_materialize_grads(False)  # an output the loss does not use gets no zero-filled gradient
    if not aux:
        ctx.mark_non_differentiable(radii, depth)
        return color, radii, depth
    ctx.mark_non_differentiable(radii)
    maps = (st.normal, st.moments) if dist is not None else (st.normal,) if normal else ()
    return (color, radii, depth, accumulated_alpha(st), *maps)


def _raw_backward(ctx, n_inputs, grad_color, grad_depth=None, grad_alpha=None, grad_normal=None, grad_moments=None,
                  aux=True, camera=False):
    """The backward of the five classes below: one gradient per forward input (`n_inputs`), None for the
    plain values.  An output the loss does not use arrives as None and goes to the library as an absent
    map; without `aux` (RasterizeRawParams) a missing colour gradient is zeros instead.  With `camera` the
    three camera inputs get rr_backward_camera's gradients when one of them needs any."""
    if aux and all(g is None for g in (grad_color, grad_depth, grad_alpha, grad_normal, grad_moments)):
        return (None,) * n_inputs
    # (raises if a parameter changed in place since the forward)
    xyz, f_dc, f_rest, opacity, scaling, rotation, radii, geom, img, binning, ws, *keep = ctx.saved_tensors
    frame, cam, gs, num_rendered, P, M, dist = ctx.desc
    p = (xyz, f_dc, opacity, scaling, rotation, f_rest)  # kernel order
    # the zero-filled workspace serves the first backward only (a retained graph's second one
    # allocates and clears its own)
    ws_first = ws if not getattr(ctx, "ws_used", False) else None
    ctx.ws_used = True
    st = RawFrame(frame, cam, gs, (tuple(keep), p), radii, geom, img, binning, num_rendered, P, M, ws_first,
                  dist=dist)
    fo = dict(dtype=torch.float32, device=xyz.device)
    if not aux and grad_color is None:  # the image unused by the loss (materialize_grads off)
        grad_color = torch.zeros((3, frame.height, frame.width), **fo)
    grads = dict(xyz=torch.empty_like(p[0]), f_dc=torch.empty_like(p[1]), opacity=torch.empty_like(p[2]),
                 scaling=torch.empty_like(p[3]), rotation=torch.empty_like(p[4]), f_rest=torch.empty_like(p[5]))
    d2 = torch.empty((P, 3), **fo)
    cg = None
    if camera and any(ctx.needs_input_grad[12:15]):  # else a fixed camera: the plain depth backward
        cg = (torch.empty((4, 4), **fo), torch.empty((4, 4), **fo), torch.empty((3,), **fo))
    dabs = torch.empty((P, 3), **fo) if ctx.absgrad else None
    backward(st, grad_color, grads, dmeans2D=d2, dL_ddepth=grad_depth, dL_dalpha=grad_alpha, dL_dnormal=grad_normal,
             dL_dmoments=grad_moments, cam_grads=cg, absgrad=ctx.absgrad, dmeans2D_abs=dabs)
    if ctx.absgrad:  # [P,3], gsplat's convention, beside the signed .grad
        ctx.means2D.absgrad = dabs
    # (in the inputs' own shapes: a flat [16] matrix gets a flat gradient)
    d_cam = tuple(g.view(s) for g, s in zip(cg, ctx.cam_shapes)) if cg is not None else (None,) * 3
    return (grads["xyz"], grads["f_dc"], grads["f_rest"], grads["opacity"], grads["scaling"], grads["rotation"], d2,
            None, None, None, None, None, *d_cam) + (None,) * (n_inputs - 15)


class RasterizeRawParams(torch.autograd.Function):
    """The rasterizer as an autograd function of GaussianModel's RAW parameters (render()'s fast
    path, rain_amd/renderer.py): the getters' activations (exp, normalize, sigmoid, the f_dc /
    f_rest concatenation — gaussian_model.py:85-105) run inside the preprocess and their chain rule
    inside the per-Gaussian backward, so autograd sees one node instead of the getters' elementwise
    kernels and the [P,16,3] feature copy.  Gradients: the six raw parameters and means2D (the
    NDC-space screen gradient the reference leaves in viewspace_points.grad); the same arithmetic
    as GaussianRasterizer over the activated tensors (tests/test_fused_gpu.py)."""

    @staticmethod
    def forward(ctx, xyz, f_dc, f_rest, opacity, scaling, rotation, means2D, sh_degree, W, H, tanfovx, tanfovy,
                viewmatrix, projmatrix, campos, bg, low_pass, scale_modifier):
        return _raw_forward(ctx, (xyz, f_dc, f_rest, opacity, scaling, rotation, means2D, sh_degree, W, H, tanfovx,
                                  tanfovy, viewmatrix, projmatrix, campos, bg, low_pass, scale_modifier), aux=False)

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, _grad_depth):
        return _raw_backward(ctx, _RAW_INPUTS, grad_color, aux=False)


class RasterizeRawParamsDepth(torch.autograd.Function):
    """RasterizeRawParams with differentiable depth and accumulated alpha (render(depth_grad=True)):
    returns (color, radii, depth, alpha) — depth = sum alpha_i T_i z_i, alpha = 1 - T_final, both
    [1,H,W] — and its backward adds their gradients to the colour's (rr_backward_aux).  An output
    the loss does not use arrives as None and goes to the library as an absent map."""

    @staticmethod
    def forward(ctx, xyz, f_dc, f_rest, opacity, scaling, rotation, means2D, sh_degree, W, H, tanfovx, tanfovy,
                viewmatrix, projmatrix, campos, bg, low_pass, scale_modifier):
        return _raw_forward(ctx, (xyz, f_dc, f_rest, opacity, scaling, rotation, means2D, sh_degree, W, H, tanfovx,
                                  tanfovy, viewmatrix, projmatrix, campos, bg, low_pass, scale_modifier))

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, grad_depth, grad_alpha):
        return _raw_backward(ctx, _RAW_INPUTS, grad_color, grad_depth, grad_alpha)


class RasterizeRawParamsCamera(torch.autograd.Function):
    """RasterizeRawParamsDepth with the camera as a differentiable input (render(pose_grad=True)): the
    same (color, radii, depth, alpha), and its backward also returns the gradients of `viewmatrix`,
    `projmatrix` and `campos` — three independent inputs, each in its memory layout
    (rr_backward_camera).  When none of the three requires a gradient the plain depth backward runs."""

    @staticmethod
    def forward(ctx, xyz, f_dc, f_rest, opacity, scaling, rotation, means2D, sh_degree, W, H, tanfovx, tanfovy,
                viewmatrix, projmatrix, campos, bg, low_pass, scale_modifier):
        return _raw_forward(ctx, (xyz, f_dc, f_rest, opacity, scaling, rotation, means2D, sh_degree, W, H, tanfovx,
                                  tanfovy, viewmatrix, projmatrix, campos, bg, low_pass, scale_modifier), camera=True)

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, grad_depth, grad_alpha):
        return _raw_backward(ctx, _RAW_INPUTS, grad_color, grad_depth, grad_alpha, camera=True)


class RasterizeRawParamsNormal(torch.autograd.Function):
    """RasterizeRawParamsDepth plus a differentiable aux normal map (render(normal_grad=True)):
    returns (color, radii, depth, alpha, normal) — normal = sum alpha_i T_i n_i [3,H,W] — and its
    backward adds the normal's gradient to the others' (rr_backward_aux_normal)."""

    @staticmethod
    def forward(ctx, xyz, f_dc, f_rest, opacity, scaling, rotation, means2D, sh_degree, W, H, tanfovx, tanfovy,
                viewmatrix, projmatrix, campos, bg, low_pass, scale_modifier):
        return _raw_forward(ctx, (xyz, f_dc, f_rest, opacity, scaling, rotation, means2D, sh_degree, W, H, tanfovx,
                                  tanfovy, viewmatrix, projmatrix, campos, bg, low_pass, scale_modifier), normal=True)

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, grad_depth, grad_alpha, grad_normal):
        return _raw_backward(ctx, _RAW_INPUTS, grad_color, grad_depth, grad_alpha, grad_normal)


class RasterizeRawParamsDist(torch.autograd.Function):
    """RasterizeRawParamsDepth plus the differentiable depth-moment maps of the distortion loss
    (render(dist_grad=True)), and with `normal` the aux normal map too: returns (color, radii, depth,
    alpha, normal or None, moments) — moments = (sum alpha_i T_i m_i, sum alpha_i T_i m_i^2) [2,H,W] —
    and its backward adds their gradients to the others' (rr_backward_aux_dist)."""

    @staticmethod
    def forward(ctx, xyz, f_dc, f_rest, opacity, scaling, rotation, means2D, sh_degree, W, H, tanfovx, tanfovy,
                viewmatrix, projmatrix, campos, bg, low_pass, scale_modifier, dist_near, dist_far, normal):
        return _raw_forward(ctx, (xyz, f_dc, f_rest, opacity, scaling, rotation, means2D, sh_degree, W, H, tanfovx,
                                  tanfovy, viewmatrix, projmatrix, campos, bg, low_pass, scale_modifier),
                            normal=bool(normal), dist=(dist_near, dist_far))

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, grad_depth, grad_alpha, grad_normal, grad_moments):
        return _raw_backward(ctx, _RAW_INPUTS + 3, grad_color, grad_depth, grad_alpha, grad_normal, grad_moments)
