"""The call protocols of the render ABI (include/rain_raster.h), written once for the three modules that
drive it through ctypes: the reference-API route (diff_gaussian_rasterization/_C.py), the raw-parameter
route (fused.py) and the Gaussian-sharded step (sharded.py).

What lives here and nowhere else: the device-pointer helper, the camera block, the field order and row
widths of a raw-mode rr_gaussians, the binning buffer's growth policy, the workspace registration protocol
(register before the render, drop the registration when the render fails, flag a copy of the frame for the
backward), the counted two-stage forward, the one-call forward with its RR_INCOMPLETE retry, and which
backward entry point a set of output gradients selects, with its argument tuple.

Every function that calls the library takes the loaded library `L` and the `stream`; none of them looks
either up, so a stand-in `L` and CPU tensors drive them without a GPU (tests/test_raster_driver_cpu.py).
Validation, refusals and output allocation stay with the callers.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native as N


def ptr(t, byte_offset=0):
    """Device pointer of a tensor (plus `byte_offset`), or None (NULL) for None and for an empty ("absent")
    tensor."""
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr() + byte_offset)


def camera_block(bg, viewmatrix, projmatrix, campos):
    """(keep, RRCamera): the four arrays made contiguous, to be kept alive beside the struct of their
    pointers.  None stays None (NULL)."""
    keep = (bg if bg is None else bg.contiguous(), viewmatrix if viewmatrix is None else viewmatrix.contiguous(),
            projmatrix if projmatrix is None else projmatrix.contiguous(),
            campos if campos is None else campos.contiguous())
    return keep, N.RRCamera(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]))


def raw_gaussians(xyz, f_dc, opacity, scaling, rotation, f_rest, row=0):
    """The rr_gaussians of an RR_FLAG_RAW_PARAMS frame over GaussianModel's raw parameters (contiguous
    float32, in the kernels' argument order), starting at Gaussian `row`: xyz, f_dc, no precomputed colour,
    opacity, scaling, rotation, no precomputed covariance, f_rest (absent when M == 1)."""
    M = 1 + f_rest.shape[1]
    return N.RRGaussians(ptr(xyz, 12 * row), ptr(f_dc, 12 * row), None, ptr(opacity, 4 * row), ptr(scaling, 12 * row),
                         ptr(rotation, 16 * row), None, ptr(f_rest, 12 * (M - 1) * row) if M > 1 else None)


class BinningCache:
    """A grow-only binning buffer reused frame after frame (the training loop renders one frame,
    runs its backward, then renders the next, all on one stream, so frame s+1's binning never
    overwrites a list frame s's backward still reads).  With it the forward is one native call
    (rr_forward): the device waits only for the pair-count read-back, not for a return to Python."""

    def __init__(self, headroom: float = 1.25):
        self.buf = None
        self.headroom = headroom

    def get(self, nbytes: int, dev) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != dev:
            self.buf = torch.empty((int(nbytes * self.headroom) + 4096,), dtype=torch.uint8, device=dev)
        return self.buf


def register_workspace(L, P: int, dev, ws=None):
    """The backward's accumulator workspace (`ws`, or a new buffer), registered for the coming render to
    zero-fill (rr_set_forward_workspace: the backward then skips its clear).  None for P <= 0."""
    if P <= 0:
        return None
    if ws is None:
        ws = torch.empty((L.rr_backward_workspace_bytes(P),), dtype=torch.uint8, device=dev)
    N.check(L.rr_set_forward_workspace(ptr(ws), ws.numel()), "register workspace")
    return ws


def check_render(L, rc: int, what: str):
    """N.check, dropping a workspace registration a failed call left pending (it must not outlive
    its buffer)."""
    if rc not in (0, N.RR_INCOMPLETE):
        L.rr_set_forward_workspace(None, 0)
    N.check(rc, what)


def backward_frame(frame, registered: bool, flags: int = 0):
    """The frame a backward passes: the forward's own, or, when this backward has flags of its own
    (RR_FLAG_WORKSPACE_REGISTERED for a workspace the forward's render zero-filled, and `flags`), a copy
    carrying them.  The forward's frame is never modified."""
    if registered:
        flags |= N.RR_FLAG_WORKSPACE_REGISTERED
    if not flags:
        return frame
    out = N.RRFrame.from_buffer_copy(frame)
    out.flags |= flags
    return out


def render_counted(L, frame, cam, gs, radii, geom, img, cache, color, depth, normal, moments, dist, stream, what):
    """The counted two-stage forward: rr_forward_geometry, a binning buffer of the size its pair count
    asks for (from `cache`, if given), then rr_forward_render_dist with `dist` = (near, far) or
    rr_forward_render_aux without; `normal` / `moments` are the optional aux outputs.
    Returns (binning, num_rendered)."""
    nr, npairs = ctypes.c_int(0), ctypes.c_int(0)
    check_render(L, L.rr_forward_geometry(ctypes.byref(frame), ctypes.byref(cam), ctypes.byref(gs), ptr(radii),
                                          ptr(geom), geom.numel(), ptr(img), img.numel(), ctypes.byref(nr),
                                          ctypes.byref(npairs), stream), what)
    nbin = L.rr_binning_bytes(npairs.value, frame.width, frame.height) if npairs.value > 0 else 0
    binning = cache.get(nbin, geom.device) if cache is not None and nbin > 0 else \
        torch.empty((nbin,), dtype=torch.uint8, device=geom.device)
    if dist is not None:
        rc = L.rr_forward_render_dist(ctypes.byref(frame), ctypes.byref(cam), ctypes.byref(gs), ptr(radii), ptr(geom),
                                      ptr(img), ptr(binning), binning.numel(), npairs.value, ptr(color), ptr(depth),
                                      ptr(normal), ptr(moments), dist[0], dist[1], stream)
    else:
        rc = L.rr_forward_render_aux(ctypes.byref(frame), ctypes.byref(cam), ctypes.byref(gs), ptr(radii), ptr(geom),
                                     ptr(img), ptr(binning), binning.numel(), npairs.value, ptr(color), ptr(depth),
                                     ptr(normal), stream)
    check_render(L, rc, what)
    return binning, nr.value


def render_one_call(L, frame, cam, gs, radii, geom, img, cache, color, depth, stream, what):
    """The one-call forward into the cache's buffer: rr_forward, or with `gs` None, for a geometry buffer
    that is filled already, rr_forward_from_geometry.  When the pairs outgrew the buffer (RR_INCOMPLETE)
    it is grown (without a cache: allocated to size) and stage 2 runs on its own (rr_forward_render /
    rr_forward_render_geometry).  Returns (binning, num_rendered, num_pairs)."""
    dev = geom.device
    binning = cache.buf if cache is not None and cache.buf is not None and cache.buf.device == dev \
        else torch.empty((0,), dtype=torch.uint8, device=dev)
    nr, npairs, need = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    if gs is not None:
        rc = L.rr_forward(ctypes.byref(frame), ctypes.byref(cam), ctypes.byref(gs), ptr(radii), ptr(geom),
                          geom.numel(), ptr(img), img.numel(), ptr(binning), binning.numel(), ctypes.byref(nr),
                          ctypes.byref(npairs), ctypes.byref(need), ptr(color), ptr(depth), stream)
    else:
        rc = L.rr_forward_from_geometry(ctypes.byref(frame), ctypes.byref(cam), ptr(radii), ptr(geom), geom.numel(),
                                        ptr(img), img.numel(), ptr(binning), binning.numel(), ctypes.byref(nr),
                                        ctypes.byref(npairs), ctypes.byref(need), ptr(color), ptr(depth), stream)
    if rc == N.RR_INCOMPLETE:
        binning = cache.get(need.value, dev) if cache is not None else \
            torch.empty((need.value,), dtype=torch.uint8, device=dev)
        if gs is not None:
            rc = L.rr_forward_render(ctypes.byref(frame), ctypes.byref(cam), ctypes.byref(gs), ptr(radii), ptr(geom),
                                     ptr(img), ptr(binning), binning.numel(), npairs.value, ptr(color), ptr(depth),
                                     stream)
        else:
            rc = L.rr_forward_render_geometry(ctypes.byref(frame), ctypes.byref(cam), ptr(radii), ptr(geom), ptr(img),
                                              ptr(binning), binning.numel(), npairs.value, ptr(color), ptr(depth),
                                              stream)
    check_render(L, rc, what)
    return binning, nr.value, npairs.value


def backward(L, frame, cam, gs, radii, geom, img, binning, num_rendered, dL_dpix, dL_ddepth, dL_dalpha, dL_dnormal,
             dL_dmoments, dist, ws, grads, cam_grads, stream, what):
    """The backward of a frame rendered into (radii, geom, img, binning, num_rendered), into `grads` (an
    RRGrads).  The output gradients are contiguous float32 tensors, None when absent: an absent map goes
    to the library as NULL, and the library picks the kernel variants from which maps are there.
    `dist`: the frame's (near, far), read only with dL_dmoments.  `ws`: rr_backward_workspace_bytes(P) bytes.
    `cam_grads` = (d_viewmatrix, d_projmatrix, d_campos) tensors, or None, selects rr_backward_camera
    (the callers refuse it together with dL_dnormal / dL_dmoments)."""
    head = (ctypes.byref(frame), ctypes.byref(cam), ctypes.byref(gs), ptr(radii), ptr(geom), ptr(img), ptr(binning),
            int(num_rendered), ptr(dL_dpix))
    tail = (ptr(ws), ws.numel(), ctypes.byref(grads))
    if cam_grads is not None:
        scratch = torch.empty((L.rr_camera_grad_scratch_bytes(frame.P),), dtype=torch.uint8, device=ws.device)
        cg = N.RRCameraGrads(ptr(cam_grads[0]), ptr(cam_grads[1]), ptr(cam_grads[2]), ptr(scratch), scratch.numel())
        rc = L.rr_backward_camera(*head, ptr(dL_ddepth), ptr(dL_dalpha), *tail, ctypes.byref(cg), stream)
    elif dL_ddepth is None and dL_dalpha is None and dL_dnormal is None and dL_dmoments is None:
        # a colour-only backward stays on rr_backward (the reference's call)
        rc = L.rr_backward(*head, *tail, stream)
    else:
        # every other case is rr_backward_aux_dist, which with NULL maps is exactly each smaller entry point
        near, far = dist if dL_dmoments is not None else (0.0, 0.0)
        rc = L.rr_backward_aux_dist(*head, ptr(dL_ddepth), ptr(dL_dalpha), ptr(dL_dnormal), ptr(dL_dmoments), near,
                                    far, *tail, stream)
    N.check(rc, what)
