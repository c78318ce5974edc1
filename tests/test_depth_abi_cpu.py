"""CPU checks of the depth / accumulated-alpha surface: the C ABI exports and lists rr_backward_aux
and rr_render_alpha, rr_backward_aux validates like rr_backward, and GaussianRasterizer.forward_depth
keeps forward()'s argument checks and refuses CPU tensors (no CPU fallback)."""
import ctypes
import inspect

import pytest
import torch

from rain_amd import _native as N
from rain_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C


def test_new_symbols_exported_and_listed():
    so = ctypes.CDLL(N.RASTER_LIB)
    for name in ("rr_backward_aux", "rr_render_alpha"):
        assert hasattr(so, name), f"librain_raster.so does not export {name}"
        assert name in N.RASTER_SYMBOLS
    L = N.raster()
    assert len(L.rr_backward_aux.argtypes) == len(L.rr_backward.argtypes) + 2
    assert len(L.rr_render_alpha.argtypes) == 4


def test_python_surface_exists():
    p = list(inspect.signature(_C.rasterize_gaussians_backward_depth).parameters)
    assert p[:22] == list(inspect.signature(_C.rasterize_gaussians_backward).parameters)
    assert p[22:] == ["dL_dout_depth", "dL_dout_alpha"]
    assert list(inspect.signature(_C.accumulated_alpha).parameters) == ["imageBuffer", "H", "W"]
    assert list(inspect.signature(GaussianRasterizer.forward_depth).parameters) == \
        list(inspect.signature(GaussianRasterizer.forward).parameters)
    from rain_amd import fused, renderer

    sig = inspect.signature(fused.backward).parameters
    assert sig["dL_ddepth"].default is None and sig["dL_dalpha"].default is None
    assert inspect.signature(renderer.render).parameters["depth_grad"].default is False
    assert hasattr(fused, "RasterizeRawParamsDepth")


def _settings():
    return GaussianRasterizationSettings(
        image_height=48, image_width=64, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0,
        viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False,
        debug=False, low_pass=0.3)


def test_forward_depth_argument_messages():
    r = GaussianRasterizer(_settings())
    m = torch.zeros(5, 3)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r.forward_depth(means3D=m, means2D=m, opacities=torch.zeros(5, 1), scales=m, rotations=torch.zeros(5, 4))
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r.forward_depth(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3),
                        colors_precomp=m, scales=m, rotations=torch.zeros(5, 4))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        r.forward_depth(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
        r.forward_depth(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3), scales=m,
                        rotations=torch.zeros(5, 4), cov3D_precomp=torch.zeros(5, 6))


def test_forward_depth_has_no_cpu_fallback():
    r = GaussianRasterizer(_settings())
    m = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.forward_depth(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3), scales=m,
                        rotations=torch.zeros(5, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C.accumulated_alpha(torch.zeros(16, dtype=torch.uint8), 4, 4)


def test_rr_backward_aux_validation_without_gpu():
    """Every refusal below happens before the library touches a device (the pointers are stand-ins)."""
    L = N.raster()
    f = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0)
    cam = N.RRCamera(1, 1, 1, 1)
    g = N.RRGaussians(1, 1, None, None, 1, 1, None)
    out = N.RRGrads()
    args = dict(radii=1, geom=1, img=1, binning=1, R=5, dpix=1, dd=1, da=1, ws=1, ws_bytes=1 << 20)

    def call(frame, grads, **kw):
        a = dict(args, **kw)
        return L.rr_backward_aux(ctypes.byref(frame) if frame is not None else None, ctypes.byref(cam),
                                 ctypes.byref(g), a["radii"], a["geom"], a["img"], a["binning"], a["R"], a["dpix"],
                                 a["dd"], a["da"], a["ws"], a["ws_bytes"],
                                 ctypes.byref(grads) if grads is not None else None, None)

    assert call(None, out) == 1 and b"null frame" in L.rr_last_error()
    assert call(f, None) == 1 and b"null buffer" in L.rr_last_error()
    # all three output gradients absent: nothing to differentiate
    assert call(f, out, dpix=None, dd=None, da=None) == 1 and b"null buffer" in L.rr_last_error()
    # a gradient block without outputs, with and without the colour gradient
    assert call(f, out) == 1 and b"null gradient output" in L.rr_last_error()
    assert call(f, out, dpix=None) == 1 and b"null gradient output" in L.rr_last_error()
    assert call(f, out, ws=None) == 1 and b"null buffer" in L.rr_last_error()
    # the fused step needs raw-parameter mode, as in rr_backward
    ad = N.RRAdam()
    out_ad = N.RRGrads()
    out_ad.adam = ctypes.pointer(ad)
    assert call(f, out_ad) == 1 and b"raw-parameter mode" in L.rr_last_error()
    # P == 0 is a no-op success
    f0 = N.RRFrame(0, 0, 0, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0)
    assert call(f0, out) == 0
    # rr_render_alpha
    assert L.rr_render_alpha(None, 1, 1, None) == 1 and b"null frame" in L.rr_last_error()
    assert L.rr_render_alpha(ctypes.byref(f), 1, None, None) == 1 and b"null output" in L.rr_last_error()
    assert L.rr_render_alpha(ctypes.byref(f), None, 1, None) == 1 and b"null image buffer" in L.rr_last_error()
