"""CPU checks of the differentiable normal map's surface: the C ABI exports and lists
rr_backward_aux_normal, it validates before any device work, and the Python layers
(_C.rasterize_gaussians_backward_normal, GaussianRasterizer.forward_normal, fused.backward,
render) have the documented signatures, argument messages and no CPU fallback."""
import ctypes
import inspect

import pytest
import torch

from rain_amd import _native as N
from rain_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C


def test_symbol_exported_and_listed():
    so = ctypes.CDLL(N.RASTER_LIB)
    assert hasattr(so, "rr_backward_aux_normal"), "librain_raster.so does not export rr_backward_aux_normal"
    assert "rr_backward_aux_normal" in N.RASTER_SYMBOLS
    L = N.raster()
    aux, nrm = L.rr_backward_aux.argtypes, L.rr_backward_aux_normal.argtypes
    assert len(nrm) == len(aux) + 1
    # rr_backward_aux's arguments with one more pointer after dL_dalpha (index 10)
    assert list(nrm[:11]) == list(aux[:11]) and nrm[11] is ctypes.c_void_p and list(nrm[12:]) == list(aux[11:])


def test_python_surface_exists():
    p = list(inspect.signature(_C.rasterize_gaussians_backward_normal).parameters)
    assert p[:22] == list(inspect.signature(_C.rasterize_gaussians_backward).parameters)
    assert p[22:] == ["dL_dout_depth", "dL_dout_alpha", "dL_dout_normal"]
    assert list(inspect.signature(GaussianRasterizer.forward_normal).parameters) == \
        list(inspect.signature(GaussianRasterizer.forward).parameters)
    from rain_amd import fused, renderer

    assert inspect.signature(fused.backward).parameters["dL_dnormal"].default is None
    assert inspect.signature(fused.forward).parameters["normal"].default is False
    assert inspect.signature(renderer.render).parameters["normal_grad"].default is False
    assert hasattr(fused, "RasterizeRawParamsNormal")


def _settings():
    return GaussianRasterizationSettings(
        image_height=48, image_width=64, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0,
        viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False,
        debug=False, low_pass=0.3)


def test_forward_normal_argument_messages():
    r = GaussianRasterizer(_settings())
    m = torch.zeros(5, 3)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r.forward_normal(means3D=m, means2D=m, opacities=torch.zeros(5, 1), scales=m, rotations=torch.zeros(5, 4))
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r.forward_normal(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3),
                         colors_precomp=m, scales=m, rotations=torch.zeros(5, 4))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        r.forward_normal(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
        r.forward_normal(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3), scales=m,
                         rotations=torch.zeros(5, 4), cov3D_precomp=torch.zeros(5, 6))
    # render_depth_normal's message for a precomputed covariance
    with pytest.raises(Exception, match="render_depth_normal needs the scale/rotation pair"):
        r.forward_normal(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3),
                         cov3D_precomp=torch.zeros(5, 6))
    with pytest.raises(Exception, match="render_depth_normal needs the scale/rotation pair"):
        r.render_depth_normal(m, torch.zeros(5, 1), shs=torch.zeros(5, 1, 3))


def test_forward_normal_has_no_cpu_fallback():
    r = GaussianRasterizer(_settings())
    m = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.forward_normal(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3), scales=m,
                         rotations=torch.zeros(5, 4))


def test_render_normal_grad_refuses_python_covariance():
    from rain_amd.renderer import PipelineParams, render

    with pytest.raises(Exception, match="normal_grad=True"):
        render(None, None, PipelineParams(compute_cov3D_python=True), torch.zeros(3), normal_grad=True)


def test_rr_backward_aux_normal_validation_without_gpu():
    """Every refusal below happens before the library touches a device (the pointers are stand-ins)."""
    L = N.raster()
    flagged = N.RR_FLAG_AUX_NORMAL
    f = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, flagged)
    f_plain = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0)
    cam = N.RRCamera(1, 1, 1, 1)
    g = N.RRGaussians(1, 1, None, None, 1, 1, None)
    g_cov = N.RRGaussians(1, 1, None, None, None, None, 1)
    out = N.RRGrads()
    args = dict(radii=1, geom=1, img=1, binning=1, R=5, dpix=1, dd=1, da=1, dn=1, ws=1, ws_bytes=1 << 20)

    def call(frame, grads, gs=g, **kw):
        a = dict(args, **kw)
        return L.rr_backward_aux_normal(ctypes.byref(frame) if frame is not None else None, ctypes.byref(cam),
                                        ctypes.byref(gs), a["radii"], a["geom"], a["img"], a["binning"], a["R"],
                                        a["dpix"], a["dd"], a["da"], a["dn"], a["ws"], a["ws_bytes"],
                                        ctypes.byref(grads) if grads is not None else None, None)

    assert call(None, out) == 1 and b"null frame" in L.rr_last_error()
    assert call(f, None) == 1 and b"null buffer" in L.rr_last_error()
    # all four output gradients absent: nothing to differentiate
    assert call(f, out, dpix=None, dd=None, da=None, dn=None) == 1 and b"null buffer" in L.rr_last_error()
    # a normal gradient for a frame rendered without the flag
    assert call(f_plain, out) == 1 and b"RR_FLAG_AUX_NORMAL" in L.rr_last_error()
    assert call(f_plain, out, dpix=None, dd=None, da=None) == 1 and b"RR_FLAG_AUX_NORMAL" in L.rr_last_error()
    # ... and without it the same frame gets as far as rr_backward_aux does
    assert call(f_plain, out, dn=None) == 1 and b"null gradient output" in L.rr_last_error()
    # a normal gradient without the scale / rotation pair (flagged or not, it is refused)
    assert call(f, out, gs=g_cov) == 1 and b"scales/rotations" in L.rr_last_error()
    assert call(f_plain, out, gs=g_cov) == 1
    # the normal gradient alone passes these checks and stops at the missing outputs
    assert call(f, out, dpix=None, dd=None, da=None) == 1 and b"null gradient output" in L.rr_last_error()
    assert call(f, out, ws=None) == 1 and b"null buffer" in L.rr_last_error()
    # the fused step needs raw-parameter mode, as in rr_backward
    ad = N.RRAdam()
    out_ad = N.RRGrads()
    out_ad.adam = ctypes.pointer(ad)
    assert call(f, out_ad) == 1 and b"raw-parameter mode" in L.rr_last_error()
    # a next frame that carries the flag is refused (the current one may carry it)
    P, M = 10, 1
    raw = N.RR_FLAG_RAW_PARAMS
    f_raw = N.RRFrame(P, 0, M, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, raw | flagged)
    g_raw = N.RRGaussians(1, 1, None, 1, 1, 1, None, None)
    ad = N.RRAdam()
    for name in ("xyz", "f_dc", "opacity", "scaling", "rotation"):
        grp = getattr(ad, name)
        grp.param, grp.exp_avg, grp.exp_avg_sq = 1, 1, 1
    nf = N.RRFrame(P, 0, M, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, raw | flagged)
    nx = N.RRNextFrame(ctypes.pointer(nf), ctypes.pointer(cam), 1, 2, 1 << 30)
    out_nx = N.RRGrads()
    out_nx.adam = ctypes.pointer(ad)
    out_nx.next = ctypes.pointer(nx)
    rc = call(f_raw, out_nx, gs=g_raw)
    assert rc == 1 and b"no aux normals" in L.rr_last_error(), L.rr_last_error()
    # P == 0 is a no-op success
    f0 = N.RRFrame(0, 0, 0, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, flagged)
    assert call(f0, out) == 0
