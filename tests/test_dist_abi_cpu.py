"""CPU checks of the depth-moment / distortion-loss surface: the libraries export and list the new
entry points (rr_forward_render_dist, rr_backward_aux_dist, rl_dist_*), every argument error comes
back as a code + message before any device work (the pointers below are stand-ins, so a call that
got past validation would fault), the Python layers have the documented signatures and no CPU
fallback, and the sharded trainer refuses a non-zero lambda_dist."""
import ctypes
import inspect
import os

import pytest
import torch

from rain_amd import _native as N
from rain_amd import cameras, synthetic
from rain_amd import loss as loss_mod
from rain_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C
from rain_amd.gaussian_model import GaussianModel, OptimizationParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_ERR_ARG, RR_ERR_CAPACITY = 1, 3


def test_symbols_exported_declared_and_listed():
    so = ctypes.CDLL(N.RASTER_LIB)
    header = open(os.path.join(ROOT, "include", "rain_raster.h")).read()
    for name in ("rr_forward_render_dist", "rr_backward_aux_dist"):
        assert hasattr(so, name), f"librain_raster.so does not export {name}"
        assert name in N.RASTER_SYMBOLS and f"{name}(" in header
    L = N.raster()
    nrm, dst = L.rr_backward_aux_normal.argtypes, L.rr_backward_aux_dist.argtypes
    # rr_backward_aux_normal's arguments with (dL_dmoments, dist_near, dist_far) after dL_dnormal (index 11)
    assert len(dst) == len(nrm) + 3
    assert list(dst[:12]) == list(nrm[:12]) and list(dst[15:]) == list(nrm[12:])
    assert list(dst[12:15]) == [ctypes.c_void_p, ctypes.c_float, ctypes.c_float]
    aux, fwd = L.rr_forward_render_aux.argtypes, L.rr_forward_render_dist.argtypes
    assert list(fwd[:12]) == list(aux[:12]) and list(fwd[12:]) == [ctypes.c_void_p, ctypes.c_float, ctypes.c_float,
                                                                  ctypes.c_void_p]
    lso = ctypes.CDLL(N.LOSS_LIB)
    lheader = open(os.path.join(ROOT, "include", "rain_loss.h")).read()
    for name in ("rl_dist_workspace_bytes", "rl_dist_forward", "rl_dist_backward", "rl_dist_forward_backward"):
        assert hasattr(lso, name), f"librain_loss.so does not export {name}"
        assert name in N.LOSS_SYMBOLS and f"{name}(" in lheader


def test_python_surface_exists():
    p = list(inspect.signature(_C.rasterize_gaussians_backward_dist).parameters)
    assert p[:25] == list(inspect.signature(_C.rasterize_gaussians_backward_normal).parameters)
    assert p[25:] == ["dL_dout_moments", "dist_near", "dist_far"]
    p = list(inspect.signature(_C.rasterize_gaussians_dist).parameters)
    assert p[:20] == list(inspect.signature(_C.rasterize_gaussians).parameters)
    assert p[20:] == ["dist_near", "dist_far", "normal"]
    sig = inspect.signature(GaussianRasterizer.forward_distortion).parameters
    assert list(sig)[:9] == list(inspect.signature(GaussianRasterizer.forward).parameters)
    assert sig["dist_near"].default == 0.2 and sig["dist_far"].default == 100.0 and sig["normal"].default is False
    from rain_amd import fused, renderer

    assert inspect.signature(fused.forward).parameters["dist"].default is None
    assert inspect.signature(fused.backward).parameters["dL_dmoments"].default is None
    assert hasattr(fused, "RasterizeRawParamsDist")
    r = inspect.signature(renderer.render).parameters
    assert r["dist_grad"].default is False and r["dist_near"].default == 0.2 and r["dist_far"].default == 100.0
    opt = OptimizationParams()
    assert (opt.lambda_dist, opt.lambda_dist_from_iter, opt.dist_near, opt.dist_far) == (0.0, 3000, 0.2, 100.0)
    assert list(inspect.signature(loss_mod.fused_distortion_loss).parameters) == ["alpha", "moments", "lambda_dist"]
    p = inspect.signature(loss_mod.distortion_loss_forward_backward).parameters
    assert list(p)[:4] == ["alpha", "moments", "lambda_dist", "d_alpha"] and p["d_alpha"].default is None


def _settings():
    return GaussianRasterizationSettings(
        image_height=48, image_width=64, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0,
        viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False,
        debug=False, low_pass=0.3)


def test_forward_distortion_argument_messages_and_no_cpu_fallback():
    r = GaussianRasterizer(_settings())
    m = torch.zeros(5, 3)
    kw = dict(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3))
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r.forward_distortion(means3D=m, means2D=m, opacities=torch.zeros(5, 1), scales=m, rotations=torch.zeros(5, 4))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
        r.forward_distortion(**kw)
    with pytest.raises(Exception, match="render_depth_normal needs the scale/rotation pair"):
        r.forward_distortion(**kw, cov3D_precomp=torch.zeros(5, 6), normal=True)
    for near, far in ((0.0, 1.0), (0.2, 0.2), (0.3, 0.2), (-0.1, 1.0), (0.2, float("inf")), (float("nan"), 1.0),
                      (0.2, 0.0)):
        with pytest.raises(Exception, match="0 < dist_near < dist_far"):
            r.forward_distortion(**kw, scales=m, rotations=torch.zeros(5, 4), dist_near=near, dist_far=far)
    for near, far in ((0.2, 100.0), (0.0, 0.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            r.forward_distortion(**kw, scales=m, rotations=torch.zeros(5, 4), dist_near=near, dist_far=far)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.forward_distortion(**kw, cov3D_precomp=torch.zeros(5, 6))  # moments alone accept a covariance


def test_distortion_loss_refuses_cpu_tensors():
    A, M = torch.ones(1, 4, 5), torch.ones(2, 4, 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        loss_mod.fused_distortion_loss(A, M, 0.1)
    for fn in (loss_mod.distortion_loss_forward, loss_mod.distortion_loss_backward,
               loss_mod.distortion_loss_forward_backward):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(A, M, 0.1)


BAD_RANGES = ((0.0, 1.0), (0.2, 0.0), (0.2, 0.2), (0.3, 0.2), (-0.2, 1.0), (-1.0, -0.5), (0.2, float("inf")),
              (float("nan"), 1.0), (0.2, float("nan")))


def test_rr_backward_aux_dist_validation_without_gpu():
    """Every refusal below happens before the library touches a device.  Argument errors are RR_ERR_ARG;
    an undersized workspace is RR_ERR_CAPACITY, the code every entry point of the header uses for a
    buffer that is too small."""
    L = N.raster()
    flagged = N.RR_FLAG_AUX_NORMAL
    f = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, flagged)
    f_plain = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0)
    cam = N.RRCamera(1, 1, 1, 1)
    g = N.RRGaussians(1, 1, None, None, 1, 1, None)
    g_cov = N.RRGaussians(1, 1, None, None, None, None, 1)
    out = N.RRGrads()
    full = N.RRGrads(*([1] * 8))
    args = dict(radii=1, geom=1, img=1, binning=1, R=5, dpix=1, dd=1, da=1, dn=1, dm=1, near=0.2, far=100.0, ws=1,
                ws_bytes=1 << 20)

    def call(frame, grads, gs=g, **kw):
        a = dict(args, **kw)
        return L.rr_backward_aux_dist(ctypes.byref(frame) if frame is not None else None, ctypes.byref(cam),
                                      ctypes.byref(gs), a["radii"], a["geom"], a["img"], a["binning"], a["R"],
                                      a["dpix"], a["dd"], a["da"], a["dn"], a["dm"], a["near"], a["far"], a["ws"],
                                      a["ws_bytes"], ctypes.byref(grads) if grads is not None else None, None)

    def err():
        return L.rr_last_error()

    assert call(None, out) == RR_ERR_ARG and b"null frame" in err()
    assert call(f, None) == RR_ERR_ARG and b"null buffer" in err()
    # all five output gradients absent: nothing to differentiate
    assert call(f, out, dpix=None, dd=None, da=None, dn=None, dm=None) == RR_ERR_ARG and b"null buffer" in err()
    # near / far: refused whatever else is given (complete gradient outputs, either frame)
    for near, far in BAD_RANGES:
        for frame, grads, dn in ((f, full, 1), (f_plain, full, None), (f, out, 1)):
            assert call(frame, grads, dn=dn, near=near, far=far) == RR_ERR_ARG, (near, far)
            assert b"dist_near / dist_far" in err(), (near, far, err())
    # ... but not looked at without a moment gradient: the call then is rr_backward_aux_normal
    assert call(f, out, dm=None, near=0.3, far=0.2) == RR_ERR_ARG and b"null gradient output" in err()
    # both valid mappings pass that check and stop at the missing outputs
    for near, far in ((0.2, 100.0), (0.0, 0.0), (1e-3, 1e-2)):
        assert call(f, out, near=near, far=far) == RR_ERR_ARG and b"null gradient output" in err()
    # a normal gradient without the flag, with or without moments
    assert call(f_plain, out) == RR_ERR_ARG and b"RR_FLAG_AUX_NORMAL" in err()
    assert call(f_plain, out, dpix=None, dd=None, da=None) == RR_ERR_ARG and b"RR_FLAG_AUX_NORMAL" in err()
    # moments without a normal gradient need no flag: as far as the missing outputs
    assert call(f_plain, out, dn=None) == RR_ERR_ARG and b"null gradient output" in err()
    assert call(f_plain, out, dn=None, dpix=None, dd=None, da=None) == RR_ERR_ARG and b"null gradient output" in err()
    # moments with cov3D_precomp: refused with a normal gradient, accepted alone
    assert call(f, full, gs=g_cov) == RR_ERR_ARG and b"scales/rotations" in err()
    assert call(f_plain, full, gs=g_cov) == RR_ERR_ARG
    assert call(f_plain, out, gs=g_cov, dn=None) == RR_ERR_ARG and b"null gradient output" in err()
    # undersized / missing buffers
    assert call(f, full, ws=None) == RR_ERR_ARG and b"null buffer" in err()
    assert call(f, full, geom=None) == RR_ERR_ARG and b"null buffer" in err()
    assert call(f, full, ws_bytes=L.rr_backward_workspace_bytes(10) - 1) == RR_ERR_CAPACITY
    assert b"workspace too small" in err()
    assert call(f_plain, full, dn=None, ws_bytes=0) == RR_ERR_CAPACITY and b"workspace too small" in err()
    # the fused step needs raw-parameter mode, as in rr_backward
    ad = N.RRAdam()
    out_ad = N.RRGrads()
    out_ad.adam = ctypes.pointer(ad)
    assert call(f, out_ad) == RR_ERR_ARG and b"raw-parameter mode" in err()
    # a next frame that carries the normal flag is refused (the current one may carry it)
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
    assert call(f_raw, out_nx, gs=g_raw) == RR_ERR_ARG and b"no aux normals" in err(), err()
    # P == 0 is a no-op success
    f0 = N.RRFrame(0, 0, 0, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, flagged)
    assert call(f0, out) == 0


def test_rr_forward_render_dist_validation_without_gpu():
    L = N.raster()
    flagged = N.RR_FLAG_AUX_NORMAL
    f = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, flagged)
    f_plain = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0)
    cam = N.RRCamera(1, 1, 1, 1)
    g = N.RRGaussians(1, 1, None, 1, 1, 1, None)
    g_cov = N.RRGaussians(1, 1, None, 1, None, None, 1)

    def call(frame, gs=g, nmap=1, mom=1, near=0.2, far=100.0, color=1, binning=1, bytes_=1 << 20, pairs=100):
        return L.rr_forward_render_dist(ctypes.byref(frame) if frame is not None else None, ctypes.byref(cam),
                                        ctypes.byref(gs), 1, 1, 1, binning, bytes_, pairs, color, 1, nmap, mom, near,
                                        far, None)

    def err():
        return L.rr_last_error()

    assert call(None) == RR_ERR_ARG and b"null frame" in err()
    # out_normal exactly with the flag, as in rr_forward_render_aux
    assert call(f, nmap=None) == RR_ERR_ARG and b"out_normal" in err()
    assert call(f_plain) == RR_ERR_ARG and b"out_normal" in err()
    assert call(f, gs=g_cov) == RR_ERR_ARG and b"scales/rotations" in err()
    assert call(f_plain, nmap=None, mom=None) == RR_ERR_ARG and b"out_moments" in err()
    for near, far in BAD_RANGES:
        for frame, nmap, gs in ((f, 1, g), (f_plain, None, g), (f_plain, None, g_cov)):
            assert call(frame, gs=gs, nmap=nmap, near=near, far=far) == RR_ERR_ARG, (near, far)
            assert b"dist_near / dist_far" in err()
    # a valid call gets as far as the buffers: null output, then a render without a pair count (the
    # hand-off check, still on the host)
    for near, far in ((0.2, 100.0), (0.0, 0.0)):
        assert call(f, near=near, far=far, color=None) == RR_ERR_ARG and b"null buffer" in err()
        assert call(f_plain, nmap=None, gs=g_cov, near=near, far=far, binning=None) == RR_ERR_ARG
        assert b"null buffer" in err()
        assert call(f, near=near, far=far) == RR_ERR_ARG and b"render without a pair count" in err()
    f0 = N.RRFrame(0, 0, 0, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0)
    assert call(f0, nmap=None) == 0


def test_rl_dist_validation_without_gpu():
    L = N.loss_lib()
    H, W = 6, 8
    assert L.rl_dist_workspace_bytes(0, 5) == 0 and L.rl_dist_workspace_bytes(5, -1) == 0
    assert 8 <= L.rl_dist_workspace_bytes(3, 3) <= 4096
    assert L.rl_dist_workspace_bytes(1080, 1920) >= (1080 * 1920 + 255) // 256 * 8
    assert L.rl_dist_workspace_bytes(1080, 1920) < 1080 * 1920  # block partials only: no per-pixel planes
    base = dict(A=1, M=1, H=H, W=W, lam=0.1, ws=1, wsb=1 << 20, loss=1, parts=1, gl=1, dA=1, dM=1, acc=0)

    def fwd(**kw):
        a = dict(base, **kw)
        return L.rl_dist_forward(a["A"], a["M"], a["H"], a["W"], a["lam"], a["ws"], a["wsb"], a["loss"], a["parts"],
                                 None)

    def bwd(**kw):
        a = dict(base, **kw)
        return L.rl_dist_backward(a["A"], a["M"], a["H"], a["W"], a["lam"], a["gl"], a["dA"], a["dM"], a["acc"], None)

    def both(**kw):
        a = dict(base, **kw)
        return L.rl_dist_forward_backward(a["A"], a["M"], a["H"], a["W"], a["lam"], a["ws"], a["wsb"], a["loss"],
                                          a["parts"], a["gl"], a["dA"], a["dM"], a["acc"], None)

    def err():
        return L.rl_last_error()

    for call, who in ((fwd, b"rl_dist_forward:"), (bwd, b"rl_dist_backward:"), (both, b"rl_dist_forward_backward:")):
        for kw in (dict(A=None), dict(M=None)):
            assert call(**kw) == 1 and err().startswith(who) and b"null" in err(), (who, kw, err())
        for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(W=-1)):
            assert call(**kw) == 1 and err().startswith(who) and b"positive" in err(), (who, kw, err())
        assert call(H=1 << 14, W=1 << 14) == 1 and b"2^28" in err()
    for call in (fwd, both):
        assert call(ws=None) == 1 and b"null" in err()
        assert call(loss=None) == 1 and b"null" in err()
        assert call(wsb=L.rl_dist_workspace_bytes(H, W) - 1) == 3 and b"workspace too small" in err()
        assert call(wsb=0) == 3
    for call in (bwd, both):
        for acc in (0, 1):
            for kw in (dict(gl=None), dict(dA=None), dict(dM=None)):
                assert call(acc=acc, **kw) == 1 and b"null" in err(), kw


def test_render_dist_grad_refuses_python_covariance_with_normals():
    from rain_amd.renderer import PipelineParams, render

    with pytest.raises(Exception, match="normal_grad=True"):
        render(None, None, PipelineParams(compute_cov3D_python=True), torch.zeros(3), normal_grad=True, dist_grad=True)


def _ref_loss(img, gt, lam):
    return (img - gt).abs().mean()


def test_sharded_trainer_refuses_lambda_dist():
    """The sharded / multi-rank steps have no depth-moment backward: a non-zero lambda_dist is a
    ValueError (at construction when the trainer is sharded from the start, else at the step)."""
    from rain_amd.renderer import PipelineParams
    from rain_amd.train import TrainConfig, Trainer, resolve_options

    def trainer(**kw):
        g = GaussianModel(1, divide_ratio=0.8, device="cpu")
        g.set_params(synthetic.random_gaussians(50, sh_degree=1, seed=0, bench=True))
        g.spatial_lr_scale = 4.4
        opt = OptimizationParams(**kw)
        g.training_setup(opt)
        cams = cameras.fibonacci_cameras(4, 32, 24)
        gts = [torch.zeros(3, 24, 32) for _ in cams]
        return Trainer(g, cams, gts, opt, PipelineParams(), TrainConfig(c2f=False), scene_extent=4.4, loss_fn=_ref_loss)

    t = trainer(lambda_dist=0.1, lambda_dist_from_iter=1)
    assert not t.sharded and not t.fused
    t.sharded = True  # what world > 1 (or a forced exchange) sets; no ranks are started
    with pytest.raises(ValueError, match="lambda_dist > 0 needs the single-GPU step"):
        t.step(1)
    with pytest.raises(ValueError, match="lambda_dist > 0 needs the single-GPU step"):
        t.step(5000)
    with pytest.raises(ValueError, match="lambda_dist > 0 needs the single-GPU step"):
        resolve_options(t.opt, t.pipe, t.sharded)  # whatever lambda_dist_from_iter: the configuration is refused
    t0 = trainer()  # the default weight passes
    t0.sharded = True
    o0 = resolve_options(t0.opt, t0.pipe, t0.sharded)
    assert o0.dist_weight(1) == 0.0 and o0.dist_weight(10_000) == 0.0
    t1 = trainer(lambda_dist=0.1)
    assert t1.options.dist_weight(2999) == 0.0 and t1.options.dist_weight(3000) == pytest.approx(0.1)
