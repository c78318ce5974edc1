"""CPU checks of the absolute-gradient surface (include/rain_raster.h RR_FLAG_ABSGRAD): the flag's value, the
new output's place in rr_grads, how the switch reaches every layer without touching the pinned signatures,
the backward plan, and every refusal, each of which comes back before the library or the Python layer touches
a device."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

from rain_amd import _build as B
from rain_amd import _native as N
from rain_amd import cameras, fused
from rain_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C
from rain_amd.gaussian_model import GaussianModel, OptimizationParams
from rain_amd.renderer import PipelineParams, render

HERE = os.path.dirname(os.path.abspath(__file__))


def test_flag_value_and_header():
    assert N.RR_FLAG_ABSGRAD == 64
    flags = [N.RR_FLAG_NO_TILE_CULLING, N.RR_FLAG_RAW_PARAMS, N.RR_FLAG_FULL_BINNING, N.RR_FLAG_AUX_NORMAL,
             N.RR_FLAG_WORKSPACE_REGISTERED, N.RR_FLAG_ANTIALIAS, N.RR_FLAG_ABSGRAD]
    assert sorted(flags) == [1, 2, 4, 8, 16, 32, 64]
    header = open(os.path.join(os.path.dirname(HERE), "include", "rain_raster.h")).read()
    assert re.search(r"#define\s+RR_FLAG_ABSGRAD\s+64\b", header)
    comment = header.split("#define RR_FLAG_ABSGRAD")[0].rsplit("#define RR_FLAG_ANTIALIAS", 1)[1]
    for name in ("rr_backward_camera", "rr_backward_records", "rr_gauss_backward_views", "dL_dmeans2D_abs",
                 "follow-ups"):
        assert name in comment, name
    # the new output is the last field of rr_grads, in the header and in its ctypes mirror
    body = re.search(r"typedef struct rr_grads \{(.*?)\} rr_grads;", header, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?(?:struct\s+)?\w+\s*\*\s*(\w+);", body, re.M)
    assert fields[-2:] == ["next", "dL_dmeans2D_abs"]
    names = [n for n, _ in N.RRGrads._fields_]
    assert names[-1] == "dL_dmeans2D_abs" and names[-3:-1] == ["adam", "next"] and len(names) == 15
    assert N.RRGrads(*([None] * 14)).dL_dmeans2D_abs is None  # positional construction with 14 values stands


def test_switch_sets_the_frame_flag_and_nests():
    def flag():
        return _C._frame(1, 0, 1, 8, 8, 1.0, 1.0, 1.0, 0.3, False, False).flags & N.RR_FLAG_ABSGRAD

    assert not _C.absgrad_on() and flag() == 0
    with _C.absgrad():
        assert _C.absgrad_on() and flag() == 64
        with _C.absgrad(False):
            assert flag() == 0
            with _C.antialiased():  # the two switches are independent
                assert flag() == 0 and _C.antialiasing_on()
        assert flag() == 64 and not _C.antialiasing_on()
    assert not _C.absgrad_on() and flag() == 0
    with pytest.raises(KeyError):  # restored on the way out of a failing block too
        with _C.absgrad():
            raise KeyError
    assert flag() == 0


def test_python_surface():
    sig = inspect.signature(GaussianRasterizer.__init__).parameters
    assert list(sig) == ["self", "raster_settings", "antialiasing"]
    assert GaussianRasterizer.absgrad is False
    a = list(inspect.signature(_C.rasterize_gaussians_backward).parameters)
    b = list(inspect.signature(_C.rasterize_gaussians_backward_abs).parameters)
    assert len(a) == 22 and a == b
    p = inspect.signature(fused.backward).parameters
    assert p["absgrad"].default is False and p["dmeans2D_abs"].default is None
    assert inspect.signature(render).parameters["absgrad"].default is False
    assert inspect.signature(GaussianModel.add_densification_stats).parameters["absgrad"].default is False
    assert OptimizationParams().densify_absgrad is False
    assert OptimizationParams().densify_grad_threshold == 0.0002  # the default threshold is not changed
    assert OptimizationParams(densify_absgrad=True).densify_absgrad is True


def _settings():
    return GaussianRasterizationSettings(
        image_height=48, image_width=64, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0,
        viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False,
        debug=False, low_pass=0.3)


def test_python_refusals_without_gpu(monkeypatch):
    r = GaussianRasterizer(_settings())
    assert r.absgrad is False
    r.absgrad = True
    assert GaussianRasterizer.absgrad is False  # set on the instance
    m = torch.zeros(5, 3)
    kw = dict(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3), scales=m,
              rotations=torch.zeros(5, 4))
    # raised before _C is reached: a _C whose every entry point fails would be noticed
    import rain_amd.diff_gaussian_rasterization as dgr

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"_C.{name} reached")

    with monkeypatch.context() as mp:
        mp.setattr(dgr, "_C", Untouchable())
        for name in ("forward_depth", "forward_normal", "forward_distortion", "forward_camera"):
            with pytest.raises(ValueError, match=f"{name} does not combine with absgrad"):
                getattr(r, name)(**kw)
        with pytest.raises(ValueError, match="render_depth_normal does not combine with absgrad"):
            r.render_depth_normal(m, torch.zeros(5, 1), shs=torch.zeros(5, 1, 3), scales=m,
                                  rotations=torch.zeros(5, 4))
    # forward() honours it: it reaches the device check (no CPU fallback) with the switch on, and restores it
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r(**kw)
    assert not _C.absgrad_on()
    cam = cameras.fibonacci_cameras(8, 64, 48)[0]
    for extra in ("depth_grad", "normal_grad", "dist_grad", "pose_grad"):
        with pytest.raises(ValueError, match="absgrad=True.*does not combine"):
            render(cam, None, PipelineParams(), torch.zeros(3), absgrad=True, **{extra: True})
    st = fused.RawFrame(N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, N.RR_FLAG_RAW_PARAMS), None, None,
                        (), None, None, None, None, 0, 10, 1)
    dpix, amap = torch.zeros(3, 48, 64), torch.zeros(1, 48, 64)
    with monkeypatch.context() as mp:
        mp.setattr(N, "raster", lambda: (_ for _ in ()).throw(AssertionError("the library was reached")))
        for k in ("dL_ddepth", "dL_dalpha"):
            with pytest.raises(RuntimeError, match="absgrad does not combine with depth / alpha / normal / moments"):
                fused.backward(st, dpix, {}, absgrad=True, **{k: amap})
        with pytest.raises(RuntimeError, match="absgrad does not combine with depth / alpha / normal / moments"):
            fused.backward(st, dpix, {}, absgrad=True, dL_dnormal=dpix)
        with pytest.raises(RuntimeError, match="absgrad does not combine with depth / alpha / normal / moments"):
            fused.backward(st, dpix, {}, absgrad=True, dL_dmoments=torch.zeros(2, 48, 64))
        cg = (torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(3))
        with pytest.raises(RuntimeError, match="absgrad does not combine with camera gradients"):
            fused.backward(st, dpix, {}, absgrad=True, cam_grads=cg)
        with pytest.raises(RuntimeError, match="dmeans2D_abs needs absgrad=True"):
            fused.backward(st, dpix, {}, dmeans2D_abs=torch.zeros(10, 3))
        for bad in (torch.zeros(10, 2), torch.zeros(10, 3, dtype=torch.float64), torch.zeros(3, 10).t()):
            with pytest.raises(RuntimeError, match="dmeans2D_abs must be a contiguous float32"):
                fused.backward(st, dpix, {}, absgrad=True, dmeans2D_abs=bad)


def test_stand_in_c_without_the_switch(monkeypatch):
    """A `_C` without absgrad() (the CPU oracle bound in its place) serves the signed gradients only."""
    import rain_amd.diff_gaussian_rasterization as dgr
    from tests import oracle_c

    monkeypatch.setattr(dgr, "_C", oracle_c)
    assert not dgr._absgrad_on()
    with dgr._absgrad(False):
        pass
    with pytest.raises(RuntimeError, match="absgrad needs the rasterizer's own _C"):
        dgr._absgrad(True)


def test_trainer_refusals():
    from rain_amd.renderer import PipelineParams
    from rain_amd.train import Trainer, resolve_options

    t = Trainer.__new__(Trainer)
    t.opt, t.pipe, t.sharded = OptimizationParams(densify_absgrad=True), PipelineParams(), True
    with pytest.raises(ValueError, match="densify_absgrad needs the single-GPU step"):
        resolve_options(t.opt, t.pipe, t.sharded)
    t.sharded = False
    assert resolve_options(t.opt, t.pipe, t.sharded).absgrad is True
    t.opt = OptimizationParams(densify_absgrad=True, densify_strategy="mcmc", cap_max=100)
    with pytest.raises(ValueError, match="densify_absgrad does not combine with densify_strategy 'mcmc'"):
        resolve_options(t.opt, t.pipe, t.sharded)
    for k in ("lambda_normal", "lambda_dist"):
        t.opt = OptimizationParams(densify_absgrad=True, **{k: 0.05})
        with pytest.raises(ValueError, match="densify_absgrad does not combine with lambda_normal / lambda_dist"):
            resolve_options(t.opt, t.pipe, t.sharded)
    t.opt, t.sharded = OptimizationParams(), True
    assert resolve_options(t.opt, t.pipe, t.sharded).absgrad is False
    assert "resolve_options(self.opt, self.pipe, self.sharded)" in inspect.getsource(Trainer.__init__)


def test_c_refusals_without_gpu():
    """Every refusal below happens before the library touches a device (the pointers are stand-ins)."""
    L = N.raster()
    ab = N.RR_FLAG_ABSGRAD
    f = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, ab)
    fraw = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, ab | N.RR_FLAG_RAW_PARAMS)
    f0 = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, 0)
    cam = N.RRCamera(16, 16, 16, 16)
    g = N.RRGaussians(16, 16, None, 16, 16, 16, None)
    out = N.RRGrads()
    head = lambda fr: (ctypes.byref(fr), ctypes.byref(cam), ctypes.byref(g), 16, 16, 16, 16, 5, 16)  # noqa: E731
    tail = (16, 1 << 20, ctypes.byref(out))

    def refused(rc, *words):
        msg = L.rr_last_error()
        assert rc == 1 and b"RR_FLAG_ABSGRAD" in msg, msg
        for w in words:
            assert w in msg, msg

    # the flag with any aux map, through every entry point that takes one
    for k in range(4):
        maps = [None] * 4
        maps[k] = 16
        for fr in (f, fraw):
            refused(L.rr_backward_aux_dist(*head(fr), *maps, 0.2, 100.0, *tail, None), b"depth / alpha / normal / moments")
    refused(L.rr_backward_aux(*head(f), 16, None, *tail, None), b"depth / alpha")
    refused(L.rr_backward_aux_normal(*head(f), None, None, 16, *tail, None), b"normal")
    # camera gradients
    cg = N.RRCameraGrads(16, 16, 16, 16, L.rr_camera_grad_scratch_bytes(10))
    refused(L.rr_backward_camera(*head(f), None, None, *tail, ctypes.byref(cg), None), b"rr_backward_camera")
    # the sharded step's two halves
    refused(L.rr_backward_records(ctypes.byref(f), ctypes.byref(cam), 16, 16, 16, 16, 5, 16, 16, 1 << 20, 0, 1, 16,
                                  None), b"rr_backward_records")
    view = N.RRView()
    refused(L.rr_gauss_backward_views(ctypes.byref(fraw), ctypes.byref(view), 1, ctypes.byref(g), 16, 10, 1.0,
                                      ctypes.byref(out), None), b"rr_gauss_backward_views")
    # the output without the flag
    out_abs = N.RRGrads()
    out_abs.dL_dmeans2D_abs = 16
    rc = L.rr_backward(*head(f0), 16, 1 << 20, ctypes.byref(out_abs), None)
    refused(rc, b"dL_dmeans2D_abs needs")
    rc = L.rr_gauss_backward_views(ctypes.byref(N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0,
                                                          N.RR_FLAG_RAW_PARAMS)), ctypes.byref(view), 1,
                                   ctypes.byref(g), 16, 10, 1.0, ctypes.byref(out_abs), None)
    refused(rc, b"dL_dmeans2D_abs needs")
    # with the flag, rr_backward and the aux entry points with every map NULL get past these refusals, to their
    # own next check; and so does a frame without the flag
    for call in (lambda o: L.rr_backward(*head(f), 16, 1 << 20, ctypes.byref(o), None),
                 lambda o: L.rr_backward_aux(*head(f), None, None, 16, 1 << 20, ctypes.byref(o), None),
                 lambda o: L.rr_backward_aux_dist(*head(f), None, None, None, None, 0.0, 0.0, 16, 1 << 20,
                                                  ctypes.byref(o), None),
                 lambda o: L.rr_backward_camera(*head(f), None, None, 16, 1 << 20, ctypes.byref(o), None, None)):
        for o in (out, out_abs):
            rc = call(o)
            assert rc == 1 and b"null gradient output" in L.rr_last_error(), L.rr_last_error()
    rc = L.rr_backward_aux_dist(*head(f0), 16, None, None, None, 0.0, 0.0, *tail, None)
    assert rc == 1 and b"RR_FLAG_ABSGRAD" not in L.rr_last_error()


def test_add_densification_stats_reads_absgrad():
    """On CPU tensors (the torch restatement): masked rows gain the norm of .absgrad, not of .grad."""
    g = GaussianModel(0, device="cpu")
    P = 7
    g.xyz_gradient_accum, g.denom = torch.full((P, 1), 0.5), torch.ones((P, 1))
    gen = torch.Generator().manual_seed(3)
    vsp = torch.zeros(P, 3, requires_grad=True)
    vsp.grad = torch.randn(P, 3, generator=gen)
    vsp.absgrad = torch.rand(P, 3, generator=gen) + vsp.grad.abs()
    mask = torch.tensor([True, False, True, True, False, False, True])
    g.add_densification_stats(vsp, mask, absgrad=True)
    want = 0.5 + torch.where(mask, torch.norm(vsp.absgrad[:, :2], dim=-1), torch.zeros(P))
    torch.testing.assert_close(g.xyz_gradient_accum[:, 0], want, rtol=0, atol=0)
    torch.testing.assert_close(g.denom[:, 0], 1.0 + mask.float(), rtol=0, atol=0)
    g.add_densification_stats(vsp, mask)  # the default still reads .grad
    want = want + torch.where(mask, torch.norm(vsp.grad[:, :2], dim=-1), torch.zeros(P))
    torch.testing.assert_close(g.xyz_gradient_accum[:, 0], want, rtol=0, atol=0)


def test_backward_plan_with_absgrad(tmp_path):
    """tests/host/absgrad_plan_check.hip, built with the product's compiler and include paths and run as a
    stand-alone program (no GPU): plan_backward(g, false, true) is the abs blend with the plain per-Gaussian
    kernel, and with the argument omitted every plan is unchanged."""
    exe = str(tmp_path / "absgrad_plan_check")
    cmd = [B.HIPCC, *B.CXXFLAGS, "-O1", os.path.join(HERE, "host", "absgrad_plan_check.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout and r.stdout.split()[0] == "130"
