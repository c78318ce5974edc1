"""CPU checks of the anti-aliasing surface (include/rain_raster.h RR_FLAG_ANTIALIAS): the flag's value, how
the switch reaches every layer without touching the pinned signatures, and every refusal, each of which comes
back before the library or the Python layer touches a device."""
import ctypes
import inspect
import re

import pytest
import torch

from rain_amd import _native as N
from rain_amd import cameras, fused
from rain_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C
from rain_amd.renderer import PipelineParams, render


def test_flag_value_and_header():
    assert N.RR_FLAG_ANTIALIAS == 32
    flags = [N.RR_FLAG_NO_TILE_CULLING, N.RR_FLAG_RAW_PARAMS, N.RR_FLAG_FULL_BINNING, N.RR_FLAG_AUX_NORMAL,
             N.RR_FLAG_WORKSPACE_REGISTERED, N.RR_FLAG_ANTIALIAS]
    assert sorted(flags) == [1, 2, 4, 8, 16, 32]
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "rain_raster.h")).read()
    assert re.search(r"#define\s+RR_FLAG_ANTIALIAS\s+32\b", header)
    for name in ("rr_preprocess_rows", "rr_preprocess_rows_views", "rr_gauss_backward_views", "rr_backward_camera"):
        assert name in header.split("#define RR_FLAG_ANTIALIAS")[0].rsplit("Anti-aliased rendering", 1)[1], name


def test_settings_keep_their_13_fields():
    assert GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug", "low_pass")


def test_switch_sets_the_frame_flag_and_nests():
    def flag():
        return _C._frame(1, 0, 1, 8, 8, 1.0, 1.0, 1.0, 0.3, False, False).flags & N.RR_FLAG_ANTIALIAS

    assert not _C.antialiasing_on() and flag() == 0
    with _C.antialiased():
        assert _C.antialiasing_on() and flag() == 32
        with _C.antialiased(False):
            assert flag() == 0
        assert flag() == 32
    assert not _C.antialiasing_on() and flag() == 0
    with pytest.raises(KeyError):  # restored on the way out of a failing block too
        with _C.antialiased():
            raise KeyError
    assert flag() == 0


def test_python_surface():
    sig = inspect.signature(GaussianRasterizer.__init__).parameters
    assert list(sig) == ["self", "raster_settings", "antialiasing"] and sig["antialiasing"].default is False
    assert PipelineParams().antialiasing is False
    assert PipelineParams(antialiasing=True).antialiasing is True
    for fn in (fused.forward, fused.forward_params, fused.prepare_next):
        assert inspect.signature(fn).parameters["antialiasing"].default is False
    from rain_amd import compact, render_views

    for mod in (compact, render_views):
        assert "--antialiasing" in inspect.getsource(mod.main)


def _settings():
    return GaussianRasterizationSettings(
        image_height=48, image_width=64, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0,
        viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False,
        debug=False, low_pass=0.3)


def test_python_refusals_without_gpu():
    r = GaussianRasterizer(_settings(), antialiasing=True)
    assert r.antialiasing is True and GaussianRasterizer(_settings()).antialiasing is False
    m = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="forward_camera does not combine with antialiasing"):
        r.forward_camera(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3), scales=m,
                         rotations=torch.zeros(5, 4))
    # the other modes still reach the device check (no CPU fallback), with the switch on
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.forward(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3), scales=m,
                  rotations=torch.zeros(5, 4))
    assert not _C.antialiasing_on()
    e = torch.Tensor([])
    with _C.antialiased():
        with pytest.raises(RuntimeError, match="camera gradients do not combine with antialiasing"):
            _C.rasterize_gaussians_backward_camera(*([e] * 24))
    cam = cameras.fibonacci_cameras(8, 64, 48)[0]
    with pytest.raises(ValueError, match="pose_grad=True.*antialiasing"):
        render(cam, None, PipelineParams(antialiasing=True), torch.zeros(3), pose_grad=True)
    from rain_amd import pose

    with pytest.raises(ValueError, match="refine_pose does not combine with pipe.antialiasing"):
        pose.refine_pose(cam, None, PipelineParams(antialiasing=True), torch.zeros(3), torch.zeros(3, 48, 64), 1, 1e-3)
    st = fused.RawFrame(N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, N.RR_FLAG_RAW_PARAMS | 32), None, None,
                        (), None, None, None, None, 0, 10, 1)
    cg = (torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(3))
    with pytest.raises(RuntimeError, match="camera gradients do not combine with antialiasing"):
        fused.backward(st, torch.zeros(3, 48, 64), {}, cam_grads=cg)


def test_sharded_trainers_refuse_at_construction():
    from rain_amd.gaussian_model import OptimizationParams
    from rain_amd.train import Trainer, resolve_options

    t = Trainer.__new__(Trainer)
    t.opt, t.pipe, t.sharded = OptimizationParams(), PipelineParams(antialiasing=True), True
    with pytest.raises(ValueError, match="pipe.antialiasing needs the single-GPU step"):
        resolve_options(t.opt, t.pipe, t.sharded)
    t.sharded = False
    assert resolve_options(t.opt, t.pipe, t.sharded).antialiasing is True
    t.pipe = PipelineParams()
    assert resolve_options(t.opt, t.pipe, t.sharded).antialiasing is False
    assert "resolve_options(self.opt, self.pipe, self.sharded)" in inspect.getsource(Trainer.__init__)


def test_c_refusals_without_gpu():
    """Every refusal below happens before the library touches a device (the pointers are stand-ins)."""
    L = N.raster()
    aa = N.RR_FLAG_ANTIALIAS
    f = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, aa)
    fraw = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, aa | N.RR_FLAG_RAW_PARAMS)
    cam = N.RRCamera(16, 16, 16, 16)
    g = N.RRGaussians(16, 16, None, 16, 16, 16, None)
    out = N.RRGrads()
    cg = N.RRCameraGrads(16, 16, 16, 16, L.rr_camera_grad_scratch_bytes(10))
    rc = L.rr_backward_camera(ctypes.byref(f), ctypes.byref(cam), ctypes.byref(g), 16, 16, 16, 16, 5, 16, 16, 16, 16,
                              1 << 20, ctypes.byref(out), ctypes.byref(cg), None)
    assert rc == 1 and b"RR_FLAG_ANTIALIAS" in L.rr_last_error() and b"camera" in L.rr_last_error()
    # cg == NULL is rr_backward_aux, which honours the flag: it gets as far as the next check
    rc = L.rr_backward_camera(ctypes.byref(f), ctypes.byref(cam), ctypes.byref(g), 16, 16, 16, 16, 5, 16, 16, 16, 16,
                              1 << 20, ctypes.byref(out), None, None)
    assert rc == 1 and b"null gradient output" in L.rr_last_error()
    rc = L.rr_preprocess_rows(ctypes.byref(f), ctypes.byref(cam), ctypes.byref(g), 256, 16, 16, 16, 16, 16, 16, None)
    assert rc == 1 and b"RR_FLAG_ANTIALIAS" in L.rr_last_error() and b"row blocks" in L.rr_last_error()
    view = N.RRView()
    offs = (ctypes.c_size_t * 6)(0, 0, 0, 0, 0, 0)
    rc = L.rr_preprocess_rows_views(ctypes.byref(fraw), ctypes.byref(view), 1, ctypes.byref(g), 256, 16, 0, offs, 0,
                                    None)
    assert rc == 1 and b"RR_FLAG_ANTIALIAS" in L.rr_last_error() and b"row blocks" in L.rr_last_error()
    rc = L.rr_gauss_backward_views(ctypes.byref(fraw), ctypes.byref(view), 1, ctypes.byref(g), 16, 10, 1.0,
                                   ctypes.byref(out), None)
    assert rc == 1 and b"RR_FLAG_ANTIALIAS" in L.rr_last_error() and b"sharded backward" in L.rr_last_error()
    # without the flag the same calls get past these refusals (to their own next check)
    f0 = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, N.RR_FLAG_RAW_PARAMS)
    rc = L.rr_gauss_backward_views(ctypes.byref(f0), ctypes.byref(view), 0, ctypes.byref(g), 16, 10, 1.0,
                                   ctypes.byref(out), None)
    assert rc == 1 and b"RR_FLAG_ANTIALIAS" not in L.rr_last_error()
