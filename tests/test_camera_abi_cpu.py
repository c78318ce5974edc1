"""CPU checks of the camera-gradient surface: the C ABI exports and lists rr_backward_camera and
rr_camera_grad_scratch_bytes, every refusal comes back before the library touches a device, the
Python layers have the documented signatures and messages, and CameraPose is differentiable and
equals its base camera at zero deltas."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from rain_amd import _native as N
from rain_amd import cameras
from rain_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C


def test_new_symbols_exported_and_listed():
    so = ctypes.CDLL(N.RASTER_LIB)
    for name in ("rr_backward_camera", "rr_camera_grad_scratch_bytes"):
        assert hasattr(so, name), f"librain_raster.so does not export {name}"
        assert name in N.RASTER_SYMBOLS
    L = N.raster()
    aux, cam = L.rr_backward_aux.argtypes, L.rr_backward_camera.argtypes
    # rr_backward_aux's arguments with the camera-gradient block before the stream
    assert len(cam) == len(aux) + 1 and list(cam[:-2]) == list(aux[:-1]) and cam[-1] is aux[-1]
    assert [f[0] for f in N.RRCameraGrads._fields_] == ["dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos", "scratch",
                                                        "scratch_bytes"]
    # one 32-float row per workgroup of 256 Gaussians, at least one
    assert L.rr_camera_grad_scratch_bytes(0) == L.rr_camera_grad_scratch_bytes(256) >= 128
    assert L.rr_camera_grad_scratch_bytes(257) >= 256
    assert L.rr_camera_grad_scratch_bytes(1_000_000) >= 3907 * 128


def test_rr_backward_camera_validation_without_gpu():
    """Every refusal below happens before the library touches a device (the pointers are stand-ins)."""
    L = N.raster()
    f = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0)
    fraw = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0, N.RR_FLAG_RAW_PARAMS)
    cam = N.RRCamera(1, 1, 1, 1)
    g = N.RRGaussians(16, 16, None, 16, 16, 16, None)
    out = N.RRGrads()
    need = L.rr_camera_grad_scratch_bytes(10)

    def call(frame, grads, cg, dpix=16, dd=16, da=16):
        return L.rr_backward_camera(ctypes.byref(frame) if frame is not None else None, ctypes.byref(cam),
                                    ctypes.byref(g), 16, 16, 16, 16, 5, dpix, dd, da, 16, 1 << 20,
                                    ctypes.byref(grads) if grads is not None else None,
                                    ctypes.byref(cg) if cg is not None else None, None)

    ok = N.RRCameraGrads(16, 16, 16, 16, need)
    assert call(None, out, ok) == 1 and b"null frame" in L.rr_last_error()
    for i in range(3):  # all three outputs are required
        cg = N.RRCameraGrads(*[None if j == i else 16 for j in range(3)], 16, need)
        assert call(f, out, cg) == 1 and b"rr_camera_grads: null gradient output" in L.rr_last_error()
    assert call(f, out, N.RRCameraGrads(16, 16, 16, None, need)) == 1 and b"scratch" in L.rr_last_error()
    assert call(f, out, N.RRCameraGrads(16, 16, 16, 24, need)) == 1 and b"16-byte aligned" in L.rr_last_error()
    # too small a scratch: RR_ERR_CAPACITY (3)
    assert call(f, out, N.RRCameraGrads(16, 16, 16, 16, need - 1)) == 3 and b"scratch too small" in L.rr_last_error()
    # the fused optimizer step and the next frame get no camera variant
    ad, nx = N.RRAdam(), N.RRNextFrame()
    out_ad = N.RRGrads()
    out_ad.adam = ctypes.pointer(ad)
    assert call(fraw, out_ad, ok) == 1 and b"rr_grads.adam / rr_grads.next" in L.rr_last_error()
    out_nx = N.RRGrads()
    out_nx.next = ctypes.pointer(nx)
    assert call(fraw, out_nx, ok) == 1 and b"rr_grads.adam / rr_grads.next" in L.rr_last_error()
    # past the camera block the call validates like rr_backward_aux
    assert call(f, None, ok) == 1 and b"null buffer" in L.rr_last_error()
    assert call(f, out, ok, dpix=None, dd=None, da=None) == 1 and b"null buffer" in L.rr_last_error()
    assert call(f, out, ok) == 1 and b"null gradient output" in L.rr_last_error()
    assert call(f, out, ok, dd=None, da=None) == 1 and b"null gradient output" in L.rr_last_error()  # colour only
    # cg == NULL is rr_backward_aux: the same refusals, and P == 0 is a no-op success
    assert call(f, out, None) == 1 and b"null gradient output" in L.rr_last_error()
    f0 = N.RRFrame(0, 0, 0, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0)
    assert call(f0, out, None) == 0


def test_python_surface_exists():
    p = list(inspect.signature(_C.rasterize_gaussians_backward_camera).parameters)
    assert p == list(inspect.signature(_C.rasterize_gaussians_backward_depth).parameters)
    assert list(inspect.signature(GaussianRasterizer.forward_camera).parameters) == \
        list(inspect.signature(GaussianRasterizer.forward_depth).parameters)
    from rain_amd import diff_gaussian_rasterization as dgr
    from rain_amd import fused, pose, renderer

    assert hasattr(dgr, "_RasterizeGaussiansCamera") and hasattr(fused, "RasterizeRawParamsCamera")
    assert inspect.signature(fused.backward).parameters["cam_grads"].default is None
    assert inspect.signature(renderer.render).parameters["pose_grad"].default is False
    assert list(inspect.signature(pose.refine_pose).parameters) == [
        "camera", "pc", "pipe", "bg", "target_image", "iters", "lr", "target_depth", "low_pass"]
    sig = inspect.signature(pose.refine_pose).parameters
    assert sig["target_depth"].default is None and sig["low_pass"].default == 0.3


def _settings():
    return GaussianRasterizationSettings(
        image_height=48, image_width=64, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0,
        viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False,
        debug=False, low_pass=0.3)


def test_forward_camera_argument_messages_and_no_cpu_fallback():
    r = GaussianRasterizer(_settings())
    m = torch.zeros(5, 3)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r.forward_camera(means3D=m, means2D=m, opacities=torch.zeros(5, 1), scales=m, rotations=torch.zeros(5, 4))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        r.forward_camera(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.forward_camera(means3D=m, means2D=m, opacities=torch.zeros(5, 1), shs=torch.zeros(5, 1, 3), scales=m,
                         rotations=torch.zeros(5, 4))


def test_render_pose_grad_does_not_combine_with_normal_or_dist():
    from rain_amd.renderer import PipelineParams, render

    cam = cameras.fibonacci_cameras(8, 64, 48)[0]
    for kw in (dict(normal_grad=True), dict(dist_grad=True), dict(normal_grad=True, dist_grad=True)):
        with pytest.raises(Exception) as e:
            render(cam, None, PipelineParams(), torch.zeros(3), pose_grad=True, **kw)
        assert str(e.value) == "render(pose_grad=True) does not combine with normal_grad / dist_grad yet"


def test_fused_backward_refuses_camera_with_normal_moments_adam():
    from rain_amd import fused

    cg = (torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(3))
    z = torch.zeros(3, 4, 4)
    with pytest.raises(RuntimeError, match="do not combine with dL_dnormal / dL_dmoments"):
        fused.backward(None, z, {}, dL_dnormal=z, cam_grads=cg)
    with pytest.raises(RuntimeError, match="do not combine with dL_dnormal / dL_dmoments"):
        fused.backward(None, z, {}, dL_dmoments=z[:2], cam_grads=cg)
    with pytest.raises(RuntimeError, match="do not combine with the fused optimizer step"):
        fused.backward(None, z, None, adam=N.RRAdam(), cam_grads=cg)


def test_camera_pose_equals_base_camera_at_zero_deltas():
    for cam in cameras.fibonacci_cameras(8, 64, 48):
        pose = cameras.CameraPose(cam)
        assert [n for n, _ in pose.named_parameters()] == ["rot_delta", "trans_delta"]
        assert all(float(p.detach().abs().max()) == 0.0 and p.shape == (3,) for p in pose.parameters())
        wvt, fpt = pose.world_view_transform, pose.full_proj_transform
        assert wvt.is_contiguous() and wvt.requires_grad and fpt.requires_grad and pose.camera_center.requires_grad
        assert wvt.detach().numpy().tobytes() == cam.world_view_transform.numpy().tobytes()
        assert fpt.detach().numpy().tobytes() == cam.full_proj_transform.numpy().tobytes()
        assert torch.allclose(pose.camera_center.detach(), cam.camera_center, atol=1e-5)
        assert (pose.FoVx, pose.FoVy, pose.image_width, pose.image_height) == \
            (cam.FoVx, cam.FoVy, cam.image_width, cam.image_height)


def test_camera_pose_gradcheck_and_closed_form_centre():
    cam = cameras.fibonacci_cameras(8, 64, 48)[3]

    def outputs(rot, trans):  # the module evaluated on gradcheck's own leaves in place of its parameters
        p = cameras.CameraPose(cam, dtype=torch.float64)
        del p._parameters["rot_delta"], p._parameters["trans_delta"]
        p.rot_delta, p.trans_delta = rot, trans
        return p.world_view_transform, p.full_proj_transform, p.camera_center

    for x in (np.zeros(6), np.array([0.3, -0.2, 0.5, 0.1, -0.4, 0.2])):
        rot = torch.tensor(x[:3], dtype=torch.float64, requires_grad=True)
        trans = torch.tensor(x[3:], dtype=torch.float64, requires_grad=True)
        assert torch.autograd.gradcheck(outputs, (rot, trans), eps=1e-6, atol=1e-8)
        wvt, _fpt, centre = outputs(rot, trans)
        assert torch.isfinite(torch.autograd.grad(wvt.sum() + centre.sum(), [rot, trans])[0]).all()
        # -R'^T t' is the translation row of the inverse
        assert torch.allclose(centre, wvt.inverse()[3, :3], atol=1e-12)
        Rn = wvt[:3, :3]
        assert torch.allclose(Rn @ Rn.T, torch.eye(3, dtype=torch.float64), atol=1e-6)  # (the base R is fp32)
