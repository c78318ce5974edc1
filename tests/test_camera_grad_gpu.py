"""Camera-pose gradients (rr_backward_camera) on the GPU.

The reference is tests/camera_ref.py (float64, pinned by tests/test_camera_ref_cpu.py, which also holds
every scene here to kappa <= 50).  Bars: the project's parity bar of 1e-4 relative L1 against the
reference, 1e-5 between GPU runs that differ only in the order of their float atomics."""
import numpy as np
import pytest
import torch

from rain_amd import _native as N
from rain_amd import cameras
from rain_amd import renderer as renderer_mod
from rain_amd.renderer import PipelineParams, render
from tests.camera_ref import COMBOS, SCENES, camera_reference, chain_pose, combine, kappa, scene_reference
from tests.common import GRAD_NAMES, oracle_run, rel_l1
from tests.test_depth_grad_gpu import _backward_args, _forward, _gpu_inputs, _model, _settings, _trel

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 2], ids=["default_binning", "early_stop_split2"])
def binning(request):
    if request.param:
        N.check(N.raster().rr_set_binning_config(request.param, 1), "binning config")
    yield request.param
    N.check(N.raster().rr_set_binning_config(0, 0), "binning config")


def _check_zero_entries(d_view, d_proj):
    assert np.all(d_view.reshape(4, 4)[:, 3] == 0.0)  # memory 3, 7, 11, 15: read by no kernel
    assert np.all(d_proj.reshape(4, 4)[:, 2] == 0.0)  # the z row: 2, 6, 10, 14


@pytest.mark.parametrize("scene", list(SCENES))
def test_camera_gradient_parity(oracle, gpu, binning, scene):
    from rain_amd.diff_gaussian_rasterization import _C

    ref = scene_reference(oracle, scene)
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    fw = _forward(d, s)
    assert np.array_equal(fw[2].cpu().numpy(), ref["radii"])
    if scene == "clamp":
        assert ref["parts"]["colour"]["maps"]["clamped"].sum() > 0
    e = torch.Tensor([])
    maps = dict(colour=torch.from_numpy(ref["dpix"]).to(gpu), depth=torch.from_numpy(ref["dd"]).to(gpu),
                alpha=torch.from_numpy(ref["da"]).to(gpu))
    for combo, which in COMBOS.items():
        gp, gd, ga = (maps[k] if k in which else e for k in ("colour", "depth", "alpha"))
        got = _C.rasterize_gaussians_backward_camera(*_backward_args(d, s, fw, gp), gd, ga)
        torch.cuda.synchronize()
        assert len(got) == 11 and got[8].shape == (4, 4) and got[9].shape == (4, 4) and got[10].shape == (3,)
        d_view, d_proj, d_campos = (t.cpu().numpy() for t in got[8:])
        _check_zero_entries(d_view, d_proj)
        for name, g in (("view", d_view), ("proj", d_proj), ("campos", d_campos)):
            want = combine(ref["parts"], which, name)
            assert np.isfinite(g).all(), (combo, name)
            if np.abs(combine(ref["parts"], which, "S_" + name)).sum() == 0:  # precomputed colours, or no colour term
                assert name == "campos" and np.all(g == 0.0), (combo, name)
                continue
            err = rel_l1(g, want)
            print(f"{scene} {combo}: d_{name} rel L1 {err:.3e}")
            assert err <= 1e-4, f"{combo} d_{name}: rel L1 {err:.3e}"
        if combo == "all":
            # the Gaussians' gradients are the depth backward's, and a second run repeats the first
            plain = _C.rasterize_gaussians_backward_depth(*_backward_args(d, s, fw, gp), gd, ga)
            again = _C.rasterize_gaussians_backward_camera(*_backward_args(d, s, fw, gp), gd, ga)
            torch.cuda.synchronize()
            for k, a, b in zip(GRAD_NAMES, got[:8], plain):
                if a.numel():
                    assert rel_l1(a.cpu().numpy(), b.cpu().numpy()) <= 1e-5, k
            for k, a, b in zip(list(GRAD_NAMES) + ["d_view", "d_proj", "d_campos"], got, again):
                if a.numel():
                    assert rel_l1(a.cpu().numpy(), b.cpu().numpy()) <= 1e-5, k


def test_empty_frames_give_exact_zeros(oracle, gpu):
    from rain_amd.diff_gaussian_rasterization import _C

    ref = scene_reference(oracle, "tiny")
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    dpix = torch.from_numpy(ref["dpix"]).to(gpu)
    dd = torch.from_numpy(ref["dd"]).to(gpu)
    # every Gaussian behind the camera: the frame renders nothing
    back = dict(d, means3D=(2.0 * s["campos"][None] - d["means3D"]).contiguous())
    fw = _forward(back, s)
    assert int((fw[2] > 0).sum()) == 0
    got = _C.rasterize_gaussians_backward_camera(*_backward_args(back, s, fw, dpix), dd, torch.Tensor([]))
    for t in got[8:]:
        assert float(t.abs().max()) == 0.0
    assert float(got[3].abs().max()) == 0.0
    # no Gaussians at all
    none = {k: v[:0].contiguous() for k, v in d.items()}
    fw0 = _forward(none, s)
    got0 = _C.rasterize_gaussians_backward_camera(*_backward_args(none, s, fw0, dpix), dd, torch.Tensor([]))
    assert len(got0) == 11 and got0[3].shape == (0, 3)
    assert [tuple(t.shape) for t in got0[8:]] == [(4, 4), (4, 4), (3,)]
    for t in got0[8:]:
        assert float(t.abs().max()) == 0.0


def test_forward_camera_autograd(oracle, gpu):
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    ref = scene_reference(oracle, "sh3")
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    H, W = s["image_height"], s["image_width"]
    gen = torch.Generator().manual_seed(21)
    target = (3.0 + torch.rand((1, H, W), generator=gen)).to(gpu)
    w = torch.randn((3, H, W), generator=gen).to(gpu)
    v0, p0, c0 = (s[k].clone().requires_grad_() for k in ("viewmatrix", "projmatrix", "campos"))
    # the settings hold tensors computed from the leaves (the projection as a strided view)
    sc = dict(s, viewmatrix=v0 * 1.0, projmatrix=(p0.t().contiguous() * 1.0).t(), campos=c0 + 0.0)
    assert not sc["projmatrix"].is_contiguous()
    leaves = {k: d[k].clone().requires_grad_() for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    means2D = torch.zeros_like(d["means3D"]).requires_grad_()

    def loss_of(color, depth, alpha):
        return (depth / (alpha + 1e-6) - target).abs().mean() + (color * w).sum() + 0.1 * alpha.mean()

    color, radii, depth, alpha = GaussianRasterizer(_settings(sc)).forward_camera(
        leaves["means3D"], means2D, leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
        rotations=leaves["rotations"])
    assert color.requires_grad and depth.requires_grad and alpha.requires_grad and not radii.requires_grad
    loss_of(color, depth, alpha).backward()
    fw = _forward(d, s)
    assert torch.equal(fw[1], color.detach()) and torch.equal(fw[3], depth.detach())
    c, dp, al = (t.detach().clone().requires_grad_() for t in (color, depth, alpha))
    loss_of(c, dp, al).backward()
    byhand = _C.rasterize_gaussians_backward_camera(*_backward_args(d, s, fw, c.grad), dp.grad, al.grad)
    for name, leaf, g in (("view", v0, byhand[8]), ("proj", p0, byhand[9]), ("campos", c0, byhand[10])):
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape, name
        assert float(g.abs().sum()) > 0.0, name
        assert rel_l1(leaf.grad.cpu().numpy(), g.cpu().numpy()) <= 1e-5, name
    for leaf, k in (("means3D", 3), ("shs", 5), ("opacities", 2), ("scales", 6), ("rotations", 7)):
        assert rel_l1(leaves[leaf].grad.cpu().numpy(), byhand[k].cpu().numpy()) <= 1e-5, leaf
    # a fixed camera: the same outputs and Gaussian gradients (the plain depth backward), nothing for the camera
    leaves2 = {k: d[k].clone().requires_grad_() for k in leaves}
    out = GaussianRasterizer(_settings(s)).forward_camera(
        leaves2["means3D"], torch.zeros_like(d["means3D"]), leaves2["opacities"], shs=leaves2["shs"],
        scales=leaves2["scales"], rotations=leaves2["rotations"])
    assert torch.equal(out[0], color.detach()) and torch.equal(out[3], alpha.detach())
    loss_of(out[0], out[2], out[3]).backward()
    assert rel_l1(leaves2["means3D"].grad.cpu().numpy(), leaves["means3D"].grad.cpu().numpy()) <= 1e-5


def _activated_inputs(g):
    """The model's activated tensors as the oracle's inputs (CPU float32)."""
    with torch.no_grad():
        return dict(means3D=g.get_xyz.cpu().contiguous(), opacities=g.get_opacity.cpu().contiguous(),
                    shs=g.get_features.cpu().contiguous(), scales=g.get_scaling.cpu().contiguous(),
                    rotations=g.get_rotation.cpu().contiguous())


def test_render_pose_grad(oracle, gpu, monkeypatch):
    """render(pose_grad=True) on both routes: the six CameraPose gradients agree between the routes
    (1e-5) and with the float64 reference chained through a float64 CameraPose (1e-4), and its outputs
    are bitwise those of render(depth_grad=True)."""
    P, W, H = 3000, 128, 96
    cam = cameras.fibonacci_cameras(8, W, H)[5]
    delta = np.array([0.004, -0.003, 0.005, 0.02, -0.01, 0.015])
    bg = torch.tensor([0.3, 0.1, 0.2], device=gpu)
    gen = torch.Generator("cuda").manual_seed(9)
    wcol = torch.randn(3, H, W, device=gpu, generator=gen) / (3 * H * W)
    target = 3.0 + torch.rand(1, H, W, device=gpu, generator=gen)
    g = _model(P, 3, 3, seed=4)  # its parameters require gradients too: the joint pose-and-scene case
    results = []
    for raw in (True, False):
        monkeypatch.setattr(renderer_mod, "RAW_RENDER", raw)
        pose = cameras.CameraPose(cam.to("cuda"))
        with torch.no_grad():
            pose.rot_delta.copy_(torch.as_tensor(delta[:3], dtype=torch.float32))
            pose.trans_delta.copy_(torch.as_tensor(delta[3:], dtype=torch.float32))
        pkg = render(pose, g, PipelineParams(), bg, pose_grad=True)
        assert set(pkg) == {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha"}
        assert pkg["render"].grad_fn.__class__.__name__.startswith(
            "RasterizeRawParamsCamera" if raw else "_RasterizeGaussiansCamera")
        for k in ("render", "depth", "alpha"):
            pkg[k].retain_grad()
        loss = (pkg["render"] * wcol).sum() + 0.1 * (pkg["depth"] / (pkg["alpha"] + 1e-6) - target).abs().mean() \
            + 0.1 * pkg["alpha"].mean()
        loss.backward()
        six = torch.cat([pose.rot_delta.grad, pose.trans_delta.grad]).cpu().numpy().astype(np.float64)
        with torch.no_grad():
            same = render(pose, g, PipelineParams(), bg, depth_grad=True)
        for k in ("render", "depth", "alpha", "radii"):
            assert torch.equal(same[k], pkg[k].detach()), (raw, k)
        results.append((pose, pkg, six))
    (pose, pkg, six_raw), (_, pkg_b, six_getters) = results
    assert np.abs(six_raw).min() > 0.0
    e_routes = rel_l1(six_getters, six_raw)
    print(f"pose gradients: raw {six_raw}, getters {six_getters}, rel L1 {e_routes:.3e}")
    assert e_routes <= 1e-5
    # the reference at the matrices the rasterizer was given, with the output gradients autograd formed
    st = dict(image_height=H, image_width=W, tanfovx=float(np.tan(cam.FoVx * 0.5)), tanfovy=float(np.tan(cam.FoVy * 0.5)),
              bg=bg.cpu(), scale_modifier=1.0, viewmatrix=pose.world_view_transform.detach().cpu().contiguous(),
              projmatrix=pose.full_proj_transform.detach().cpu().contiguous(), sh_degree=3,
              campos=pose.camera_center.detach().cpu().contiguous(), prefiltered=False, debug=False, low_pass=0.3)
    inp = _activated_inputs(g)
    fw = oracle_run(oracle, inp, st)
    assert np.array_equal(fw["radii"], pkg["radii"].cpu().numpy())
    douts = dict(all=tuple(pkg[k].grad.cpu().numpy() for k in ("render", "depth", "alpha")))
    r = camera_reference(st, inp, fw["state"].blend_lists(), douts)["all"]
    k = kappa(r)
    print(f"render(pose_grad) scene: kappa {k}")
    assert max(k.values()) <= 50.0  # the condition of tests/test_camera_ref_cpu.py, on this scene
    pose64 = cameras.CameraPose(cam, dtype=torch.float64)
    with torch.no_grad():
        pose64.rot_delta.copy_(torch.as_tensor(delta[:3]))
        pose64.trans_delta.copy_(torch.as_tensor(delta[3:]))
    want = chain_pose(pose64, r)
    err = rel_l1(six_raw, want)
    print(f"pose gradients: reference {want}, rel L1 {err:.3e}")
    assert err <= 1e-4
    assert _trel(pkg_b["render"], pkg["render"]) < 1e-6
