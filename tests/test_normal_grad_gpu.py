"""Differentiable aux normal map (rr_backward_aux_normal) on the GPU.

The reference is the existing oracle plus float64 autograd (tests/normal_ref.py, pinned by
tests/test_normal_ref_cpu.py): a render with colours n_i over a zero background is the normal map,
so the oracle's backward of that run gives the normal term's alpha-path gradients and dL/dn_i, and
float64 autograd of n_i(rotations) gives the direct rotation term.  Bars: the project's parity bar
of 1e-4 relative L1 against the reference, 1e-5 between GPU runs that differ only in the order of
their float atomics."""
import numpy as np
import pytest
import torch

from rain_amd import cameras, fused
from rain_amd import renderer as renderer_mod
from rain_amd.gaussian_model import OptimizationParams
from rain_amd.loss import l1_ssim_backward, l1_ssim_forward
from rain_amd.renderer import PipelineParams, render
from tests.common import GRAD_NAMES, oracle_settings, rel_l1
from tests.normal_ref import SCENES, full_reference, perturbed_scene
# the depth file's binning fixture (default, and early-stop split 2 with min_pairs 1) and helpers
from tests.test_depth_grad_gpu import (NAMES, _depth_loss, _gpu_inputs, _model, _params, _settings,  # noqa: F401
                                       _trel, binning)

pytestmark = pytest.mark.gpu


_REF = {}


def _reference(oracle, name):
    """Per scene, computed once and left unchanged: the perturbed inputs, random output gradients,
    the oracle's colour-run gradients and the depth, alpha and normal contributions."""
    if name in _REF:
        return _REF[name]
    inp, st = perturbed_scene(**SCENES[name])
    H, W = st["image_height"], st["image_width"]
    rng = np.random.default_rng(11)
    dpix = rng.standard_normal((3, H, W)).astype(np.float32)
    dd = rng.standard_normal((1, H, W)).astype(np.float32)
    da = rng.standard_normal((1, H, W)).astype(np.float32)
    dn = rng.standard_normal((3, H, W)).astype(np.float32)
    full = full_reference(oracle, inp, st, dpix, dd, da, dn)
    n = {k: v.numpy() for k, v in inp.items()}
    nmap = oracle.forward(oracle_settings(oracle, st), n["means3D"], n["opacities"], shs=n["shs"], scales=n["scales"],
                          rotations=n["rotations"], normal=True)[5]
    _REF[name] = dict(inp=inp, st=st, dpix=dpix, dd=dd, da=da, dn=dn, radii=full["col"]["radii"], nmap=nmap,
                      colour=full["colour"], parts=full["parts"])
    return _REF[name]


def _forward_args(d, s):
    e = torch.Tensor([])
    return (s["bg"], d["means3D"], e, d["opacities"], d["scales"], d["rotations"], s["scale_modifier"], e,
            s["viewmatrix"], s["projmatrix"], s["tanfovx"], s["tanfovy"], s["image_height"], s["image_width"],
            d["shs"], s["sh_degree"], s["campos"], s["prefiltered"], s["debug"], s["low_pass"])


def _forward_aux(d, s):
    """(num_rendered, color, radii, depth, normal, geom, binning, img)"""
    from rain_amd.diff_gaussian_rasterization import _C

    return _C.rasterize_gaussians_aux(*_forward_args(d, s))


def _backward_args(d, s, fw, dpix):
    e = torch.Tensor([])
    nr, _color, radii, _depth, _normal, geom, binb, img = fw
    return (s["bg"], d["means3D"], radii, e, d["scales"], d["rotations"], s["scale_modifier"], e, s["viewmatrix"],
            s["projmatrix"], s["tanfovx"], s["tanfovy"], dpix, d["shs"], s["sh_degree"], s["campos"], geom, nr, binb,
            img, False, s["low_pass"])


@pytest.mark.parametrize("scene", list(SCENES))
def test_forward_surface(oracle, gpu, binning, scene):
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    ref = _reference(oracle, scene)
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    H, W = s["image_height"], s["image_width"]
    plain = _C.rasterize_gaussians(*_forward_args(d, s))
    aux = _forward_aux(d, s)
    with torch.no_grad():
        color, radii, depth, alpha, normal = GaussianRasterizer(_settings(s)).forward_normal(
            d["means3D"], torch.zeros_like(d["means3D"]), d["opacities"], shs=d["shs"], scales=d["scales"],
            rotations=d["rotations"])
    assert torch.equal(color, plain[1]) and torch.equal(radii, plain[2]) and torch.equal(depth, plain[3])
    assert torch.equal(alpha, _C.accumulated_alpha(plain[6], H, W))
    assert normal.shape == (3, H, W) and torch.equal(normal, aux[4])
    e = rel_l1(normal.cpu().numpy(), ref["nmap"])
    print(f"{scene}: normal map rel L1 {e:.3e}")
    assert e <= 1e-4
    tile_max = _C.debug_views(aux[5], aux[6], aux[7], aux[0], d["means3D"].shape[0], W, H)["tile_max"]
    assert int(tile_max.max()) > 64, "the scene must walk more than one 64-pair round"


@pytest.mark.parametrize("scene", list(SCENES))
def test_gradient_parity(oracle, gpu, binning, scene):
    """Measured on an MI355X over the scenes, binnings and combinations: worst relative L1 5.9e-6
    (dL_dcov3D), dL_drotations 2.8e-6 or less."""
    from rain_amd.diff_gaussian_rasterization import _C

    ref = _reference(oracle, scene)
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    fw = _forward_aux(d, s)
    assert np.array_equal(fw[2].cpu().numpy(), ref["radii"])
    dpix, dd, da, dn = (torch.from_numpy(ref[k]).to(gpu) for k in ("dpix", "dd", "da", "dn"))
    e = torch.Tensor([])
    hidden = ref["radii"] == 0
    for label, gp, gd, ga in (("all", dpix, dd, da), ("normal_only", e, e, e), ("colour+normal", dpix, e, e)):
        got = _C.rasterize_gaussians_backward_normal(*_backward_args(d, s, fw, gp), gd, ga, dn)
        torch.cuda.synchronize()
        got = dict(zip(GRAD_NAMES, (g.cpu().numpy() for g in got)))
        for k, g in got.items():
            want = ref["parts"]["normal"][k].copy()
            if gp.numel():
                want += ref["colour"][k]
            if gd.numel():
                want += ref["parts"]["depth"][k]
            if ga.numel():
                want += ref["parts"]["alpha"][k]
            assert g.shape == want.shape, (label, k)
            assert np.isfinite(g).all(), (label, k)
            assert np.abs(g[hidden]).sum() == 0.0, (label, k)  # Gaussians the forward did not keep: exact zeros
            if np.abs(want).sum() == 0:  # dL_dsh / dL_dcolors without a colour gradient
                assert label == "normal_only" and k in ("dL_dsh", "dL_dcolors"), (label, k)
                assert np.abs(g).max() == 0.0, (label, k)
                continue
            err = rel_l1(g, want)
            print(f"{scene} {label}: {k} rel L1 {err:.3e}")
            assert err <= 1e-4, f"{label} {k}: rel L1 {err:.3e}"
        if label == "normal_only":
            assert np.abs(got["dL_dsh"]).max() == 0.0 and np.abs(got["dL_dcolors"]).max() == 0.0
            assert np.abs(got["dL_drotations"]).sum() > 0.0


def test_absent_or_zero_normal_gradient_changes_nothing(oracle, gpu, binning):
    from rain_amd.diff_gaussian_rasterization import _C

    ref = _reference(oracle, "sh3")
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    H, W = s["image_height"], s["image_width"]
    fw = _forward_aux(d, s)
    dpix, dd, da = (torch.from_numpy(ref[k]).to(gpu) for k in ("dpix", "dd", "da"))
    args = _backward_args(d, s, fw, dpix)
    depth = _C.rasterize_gaussians_backward_depth(*args, dd, da)
    absent = _C.rasterize_gaussians_backward_normal(*args, dd, da, torch.Tensor([]))
    zeros = _C.rasterize_gaussians_backward_normal(*args, dd, da, torch.zeros((3, H, W), device=gpu))
    for k, p, a, b in zip(GRAD_NAMES, depth, absent, zeros):
        assert rel_l1(a.cpu().numpy(), p.cpu().numpy()) <= 1e-5, k
        assert rel_l1(b.cpu().numpy(), p.cpu().numpy()) <= 1e-5, k


def test_autograd_surface(oracle, gpu):
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    ref = _reference(oracle, "sh3")
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    H, W = s["image_height"], s["image_width"]
    gen = torch.Generator().manual_seed(21)
    target = (3.0 + torch.rand((1, H, W), generator=gen)).to(gpu)
    w = torch.randn((3, H, W), generator=gen).to(gpu)
    ntarget = torch.nn.functional.normalize(torch.randn((3, H, W), generator=gen), dim=0).to(gpu)
    leaves = {k: d[k].clone().requires_grad_() for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    means2D = torch.zeros_like(d["means3D"]).requires_grad_()
    r = GaussianRasterizer(_settings(s))

    def run(fn):
        return fn(leaves["means3D"], means2D, leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
                  rotations=leaves["rotations"])

    def loss_of(color, depth, alpha, normal):
        return (depth / (alpha + 1e-6) - target).abs().mean() + (color * w).sum() \
            + (1.0 - (normal * ntarget).sum(0)).mean()

    color, radii, depth, alpha, normal = run(r.forward_normal)
    assert all(t.requires_grad for t in (color, depth, alpha, normal)) and not radii.requires_grad
    loss_of(color, depth, alpha, normal).backward()
    # the same output gradients fed to _C by hand
    fw = _forward_aux(d, s)
    assert torch.equal(fw[1], color.detach()) and torch.equal(fw[4], normal.detach())
    c, dp, al, nm = (t.detach().clone().requires_grad_() for t in (color, depth, alpha, normal))
    loss_of(c, dp, al, nm).backward()
    byhand = dict(zip(GRAD_NAMES, _C.rasterize_gaussians_backward_normal(*_backward_args(d, s, fw, c.grad), dp.grad,
                                                                        al.grad, nm.grad)))
    pairs = (("means3D", "dL_dmeans3D"), ("shs", "dL_dsh"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"),
             ("rotations", "dL_drotations"))
    for leaf, k in pairs:
        err = rel_l1(leaves[leaf].grad.cpu().numpy(), byhand[k].cpu().numpy())
        assert err <= 1e-5, (leaf, err)
    assert rel_l1(means2D.grad.cpu().numpy(), byhand["dL_dmeans2D"].cpu().numpy()) <= 1e-5

    # a loss on the normal alone: the other three arrive as absent gradients (no zero maps)
    for t in list(leaves.values()) + [means2D]:
        t.grad = None
    color, radii, depth, alpha, normal = run(r.forward_normal)
    (normal * ntarget).sum().backward()
    e = torch.Tensor([])
    only = dict(zip(GRAD_NAMES, _C.rasterize_gaussians_backward_normal(*_backward_args(d, s, fw, e), e, e, ntarget)))
    for leaf, k in pairs:
        assert rel_l1(leaves[leaf].grad.cpu().numpy(), only[k].cpu().numpy()) <= 1e-5, leaf
    assert float(only["dL_dsh"].abs().max()) == 0.0 and float(only["dL_dcolors"].abs().max()) == 0.0
    assert float(only["dL_drotations"].abs().sum()) > 0.0

    # forward() and forward_depth() are unchanged: same outputs, same number of outputs
    with torch.no_grad():
        out = run(r)
        outd = run(r.forward_depth)
    assert len(out) == 3 and len(outd) == 4
    assert torch.equal(out[0], color.detach()) and torch.equal(out[1], radii) and torch.equal(out[2], depth.detach())
    assert torch.equal(outd[0], color.detach()) and torch.equal(outd[2], depth.detach())
    assert torch.equal(outd[3], alpha.detach())


def _normal_loss(normal, ntarget):
    return (1.0 - (normal * ntarget).sum(0)).mean()


def test_render_normal_grad_routes_agree(gpu, monkeypatch):
    """render(normal_grad=True) on the raw-parameter route and on the getters route: outputs, the six
    leaf gradients and viewspace_points.grad (bars of test_render_depth_grad_routes_agree)."""
    P, W, H = 30_000, 200, 150
    cam = cameras.fibonacci_cameras(8, W, H)[5].to("cuda")
    bg = torch.tensor([0.3, 0.1, 0.2], device="cuda")
    gen = torch.Generator("cuda").manual_seed(9)
    wcol = torch.randn(3, H, W, device="cuda", generator=gen) / (3 * H * W)
    target = 3.0 + torch.rand(1, H, W, device="cuda", generator=gen)
    ntarget = torch.nn.functional.normalize(torch.randn(3, H, W, device="cuda", generator=gen), dim=0)
    outs = []
    for raw in (False, True):
        monkeypatch.setattr(renderer_mod, "RAW_RENDER", raw)
        g = _model(P, 3, 3, seed=4)
        pkg = render(cam, g, PipelineParams(), bg, normal_grad=True)
        assert set(pkg) == {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha", "normal"}
        assert pkg["render"].grad_fn.__class__.__name__.startswith("RasterizeRawParamsNormal") == raw
        assert pkg["depth"].requires_grad and pkg["alpha"].requires_grad and pkg["normal"].requires_grad
        assert pkg["normal"].shape == (3, H, W)
        loss = (pkg["render"] * wcol).sum() + _depth_loss(pkg["depth"], pkg["alpha"], target) \
            + 0.1 * pkg["alpha"].mean() + _normal_loss(pkg["normal"], ntarget)
        loss.backward()
        outs.append((pkg, {k: v.grad.clone() for k, v in _params(g).items()}))
    (pa, ga), (pb, gb) = outs
    assert torch.equal(pa["radii"], pb["radii"])
    for k in ("render", "depth", "alpha", "normal"):
        assert _trel(pb[k], pa[k]) < 1e-6, k
    for k in NAMES:
        assert torch.isfinite(gb[k]).all(), k
        assert float(ga[k].abs().sum()) > 0.0, k
        assert _trel(gb[k], ga[k]) < 1e-4, (k, _trel(gb[k], ga[k]))
    va, vb = pa["viewspace_points"].grad, pb["viewspace_points"].grad
    assert vb.shape == va.shape == (P, 3) and float(vb[:, 2].abs().max()) == 0.0
    assert _trel(vb, va) < 1e-4
    # the default call is unchanged: neither map, a depth without gradient
    plain = render(cam, g, PipelineParams(), bg)
    assert "normal" not in plain and "alpha" not in plain and not plain["depth"].requires_grad


def test_adam_fused_into_normal_backward_matches_separate_step(gpu):
    """test_adam_fused_into_depth_backward_matches_separate_step with a normal term in the loss: the
    step applied inside rr_backward_aux_normal equals gradients written out + FusedAdam.step()."""
    P, W, H = 20_000, 160, 120
    cam = cameras.fibonacci_cameras(8, W, H)[2].to("cuda")
    bg = torch.zeros(3, device="cuda")
    gen = torch.Generator("cuda").manual_seed(9)
    gt = torch.rand(3, H, W, device="cuda", generator=gen)
    target = 3.0 + torch.rand(1, H, W, device="cuda", generator=gen)
    ntarget = torch.nn.functional.normalize(torch.randn(3, H, W, device="cuda", generator=gen), dim=0)
    models = []
    for fuse in (False, True):
        g = _model(P, 3, 3, seed=4)
        g.training_setup(OptimizationParams())
        for it in range(3):  # a few steps so the moments are non-trivial
            color, radii, depth, st = fused.forward(g, cam, bg, 0.3, normal=True)
            assert st.normal is not None and st.normal.shape == (3, H, W)
            alpha = fused.accumulated_alpha(st)
            _, _, ws = l1_ssim_forward(color, gt, 0.2)
            dimg = l1_ssim_backward(color, gt, 0.2, ws)
            dl, al, nm = (t.detach().requires_grad_() for t in (depth, alpha, st.normal))
            (0.1 * _depth_loss(dl, al, target) + 0.05 * al.mean() + 0.1 * _normal_loss(nm, ntarget)).backward()
            if fuse:
                fused.backward(st, dimg, None, None, adam=g.optimizer.fused_step(g), dL_ddepth=dl.grad,
                               dL_dalpha=al.grad, dL_dnormal=nm.grad)
            else:
                g.bind_flat_grad()
                fused.backward(st, dimg, {k: v.grad for k, v in _params(g).items()}, None, dL_ddepth=dl.grad,
                               dL_dalpha=al.grad, dL_dnormal=nm.grad)
                g.optimizer.step()
        models.append(g)
    a, b = models
    for k in NAMES:
        x, y = _params(a)[k].detach(), _params(b)[k].detach()
        assert (x - y).abs().max() <= 1e-5 * max(1.0, float(y.abs().max())), (k, float((x - y).abs().max()))
    for pa, pb in zip(a.params(), b.params()):
        sa, sb = a.optimizer.state[pa], b.optimizer.state[pb]
        assert float(sa["step"]) == float(sb["step"]) == 3.0
        for m in ("exp_avg", "exp_avg_sq"):
            x, y = sa[m], sb[m]
            scale = max(float(y.abs().max()), 1e-30)
            assert float((x - y).abs().max()) <= 1e-4 * scale, (m, float((x - y).abs().max()), scale)
            assert _trel(x, y) < 1e-4, (m, _trel(x, y))
