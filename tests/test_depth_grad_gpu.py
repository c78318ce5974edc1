"""Differentiable depth and accumulated-alpha outputs (rr_backward_aux, rr_render_alpha) on the GPU.

The reference is the existing oracle alone (tests/depth_ref.py, pinned by tests/test_depth_ref_cpu.py):
a render with colours [z_i, 1, 0] over a zero background has the depth map in channel 0 and the
accumulated alpha in channel 1, so the oracle's backward of that run gives the depth and alpha
gradients.  Bars: the project's parity bar of 1e-4 relative L1 against the oracle, 1e-5 between GPU
runs that differ only in the order of their float atomics."""
import numpy as np
import pytest
import torch

from rain_amd import _native as N
from rain_amd import cameras, fused, synthetic
from rain_amd import renderer as renderer_mod
from rain_amd.gaussian_model import GaussianModel, OptimizationParams
from rain_amd.loss import l1_ssim_backward, l1_ssim_forward
from rain_amd.renderer import PipelineParams, render
from tests.common import GRAD_NAMES, make_scene, oracle_run, rel_l1
from tests.depth_ref import GEOMETRIC, trick_scene

pytestmark = pytest.mark.gpu

SCENES = {
    "sh3": dict(P=3000, W=128, H=96, sh_degree=3),                                  # several 64-pair rounds, odd tails
    "ragged_bg": dict(P=2000, W=100, H=75, sh_degree=1, bg=(1.0, 0.5, 0.25)),       # ragged tiles, background in tfbg
    "low_pass_300": dict(P=800, W=160, H=120, sh_degree=3, low_pass=300.0),         # wide splats
    "precomp": dict(P=1500, W=96, H=80, sh_degree=3, precomp_colors=True, precomp_cov=True),
}
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


@pytest.fixture(params=[0, 2], ids=["default_binning", "early_stop_split2"])
def binning(request):
    if request.param:
        N.check(N.raster().rr_set_binning_config(request.param, 1), "binning config")
    yield request.param
    N.check(N.raster().rr_set_binning_config(0, 0), "binning config")


_REF = {}


def _reference(oracle, name):
    """Per scene, computed once and left unchanged: the inputs, random output gradients, and the
    oracle's colour-run gradients, depth-only and alpha-only contributions (the backward is linear
    in the output gradients, so every combination is a sum of these)."""
    if name in _REF:
        return _REF[name]
    inp, st = make_scene(**SCENES[name])
    H, W = st["image_height"], st["image_width"]
    rng = np.random.default_rng(11)
    dpix = rng.standard_normal((3, H, W)).astype(np.float32)
    dd = rng.standard_normal((1, H, W)).astype(np.float32)
    da = rng.standard_normal((1, H, W)).astype(np.float32)
    col = oracle_run(oracle, inp, st, dL_dpix=dpix)
    internals = col["state"].internals()
    inp2, st2 = trick_scene(inp, st, internals["depths"])
    zrow = np.asarray(st["viewmatrix"], np.float64).reshape(4, 4)[:3, 2]
    zero = {k: np.zeros_like(np.asarray(col["grads"][k], np.float64)) for k in GRAD_NAMES}
    parts = {}
    for key, ch, m in (("depth", 0, dd), ("alpha", 1, da)):
        dtrick = np.zeros((3, H, W), np.float32)
        dtrick[ch] = m[0]
        tr = oracle_run(oracle, inp2, st2, dL_dpix=dtrick)["grads"]
        part = {k: v.copy() for k, v in zero.items()}
        for k in GEOMETRIC:
            part[k] += tr[k]
        part["dL_dmeans3D"] += np.asarray(tr["dL_dcolors"], np.float64)[:, 0:1] * zrow
        parts[key] = part
    _REF[name] = dict(inp=inp, st=st, dpix=dpix, dd=dd, da=da, radii=col["radii"], depth=col["depth"],
                      final_T=internals["final_T"], colour={k: np.asarray(col["grads"][k], np.float64)
                                                            for k in GRAD_NAMES}, parts=parts)
    return _REF[name]


def _gpu_inputs(inp, st, dev):
    d = {k: v.to(dev) for k, v in inp.items()}
    s = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in st.items()}
    return d, s


def _forward(d, s):
    from rain_amd.diff_gaussian_rasterization import _C

    e = torch.Tensor([])
    return _C.rasterize_gaussians(
        s["bg"], d["means3D"], d.get("colors_precomp", e), d["opacities"], d.get("scales", e), d.get("rotations", e),
        s["scale_modifier"], d.get("cov3D_precomp", e), s["viewmatrix"], s["projmatrix"], s["tanfovx"], s["tanfovy"],
        s["image_height"], s["image_width"], d.get("shs", e), s["sh_degree"], s["campos"], s["prefiltered"],
        s["debug"], s["low_pass"])


def _backward_args(d, s, fw, dpix):
    e = torch.Tensor([])
    nr, _color, radii, _depth, geom, binb, img = fw
    return (s["bg"], d["means3D"], radii, d.get("colors_precomp", e), d.get("scales", e), d.get("rotations", e),
            s["scale_modifier"], d.get("cov3D_precomp", e), s["viewmatrix"], s["projmatrix"], s["tanfovx"],
            s["tanfovy"], dpix, d.get("shs", e), s["sh_degree"], s["campos"], geom, nr, binb, img, False,
            s["low_pass"])


def _settings(s):
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizationSettings

    return GaussianRasterizationSettings(**{k: s[k] for k in GaussianRasterizationSettings._fields})


def _assert_multi_round(fw, P, W, H):
    from rain_amd.diff_gaussian_rasterization import _C

    nr, _c, _r, _d, geom, binb, img = fw
    tile_max = _C.debug_views(geom, binb, img, nr, P, W, H)["tile_max"]
    assert int(tile_max.max()) > 64, "the scene must walk more than one 64-pair round"


@pytest.mark.parametrize("scene", list(SCENES))
def test_alpha_map(oracle, gpu, binning, scene):
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    ref = _reference(oracle, scene)
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    H, W = s["image_height"], s["image_width"]
    fw = _forward(d, s)
    _assert_multi_round(fw, d["means3D"].shape[0], W, H)
    with torch.no_grad():
        color, radii, depth, alpha = GaussianRasterizer(_settings(s)).forward_depth(
            d["means3D"], torch.zeros_like(d["means3D"]), d["opacities"], shs=d.get("shs"),
            colors_precomp=d.get("colors_precomp"), scales=d.get("scales"), rotations=d.get("rotations"),
            cov3D_precomp=d.get("cov3D_precomp"))
    assert torch.equal(color, fw[1]) and torch.equal(radii, fw[2]) and torch.equal(depth, fw[3])
    assert alpha.shape == (1, H, W)
    assert torch.equal(alpha, _C.accumulated_alpha(fw[6], H, W))
    a = alpha.cpu().numpy()[0]
    assert a.min() >= 0.0 and a.max() <= 1.0
    e = rel_l1(a, 1.0 - ref["final_T"])
    print(f"{scene}: alpha map rel L1 {e:.3e}")
    assert e <= 1e-4


@pytest.mark.parametrize("scene", list(SCENES))
def test_gradient_parity(oracle, gpu, binning, scene):
    from rain_amd.diff_gaussian_rasterization import _C

    ref = _reference(oracle, scene)
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    fw = _forward(d, s)
    _assert_multi_round(fw, d["means3D"].shape[0], s["image_width"], s["image_height"])
    assert np.array_equal(fw[2].cpu().numpy(), ref["radii"])
    dpix = torch.from_numpy(ref["dpix"]).to(gpu)
    dd, da = torch.from_numpy(ref["dd"]).to(gpu), torch.from_numpy(ref["da"]).to(gpu)
    e = torch.Tensor([])
    hidden = ref["radii"] == 0  # (80, 31, 0 and 6 Gaussians of the four scenes)
    for label, gd, ga in (("both", dd, da), ("depth_only", dd, e), ("alpha_only", e, da)):
        got = _C.rasterize_gaussians_backward_depth(*_backward_args(d, s, fw, dpix), gd, ga)
        torch.cuda.synchronize()
        for k, g in zip(GRAD_NAMES, got):
            want = ref["colour"][k].copy()
            if gd.numel():
                want += ref["parts"]["depth"][k]
            if ga.numel():
                want += ref["parts"]["alpha"][k]
            g = g.cpu().numpy()
            assert g.shape == want.shape, (label, k)
            if g.size == 0:  # dL_dsh without SH inputs: [P, 0, 3]
                continue
            assert np.isfinite(g).all(), (label, k)
            assert np.abs(g[hidden]).sum() == 0.0, (label, k)  # Gaussians the forward did not keep: exact zeros
            if np.abs(want).sum() == 0:  # (dL_dsh / dL_dscales / dL_drotations with precomputed inputs)
                assert np.abs(g).max() == 0.0, (label, k)
                continue
            err = rel_l1(g, want)
            print(f"{scene} {label}: {k} rel L1 {err:.3e}")
            assert err <= 1e-4, f"{label} {k}: rel L1 {err:.3e}"


def test_absent_or_zero_maps_change_nothing(oracle, gpu, binning):
    from rain_amd.diff_gaussian_rasterization import _C

    ref = _reference(oracle, "sh3")
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    H, W = s["image_height"], s["image_width"]
    fw = _forward(d, s)
    dpix = torch.from_numpy(ref["dpix"]).to(gpu)
    args = _backward_args(d, s, fw, dpix)
    plain = _C.rasterize_gaussians_backward(*args)
    e = torch.Tensor([])
    absent = _C.rasterize_gaussians_backward_depth(*args, e, e)
    z = torch.zeros((1, H, W), device=gpu)
    zeros = _C.rasterize_gaussians_backward_depth(*args, z, z)
    for k, p, a, b in zip(GRAD_NAMES, plain, absent, zeros):
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
    leaves = {k: d[k].clone().requires_grad_() for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    means2D = torch.zeros_like(d["means3D"]).requires_grad_()
    r = GaussianRasterizer(_settings(s))

    def loss_of(color, depth, alpha):
        return (depth / (alpha + 1e-6) - target).abs().mean() + (color * w).sum()

    color, radii, depth, alpha = r.forward_depth(leaves["means3D"], means2D, leaves["opacities"], shs=leaves["shs"],
                                                 scales=leaves["scales"], rotations=leaves["rotations"])
    assert depth.requires_grad and alpha.requires_grad and color.requires_grad and not radii.requires_grad
    loss_of(color, depth, alpha).backward()
    # the same output gradients fed to _C by hand
    fw = _forward(d, s)
    assert torch.equal(fw[1], color.detach()) and torch.equal(fw[3], depth.detach())
    c, dp, al = (t.detach().clone().requires_grad_() for t in (color, depth, alpha))
    loss_of(c, dp, al).backward()
    byhand = dict(zip(GRAD_NAMES, _C.rasterize_gaussians_backward_depth(*_backward_args(d, s, fw, c.grad), dp.grad,
                                                                       al.grad)))
    pairs = (("means3D", "dL_dmeans3D"), ("shs", "dL_dsh"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"),
             ("rotations", "dL_drotations"))
    for leaf, k in pairs:
        err = rel_l1(leaves[leaf].grad.cpu().numpy(), byhand[k].cpu().numpy())
        assert err <= 1e-5, (leaf, err)
    assert rel_l1(means2D.grad.cpu().numpy(), byhand["dL_dmeans2D"].cpu().numpy()) <= 1e-5

    # a loss on depth alone: colour and alpha arrive as absent gradients (no zero maps)
    for t in list(leaves.values()) + [means2D]:
        t.grad = None
    color, radii, depth, alpha = r.forward_depth(leaves["means3D"], means2D, leaves["opacities"], shs=leaves["shs"],
                                                 scales=leaves["scales"], rotations=leaves["rotations"])
    (depth * target).sum().backward()
    e = torch.Tensor([])
    only = dict(zip(GRAD_NAMES, _C.rasterize_gaussians_backward_depth(*_backward_args(d, s, fw, e), target, e)))
    for leaf, k in pairs:
        assert rel_l1(leaves[leaf].grad.cpu().numpy(), only[k].cpu().numpy()) <= 1e-5, leaf
    assert float(only["dL_dsh"].abs().max()) == 0.0 and float(only["dL_dcolors"].abs().max()) == 0.0
    assert float(only["dL_dmeans3D"].abs().sum()) > 0.0

    # forward() is unchanged: its depth gives the inputs no gradient.  (As in the reference, the
    # autograd function does not mark depth non-differentiable, so the tensor's requires_grad flag is
    # set; the gradient that arrives is dropped and every leaf receives exact zeros.)
    for t in list(leaves.values()) + [means2D]:
        t.grad = None
    out = r(leaves["means3D"], means2D, leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
            rotations=leaves["rotations"])
    assert len(out) == 3 and out[0].requires_grad
    assert torch.equal(out[2], depth.detach())
    (out[2] * target).sum().backward()
    for t in list(leaves.values()) + [means2D]:
        assert t.grad is None or float(t.grad.abs().max()) == 0.0


def _model(P, sh_degree, active, seed=0, dev="cuda"):
    g = GaussianModel(sh_degree, divide_ratio=0.8, device=dev)
    p = synthetic.random_gaussians(P, sh_degree=sh_degree, seed=seed, bench=True)
    p["rotation"] = p["rotation"] * 1.7  # unnormalised raw quaternions exercise F.normalize's backward
    p["scaling"] = p["scaling"] + 0.4 * torch.randn(p["scaling"].shape, generator=torch.Generator().manual_seed(seed))
    g.set_params(p)
    g.active_sh_degree = active
    g.spatial_lr_scale = 4.4
    return g


def _params(g):
    return dict(zip(NAMES, (g._xyz, g._features_dc, g._features_rest, g._opacity, g._scaling, g._rotation)))


def _trel(a, b):
    a, b = a.detach().double(), b.detach().double()
    den = float(b.abs().sum())
    return float((a - b).abs().sum()) / den if den else float(a.abs().sum())


def _depth_loss(depth, alpha, target):
    return (depth / (alpha + 1e-6) - target).abs().mean()


def test_render_depth_grad_routes_agree(gpu, monkeypatch):
    """render(depth_grad=True) on the raw-parameter route and on the getters route: outputs, the six
    leaf gradients and viewspace_points.grad (bars of test_render_raw_fast_path_matches_getters_route)."""
    P, W, H = 30_000, 200, 150
    cam = cameras.fibonacci_cameras(8, W, H)[5].to("cuda")
    bg = torch.tensor([0.3, 0.1, 0.2], device="cuda")
    gen = torch.Generator("cuda").manual_seed(9)
    wcol = torch.randn(3, H, W, device="cuda", generator=gen) / (3 * H * W)
    target = 3.0 + torch.rand(1, H, W, device="cuda", generator=gen)
    outs = []
    for raw in (False, True):
        monkeypatch.setattr(renderer_mod, "RAW_RENDER", raw)
        g = _model(P, 3, 3, seed=4)
        pkg = render(cam, g, PipelineParams(), bg, depth_grad=True)
        assert set(pkg) == {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha"}
        assert pkg["render"].grad_fn.__class__.__name__.startswith("RasterizeRawParamsDepth") == raw
        assert pkg["depth"].requires_grad and pkg["alpha"].requires_grad
        loss = (pkg["render"] * wcol).sum() + _depth_loss(pkg["depth"], pkg["alpha"], target) \
            + 0.1 * pkg["alpha"].mean()
        loss.backward()
        outs.append((pkg, {k: v.grad.clone() for k, v in _params(g).items()}))
    (pa, ga), (pb, gb) = outs
    assert torch.equal(pa["radii"], pb["radii"])
    for k in ("render", "depth", "alpha"):
        assert _trel(pb[k], pa[k]) < 1e-6, k
    for k in NAMES:
        assert torch.isfinite(gb[k]).all(), k
        assert float(ga[k].abs().sum()) > 0.0, k
        assert _trel(gb[k], ga[k]) < 1e-4, (k, _trel(gb[k], ga[k]))
    va, vb = pa["viewspace_points"].grad, pb["viewspace_points"].grad
    assert vb.shape == va.shape == (P, 3) and float(vb[:, 2].abs().max()) == 0.0
    assert _trel(vb, va) < 1e-4
    # the default call is unchanged: no alpha, a depth without gradient
    plain = render(cam, g, PipelineParams(), bg)
    assert "alpha" not in plain and not plain["depth"].requires_grad


def test_adam_fused_into_depth_backward_matches_separate_step(gpu):
    """test_adam_fused_into_backward_matches_separate_step with a depth and an alpha term in the loss:
    the step applied inside rr_backward_aux equals gradients written out + FusedAdam.step()."""
    P, W, H = 20_000, 160, 120
    cam = cameras.fibonacci_cameras(8, W, H)[2].to("cuda")
    bg = torch.zeros(3, device="cuda")
    gen = torch.Generator("cuda").manual_seed(9)
    gt = torch.rand(3, H, W, device="cuda", generator=gen)
    target = 3.0 + torch.rand(1, H, W, device="cuda", generator=gen)
    models = []
    for fuse in (False, True):
        g = _model(P, 3, 3, seed=4)
        g.training_setup(OptimizationParams())
        for it in range(3):  # a few steps so the moments are non-trivial
            color, radii, depth, st = fused.forward(g, cam, bg, 0.3)
            alpha = fused.accumulated_alpha(st)
            _, _, ws = l1_ssim_forward(color, gt, 0.2)
            dimg = l1_ssim_backward(color, gt, 0.2, ws)
            dl, al = depth.detach().requires_grad_(), alpha.detach().requires_grad_()
            (0.1 * _depth_loss(dl, al, target) + 0.05 * al.mean()).backward()
            if fuse:
                fused.backward(st, dimg, None, None, adam=g.optimizer.fused_step(g), dL_ddepth=dl.grad,
                               dL_dalpha=al.grad)
            else:
                g.bind_flat_grad()
                fused.backward(st, dimg, {k: v.grad for k, v in _params(g).items()}, None, dL_ddepth=dl.grad,
                               dL_dalpha=al.grad)
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
