"""Differentiable depth-moment maps (rr_forward_render_dist, rr_backward_aux_dist) on the GPU.

The reference is the existing oracle alone (tests/dist_ref.py, pinned by tests/test_dist_ref_cpu.py):
a render with colours [m_i, 1, m_i^2] over a zero background has M1 in channel 0 and M2 in channel 2,
and the oracle's backward of that run gives the moment term of every gradient.  The colour, depth
and alpha terms are test_depth_grad_gpu.py's (the same scenes and output gradients, computed once
for both files), the normal term is tests/normal_ref.py's.  Bars: the project's parity bar of 1e-4
relative L1 against the oracle, 1e-5 between GPU runs that differ only in the order of their float
atomics.  The early-stop split-2 binning is what catches a phase-B resume that drops M1 / M2."""
import numpy as np
import pytest
import torch

from rain_amd import cameras, fused, synthetic
from rain_amd.gaussian_model import OptimizationParams
from rain_amd.loss import l1_ssim_backward, l1_ssim_forward
from tests.common import GRAD_NAMES, oracle_run, rel_l1
from tests.dist_ref import MAPPINGS, dist_part
from tests.normal_ref import normal_part
# the depth file's scenes, reference, binning fixture (default, and early-stop split 2) and helpers
from tests.test_depth_grad_gpu import (NAMES, SCENES, _depth_loss, _gpu_inputs, _model, _params,  # noqa: F401
                                       _reference, _settings, _trel, binning)

pytestmark = pytest.mark.gpu

_REF = {}


def _dist_reference(oracle, name):
    """Per scene, computed once and left unchanged: the depth file's reference plus, per mapping, the
    expected moment maps and the moment term of every gradient, and the normal term where the
    scene has the scale / rotation pair."""
    if name in _REF:
        return _REF[name]
    ref = dict(_reference(oracle, name))
    inp, st = ref["inp"], ref["st"]
    H, W = st["image_height"], st["image_width"]
    rng = np.random.default_rng(17)
    dm = rng.standard_normal((2, H, W)).astype(np.float32)
    dn = rng.standard_normal((3, H, W)).astype(np.float32)
    z = oracle_run(oracle, inp, st)["state"].internals()["depths"]
    ref["dm"], ref["dn"], ref["z"] = dm, dn, z
    ref["moments"], ref["mparts"] = {}, {}
    for mapping, (near, far) in MAPPINGS.items():
        part, tr = dist_part(oracle, inp, st, z, dm, near, far, like=ref["colour"])
        assert np.array_equal(tr["radii"], ref["radii"])
        ref["mparts"][mapping] = part
        ref["moments"][mapping] = np.stack([tr["color"][0], tr["color"][2]])
    ref["has_normal"] = "scales" in inp
    if ref["has_normal"]:
        npart, _tr = normal_part(oracle, inp, st, dn)
        ref["npart"] = {k: np.asarray(npart[k], np.float64).reshape(ref["colour"][k].shape) for k in GRAD_NAMES}
    _REF[name] = ref
    return ref


def _forward_args(d, s):
    e = torch.Tensor([])
    return (s["bg"], d["means3D"], d.get("colors_precomp", e), d["opacities"], d.get("scales", e), d.get("rotations", e),
            s["scale_modifier"], d.get("cov3D_precomp", e), s["viewmatrix"], s["projmatrix"], s["tanfovx"], s["tanfovy"],
            s["image_height"], s["image_width"], d.get("shs", e), s["sh_degree"], s["campos"], s["prefiltered"],
            s["debug"], s["low_pass"])


def _forward_dist(d, s, near, far, normal=False):
    """(num_rendered, color, radii, depth, normal, moments, geom, binning, img)"""
    from rain_amd.diff_gaussian_rasterization import _C

    return _C.rasterize_gaussians_dist(*_forward_args(d, s), near, far, normal)


def _backward_args(d, s, fw, dpix):
    e = torch.Tensor([])
    nr, _color, radii, _depth, _normal, _mom, geom, binb, img = fw
    return (s["bg"], d["means3D"], radii, d.get("colors_precomp", e), d.get("scales", e), d.get("rotations", e),
            s["scale_modifier"], d.get("cov3D_precomp", e), s["viewmatrix"], s["projmatrix"], s["tanfovx"],
            s["tanfovy"], dpix, d.get("shs", e), s["sh_degree"], s["campos"], geom, nr, binb, img, False,
            s["low_pass"])


@pytest.mark.parametrize("mapping", list(MAPPINGS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_moment_maps(oracle, gpu, binning, scene, mapping):
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    near, far = MAPPINGS[mapping]
    ref = _dist_reference(oracle, scene)
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    H, W = s["image_height"], s["image_width"]
    P = d["means3D"].shape[0]
    plain = _C.rasterize_gaussians(*_forward_args(d, s))
    fw = _forward_dist(d, s, near, far)
    tile_max = _C.debug_views(fw[6], fw[7], fw[8], fw[0], P, W, H)["tile_max"]
    assert int(tile_max.max()) > 64, "the scene must walk more than one 64-pair round"
    with torch.no_grad():
        color, radii, depth, alpha, normal, moments = GaussianRasterizer(_settings(s)).forward_distortion(
            d["means3D"], torch.zeros_like(d["means3D"]), d["opacities"], shs=d.get("shs"),
            colors_precomp=d.get("colors_precomp"), scales=d.get("scales"), rotations=d.get("rotations"),
            cov3D_precomp=d.get("cov3D_precomp"), dist_near=near, dist_far=far)
        _c, _r, depth_ref, alpha_ref = GaussianRasterizer(_settings(s)).forward_depth(
            d["means3D"], torch.zeros_like(d["means3D"]), d["opacities"], shs=d.get("shs"),
            colors_precomp=d.get("colors_precomp"), scales=d.get("scales"), rotations=d.get("rotations"),
            cov3D_precomp=d.get("cov3D_precomp"))
    # colour, radii, depth and alpha bitwise forward_depth's (and the plain forward's)
    assert torch.equal(color, _c) and torch.equal(radii, _r) and torch.equal(depth, depth_ref)
    assert torch.equal(alpha, alpha_ref)
    assert torch.equal(color, plain[1]) and torch.equal(radii, plain[2]) and torch.equal(depth, plain[3])
    assert torch.equal(fw[1], plain[1]) and torch.equal(fw[3], plain[3])
    assert normal is None and fw[4] is None
    assert moments.shape == (2, H, W) and torch.equal(moments, fw[5])
    got = moments.cpu().numpy()
    for i, nm in enumerate(("M1", "M2")):
        e = rel_l1(got[i], ref["moments"][mapping][i])
        print(f"{scene} {mapping}: {nm} rel L1 {e:.3e}")
        assert e <= 1e-4, (nm, e)
    if ref["has_normal"]:  # with the normal map: the same moments, rasterize_gaussians_aux's normal
        fwn = _forward_dist(d, s, near, far, normal=True)
        aux = _C.rasterize_gaussians_aux(*_forward_args(d, s))
        assert torch.equal(fwn[5], fw[5]) and torch.equal(fwn[4], aux[4])
        assert torch.equal(fwn[1], plain[1]) and torch.equal(fwn[3], plain[3])


def _check(label, k, g, want, hidden):
    assert g.shape == want.shape, (label, k)
    if g.size == 0:  # dL_dsh without SH inputs: [P, 0, 3]
        return
    assert np.isfinite(g).all(), (label, k)
    assert np.abs(g[hidden]).sum() == 0.0, (label, k)  # Gaussians the forward did not keep: exact zeros
    if np.abs(want).sum() == 0:
        assert np.abs(g).max() == 0.0, (label, k)
        return
    err = rel_l1(g, want)
    print(f"{label}: {k} rel L1 {err:.3e}")
    assert err <= 1e-4, f"{label} {k}: rel L1 {err:.3e}"


# (colour, depth, alpha, normal, moments): "m" the random moment gradient, "z" a zero map (the moment
# kernels run, the term is zero), so that every output gradient is also checked alone
COMBOS = {
    "moments_only": (0, 0, 0, 0, "m"),
    "colour_alone": (1, 0, 0, 0, "z"),
    "depth_alone": (0, 1, 0, 0, "z"),
    "alpha_alone": (0, 0, 1, 0, "z"),
    "normal_alone": (0, 0, 0, 1, "z"),
    "all_but_normal": (1, 1, 1, 0, "m"),
    "normal+moments": (0, 0, 0, 1, "m"),
    "all": (1, 1, 1, 1, "m"),
}


@pytest.mark.parametrize("mapping", list(MAPPINGS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_gradient_parity(oracle, gpu, binning, scene, mapping):
    from rain_amd.diff_gaussian_rasterization import _C

    near, far = MAPPINGS[mapping]
    ref = _dist_reference(oracle, scene)
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    H, W = s["image_height"], s["image_width"]
    fws = {False: _forward_dist(d, s, near, far)}
    if ref["has_normal"]:
        fws[True] = _forward_dist(d, s, near, far, normal=True)
    assert np.array_equal(fws[False][2].cpu().numpy(), ref["radii"])
    t = {k: torch.from_numpy(ref[k]).to(gpu) for k in ("dpix", "dd", "da", "dn", "dm")}
    e = torch.Tensor([])
    hidden = ref["radii"] == 0
    ran = 0
    for label, (c, dd, da, dn, dm) in COMBOS.items():
        if dn and not ref["has_normal"]:
            continue
        fw = fws[bool(dn)]
        gm = t["dm"] if dm == "m" else torch.zeros((2, H, W), device=gpu)
        got = _C.rasterize_gaussians_backward_dist(*_backward_args(d, s, fw, t["dpix"] if c else e),
                                                   t["dd"] if dd else e, t["da"] if da else e, t["dn"] if dn else e,
                                                   gm, near, far)
        torch.cuda.synchronize()
        for k, g in zip(GRAD_NAMES, got):
            want = np.zeros_like(ref["colour"][k])
            if c:
                want += ref["colour"][k]
            if dd:
                want += ref["parts"]["depth"][k]
            if da:
                want += ref["parts"]["alpha"][k]
            if dn:
                want += ref["npart"][k]
            if dm == "m":
                want += ref["mparts"][mapping][k]
            _check(f"{scene} {mapping} {label}", k, g.cpu().numpy(), want, hidden)
        if label == "moments_only":
            gd = dict(zip(GRAD_NAMES, got))
            assert float(gd["dL_dmeans3D"].abs().sum()) > 0.0 and float(gd["dL_dopacity"].abs().sum()) > 0.0
            assert float(gd["dL_dcolors"].abs().max()) == 0.0
        ran += 1
    assert ran == (8 if ref["has_normal"] else 5)


def test_absent_moment_gradient_is_the_normal_backward(oracle, gpu, binning):
    from rain_amd.diff_gaussian_rasterization import _C

    ref = _dist_reference(oracle, "sh3")
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    H, W = s["image_height"], s["image_width"]
    fw = _forward_dist(d, s, 0.2, 100.0, normal=True)
    dpix, dd, da, dn = (torch.from_numpy(ref[k]).to(gpu) for k in ("dpix", "dd", "da", "dn"))
    args = _backward_args(d, s, fw, dpix)
    normal = _C.rasterize_gaussians_backward_normal(*args, dd, da, dn)
    absent = _C.rasterize_gaussians_backward_dist(*args, dd, da, dn, torch.Tensor([]), 0.2, 100.0)
    zeros = _C.rasterize_gaussians_backward_dist(*args, dd, da, dn, torch.zeros((2, H, W), device=gpu), 0.2, 100.0)
    for k, p, a, b in zip(GRAD_NAMES, normal, absent, zeros):
        assert rel_l1(a.cpu().numpy(), p.cpu().numpy()) <= 1e-5, k
        assert rel_l1(b.cpu().numpy(), p.cpu().numpy()) <= 1e-5, k
    # and without a normal gradient it is the depth backward
    e = torch.Tensor([])
    depth = _C.rasterize_gaussians_backward_depth(*args, dd, da)
    absent = _C.rasterize_gaussians_backward_dist(*args, dd, da, e, e, 0.2, 100.0)
    zeros = _C.rasterize_gaussians_backward_dist(*args, dd, da, e, torch.zeros((2, H, W), device=gpu), 0.0, 0.0)
    for k, p, a, b in zip(GRAD_NAMES, depth, absent, zeros):
        assert rel_l1(a.cpu().numpy(), p.cpu().numpy()) <= 1e-5, k
        assert rel_l1(b.cpu().numpy(), p.cpu().numpy()) <= 1e-5, k


def test_autograd_surface(oracle, gpu):
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    ref = _dist_reference(oracle, "sh3")
    d, s = _gpu_inputs(ref["inp"], ref["st"], gpu)
    H, W = s["image_height"], s["image_width"]
    gen = torch.Generator().manual_seed(21)
    w = torch.randn((3, H, W), generator=gen).to(gpu)
    ntarget = torch.nn.functional.normalize(torch.randn((3, H, W), generator=gen), dim=0).to(gpu)
    leaves = {k: d[k].clone().requires_grad_() for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    means2D = torch.zeros_like(d["means3D"]).requires_grad_()
    r = GaussianRasterizer(_settings(s))
    pairs = (("means3D", "dL_dmeans3D"), ("shs", "dL_dsh"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"),
             ("rotations", "dL_drotations"))

    def run(normal):
        return r.forward_distortion(leaves["means3D"], means2D, leaves["opacities"], shs=leaves["shs"],
                                    scales=leaves["scales"], rotations=leaves["rotations"], dist_near=0.0,
                                    dist_far=0.0, normal=normal)

    def loss_of(color, depth, alpha, normal, moments):
        dist = (alpha * moments[1:2] - moments[0:1] ** 2).mean()
        return dist + 1e-3 * (color * w).sum() + 0.1 * (depth / (alpha + 1e-6)).mean() \
            + (1.0 - (normal * ntarget).sum(0)).mean()

    color, radii, depth, alpha, normal, moments = run(True)
    assert all(t.requires_grad for t in (color, depth, alpha, normal, moments)) and not radii.requires_grad
    loss_of(color, depth, alpha, normal, moments).backward()
    fw = _forward_dist(d, s, 0.0, 0.0, normal=True)
    assert torch.equal(fw[1], color.detach()) and torch.equal(fw[5], moments.detach())
    c, dp, al, nm, mo = (t.detach().clone().requires_grad_() for t in (color, depth, alpha, normal, moments))
    loss_of(c, dp, al, nm, mo).backward()
    byhand = dict(zip(GRAD_NAMES, _C.rasterize_gaussians_backward_dist(
        *_backward_args(d, s, fw, c.grad), dp.grad, al.grad, nm.grad, mo.grad, 0.0, 0.0)))
    for leaf, k in pairs:
        err = rel_l1(leaves[leaf].grad.cpu().numpy(), byhand[k].cpu().numpy())
        assert err <= 1e-5, (leaf, err)
    assert rel_l1(means2D.grad.cpu().numpy(), byhand["dL_dmeans2D"].cpu().numpy()) <= 1e-5

    # a loss on the moments alone, without the normal map: the others arrive as absent gradients
    for t in list(leaves.values()) + [means2D]:
        t.grad = None
    color, radii, depth, alpha, normal, moments = run(False)
    assert normal is None
    wm = torch.randn((2, H, W), generator=gen).to(gpu)
    (moments * wm).sum().backward()
    e = torch.Tensor([])
    fw = _forward_dist(d, s, 0.0, 0.0)
    only = dict(zip(GRAD_NAMES, _C.rasterize_gaussians_backward_dist(*_backward_args(d, s, fw, e), e, e, e, wm, 0.0,
                                                                    0.0)))
    for leaf, k in pairs:
        assert rel_l1(leaves[leaf].grad.cpu().numpy(), only[k].cpu().numpy()) <= 1e-5, leaf
    assert float(only["dL_dsh"].abs().max()) == 0.0 and float(only["dL_dmeans3D"].abs().sum()) > 0.0


def _raw_params(scene, dev):
    """The raw parameters make_scene's inputs are the activations of (tests/common.py)."""
    kw = SCENES[scene]
    p = synthetic.random_gaussians(kw["P"], sh_degree=kw["sh_degree"], seed=0, bench=True)
    return {k: v.float().contiguous().to(dev) for k, v in p.items()}


@pytest.mark.parametrize("mapping", list(MAPPINGS))
@pytest.mark.parametrize("scene", ["sh3", "ragged_bg"])
def test_raw_parameter_backward_against_reference(oracle, gpu, binning, scene, mapping):
    """fused.forward(dist=...) / fused.backward(dL_dmoments=...) without Adam: the six raw-parameter
    gradients against the same oracle reference, chained through the getters in float64."""
    near, far = MAPPINGS[mapping]
    ref = _dist_reference(oracle, scene)
    st = ref["st"]
    H, W = st["image_height"], st["image_width"]
    raw = _raw_params(scene, gpu)
    params = tuple(raw[k] for k in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"))
    t = {k: torch.from_numpy(ref[k]).to(gpu) for k in ("dpix", "dd", "da", "dn", "dm")}
    dev = {k: (v.to(gpu) if isinstance(v, torch.Tensor) else v) for k, v in st.items()}
    for normal in (False, True):
        color, radii, depth, fr = fused.forward_params(
            params, st["sh_degree"], W, H, st["tanfovx"], st["tanfovy"], dev["viewmatrix"], dev["projmatrix"],
            dev["campos"], dev["bg"], st["low_pass"], st["scale_modifier"], normal=normal, dist=(near, far))
        # (the in-kernel getters may round a radius differently from torch's: all but a handful agree)
        assert int((radii.cpu().numpy() != ref["radii"]).sum()) <= len(ref["radii"]) // 500
        assert (fr.normal is not None) == normal and fr.moments.shape == (2, H, W)
        for i in range(2):
            assert rel_l1(fr.moments[i].cpu().numpy(), ref["moments"][mapping][i]) <= 1e-4
        grads = {k: torch.full_like(v, float("nan")) for k, v in raw.items()}
        fused.backward(fr, t["dpix"], grads, dL_ddepth=t["dd"], dL_dalpha=t["da"], dL_dnormal=t["dn"] if normal else None,
                       dL_dmoments=t["dm"])
        torch.cuda.synchronize()
        # the reference's gradients of the activated inputs, chained through the getters in float64
        want = {k: ref["colour"][k] + ref["parts"]["depth"][k] + ref["parts"]["alpha"][k] + ref["mparts"][mapping][k]
                + (ref["npart"][k] if normal else 0.0) for k in GRAD_NAMES}
        r64 = {k: v.double().cpu().requires_grad_() for k, v in raw.items()}
        act = synthetic.activated(r64)
        up = dict(means3D="dL_dmeans3D", scales="dL_dscales", rotations="dL_drotations", opacities="dL_dopacity",
                  shs="dL_dsh")
        total = sum((act[a] * torch.from_numpy(want[g]).reshape(act[a].shape)).sum() for a, g in up.items())
        chained = dict(zip(r64, torch.autograd.grad(total, list(r64.values()))))
        for k in NAMES:
            g = grads[k].cpu().numpy()
            assert np.isfinite(g).all(), k
            want_k = chained[k].numpy()
            den = np.abs(want_k).sum()
            if k == "rotation":
                # these scenes have isotropic scales and unit raw quaternions: the covariance does not
                # depend on the rotation, so F.normalize's backward removes all of dL_drotations but
                # the normal term's part (nothing at all without the normal map).  The reference's
                # dL_drotations is good to the bar relative to ITS size, and the projection
                # (I - q q^T) / |q| with |q| = 1 does not enlarge an error: the bar is relative to it.
                den = max(den, np.abs(want["dL_drotations"]).sum())
            err = float(np.abs(g - want_k).sum() / den)
            print(f"{scene} {mapping} normal={normal}: {k} rel L1 {err:.3e}")
            assert err <= 1e-4, (k, err)


def test_adam_fused_into_dist_backward_matches_separate_step(gpu):
    """test_adam_fused_into_normal_backward_matches_separate_step with a distortion term in the loss:
    the step applied inside rr_backward_aux_dist equals gradients written out + FusedAdam.step()
    (that test's bars).  The two runs differ in the order of the blend backward's float atomics, and
    Adam's g / (sqrt(v) + eps) passes a gradient's RELATIVE error on to the step; a Gaussian whose
    per-pixel terms cancel (white-noise targets give every pixel its own sign) has a sum far smaller
    than its terms and a relative error as much larger, which the bar then catches by chance (one run
    in three with white-noise targets).  The targets here are smooth, so the terms of a footprint
    agree in sign and the comparison is about the fused step, not about that cancellation."""
    P, W, H = 20_000, 160, 120
    cam = cameras.fibonacci_cameras(8, W, H)[2].to("cuda")
    bg = torch.zeros(3, device="cuda")
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device="cuda"), torch.linspace(0, 1, W, device="cuda"),
                            indexing="ij")
    gt = torch.stack([0.2 + 0.6 * xx, 0.8 - 0.5 * yy, 0.3 + 0.4 * xx * yy]).contiguous()
    target = (3.0 + xx + 0.5 * yy)[None].contiguous()
    ntarget = torch.nn.functional.normalize(torch.stack([0.3 * (xx - 0.5), 0.3 * (yy - 0.5), -torch.ones_like(xx)]),
                                            dim=0).contiguous()
    models = []
    for fuse in (False, True):
        g = _model(P, 3, 3, seed=4)
        g.training_setup(OptimizationParams())
        for it in range(3):  # a few steps so the moments are non-trivial
            normal = it != 1  # both moment modes: with and without the normal map
            color, radii, depth, st = fused.forward(g, cam, bg, 0.3, normal=normal, dist=(0.0, 0.0))
            assert st.moments is not None and st.moments.shape == (2, H, W)
            alpha = fused.accumulated_alpha(st)
            _, _, ws = l1_ssim_forward(color, gt, 0.2)
            dimg = l1_ssim_backward(color, gt, 0.2, ws)
            dl, al, mo = (t.detach().requires_grad_() for t in (depth, alpha, st.moments))
            loss = 0.1 * _depth_loss(dl, al, target) + 0.05 * al.mean() + 0.5 * (al * mo[1:2] - mo[0:1] ** 2).mean()
            nm = None
            if normal:
                nm = st.normal.detach().requires_grad_()
                loss = loss + 0.1 * (1.0 - (nm * ntarget).sum(0)).mean()
            loss.backward()
            kw = dict(dL_ddepth=dl.grad, dL_dalpha=al.grad, dL_dnormal=nm.grad if normal else None, dL_dmoments=mo.grad)
            if fuse:
                fused.backward(st, dimg, None, None, adam=g.optimizer.fused_step(g), **kw)
            else:
                g.bind_flat_grad()
                fused.backward(st, dimg, {k: v.grad for k, v in _params(g).items()}, None, **kw)
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


def test_render_dist_grad_routes_agree(gpu, monkeypatch):
    """render(dist_grad=True) on the raw-parameter route and on the getters route, alone and with
    normal_grad: outputs and the six leaf gradients (bars of test_render_depth_grad_routes_agree)."""
    from rain_amd import renderer as renderer_mod
    from rain_amd.renderer import PipelineParams, render

    P, W, H = 30_000, 200, 150
    cam = cameras.fibonacci_cameras(8, W, H)[5].to("cuda")
    bg = torch.tensor([0.3, 0.1, 0.2], device="cuda")
    gen = torch.Generator("cuda").manual_seed(9)
    wcol = torch.randn(3, H, W, device="cuda", generator=gen) / (3 * H * W)
    for with_normal in (False, True):
        outs = []
        for raw in (False, True):
            monkeypatch.setattr(renderer_mod, "RAW_RENDER", raw)
            g = _model(P, 3, 3, seed=4)
            pkg = render(cam, g, PipelineParams(), bg, dist_grad=True, dist_near=0.0, dist_far=0.0,
                         normal_grad=with_normal)
            want = {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha", "depth_moments",
                    "distortion"} | ({"normal"} if with_normal else set())
            assert set(pkg) == want
            assert pkg["render"].grad_fn.__class__.__name__.startswith("RasterizeRawParamsDist") == raw
            assert pkg["depth_moments"].shape == (2, H, W) and pkg["distortion"].shape == (1, H, W)
            assert pkg["depth_moments"].requires_grad and pkg["distortion"].requires_grad
            mo, al = pkg["depth_moments"], pkg["alpha"]
            assert torch.equal(pkg["distortion"], al * mo[1:2] - mo[0:1] * mo[0:1])
            loss = (pkg["render"] * wcol).sum() + pkg["distortion"].mean() + 0.1 * al.mean()
            if with_normal:
                loss = loss + 0.1 * pkg["normal"][2].mean()
            loss.backward()
            outs.append((pkg, {k: v.grad.clone() for k, v in _params(g).items()}))
        (pa, ga), (pb, gb) = outs
        assert torch.equal(pa["radii"], pb["radii"])
        for k in ("render", "depth", "alpha", "depth_moments"):
            assert _trel(pb[k], pa[k]) < 1e-6, k
        for k in NAMES:
            assert torch.isfinite(gb[k]).all(), k
            assert float(ga[k].abs().sum()) > 0.0, k
            assert _trel(gb[k], ga[k]) < 1e-4, (k, _trel(gb[k], ga[k]))
        assert _trel(pb["viewspace_points"].grad, pa["viewspace_points"].grad) < 1e-4
    plain = render(cam, g, PipelineParams(), bg)
    assert "depth_moments" not in plain and "alpha" not in plain and not plain["depth"].requires_grad
