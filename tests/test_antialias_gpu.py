"""Anti-aliased rendering (RR_FLAG_ANTIALIAS: the opacity compensation of the 2D dilation) on the GPU.

The reference is tests/antialias_ref.py (pinned by tests/test_antialias_ref_cpu.py): the oracle's plain run
of the scene with opacities float32(o comp), its dL_dopacity scaled by comp, and the factor's own float64
graph added to every other gradient.  Bars: the project's parity bar of 1e-4 relative L1 against the oracle
and between the two GPU routes that differ in the factor's rounding, 1e-5 between GPU runs that differ only
in the order of their float atomics, and test_fused_gpu.py's own bars for the tests mirrored from there."""
import numpy as np
import pytest
import torch

from rain_amd import _native as N
from rain_amd import cameras, fused, synthetic
from rain_amd import renderer as renderer_mod
from rain_amd.gaussian_model import GaussianModel, OptimizationParams
from rain_amd.loss import fused_l1_ssim_loss, l1_ssim_backward, l1_ssim_forward
from rain_amd.renderer import PipelineParams, render
from rain_amd.train import TrainConfig, Trainer
from tests import antialias_ref as AR
from tests.common import GRAD_NAMES, oracle_run, rel_l1
from tests.depth_ref import GEOMETRIC, trick_scene

pytestmark = pytest.mark.gpu
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ALL = list(AR.SCENES) + list(AR.THIN)


@pytest.fixture(params=[0, 2], ids=["default_binning", "early_stop_split2"])
def binning(request):
    if request.param:
        N.check(N.raster().rr_set_binning_config(request.param, 1), "binning config")
    yield request.param
    N.check(N.raster().rr_set_binning_config(0, 0), "binning config")


_REF = {}


def _reference(oracle, name):
    """Per scene, computed once and left unchanged: inputs, a random colour gradient and the reference."""
    if name not in _REF:
        inp, st = AR.scene(name)
        H, W = st["image_height"], st["image_width"]
        dpix = np.random.default_rng(11).standard_normal((3, H, W)).astype(np.float32)
        _REF[name] = dict(inp=inp, st=st, dpix=dpix, ref=AR.reference(oracle, inp, st, dpix))
    return _REF[name]


def _gpu_inputs(inp, st, dev):
    d = {k: v.to(dev) for k, v in inp.items()}
    s = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in st.items()}
    return d, s


def _forward_args(d, s):
    e = torch.Tensor([])
    return (s["bg"], d["means3D"], d.get("colors_precomp", e), d["opacities"], d.get("scales", e), d.get("rotations", e),
            s["scale_modifier"], d.get("cov3D_precomp", e), s["viewmatrix"], s["projmatrix"], s["tanfovx"], s["tanfovy"],
            s["image_height"], s["image_width"], d.get("shs", e), s["sh_degree"], s["campos"], s["prefiltered"],
            s["debug"], s["low_pass"])


def _forward(d, s, antialiasing):
    """(num_rendered, color, radii, depth, geom, binning, img)"""
    from rain_amd.diff_gaussian_rasterization import _C

    with _C.antialiased(antialiasing):
        return _C.rasterize_gaussians(*_forward_args(d, s))


def _backward_args(d, s, fw, dpix):
    e = torch.Tensor([])
    nr, radii, geom, binb, img = fw[0], fw[2], fw[-3], fw[-2], fw[-1]
    return (s["bg"], d["means3D"], radii, d.get("colors_precomp", e), d.get("scales", e), d.get("rotations", e),
            s["scale_modifier"], d.get("cov3D_precomp", e), s["viewmatrix"], s["projmatrix"], s["tanfovx"],
            s["tanfovy"], dpix, d.get("shs", e), s["sh_degree"], s["campos"], geom, nr, binb, img, False,
            s["low_pass"])


def _settings(s):
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizationSettings

    return GaussianRasterizationSettings(**{k: s[k] for k in GaussianRasterizationSettings._fields})


def _alpha(fw, s):
    from rain_amd.diff_gaussian_rasterization import _C

    return _C.accumulated_alpha(fw[-1], s["image_height"], s["image_width"]).cpu().numpy()


def _check_grads(label, got, want, exact_zero):
    """got: the 8 GPU tensors; want: {name: float64 array}; exact_zero: rows that must be all-zero."""
    for k, g in zip(GRAD_NAMES, got):
        g, w = g.cpu().numpy(), want[k]
        assert g.shape == w.shape, (label, k)
        if g.size == 0:  # dL_dsh without SH inputs: [P, 0, 3]
            continue
        assert np.isfinite(g).all(), (label, k)
        assert np.abs(g[exact_zero]).sum() == 0.0, (label, k)
        if np.abs(w).sum() == 0:  # (dL_dsh / dL_dscales / dL_drotations with precomputed inputs)
            assert np.abs(g).max() == 0.0, (label, k)
            continue
        err = rel_l1(g, w)
        print(f"{label}: {k} rel L1 {err:.3e}")
        assert err <= 1e-4, f"{label} {k}: rel L1 {err:.3e}"


# ---- 1. forward ----

@pytest.mark.parametrize("scene", ALL)
def test_forward_equals_precompensated_plain_render(oracle, gpu, binning, scene):
    t = _reference(oracle, scene)
    ref = t["ref"]
    d, s = _gpu_inputs(t["inp"], t["st"], gpu)
    dc, _ = _gpu_inputs(ref["inp_comp"], t["st"], gpu)
    aa = _forward(d, s, True)
    pre = _forward(dc, s, False)
    plain = _forward(d, s, False)
    assert torch.equal(aa[2], pre[2]) and torch.equal(aa[2], plain[2])  # radii: the geometry is untouched
    assert np.array_equal(aa[2].cpu().numpy(), ref["radii"])
    assert aa[0] == plain[0] == ref["num_rendered"]
    from rain_amd.diff_gaussian_rasterization import _C

    W, H, P = s["image_width"], s["image_height"], d["means3D"].shape[0]
    pairs = [_C.frame_stats(f[-3], f[-1], P, W, H)["num_pairs"] for f in (aa, plain)]
    assert pairs[0] <= pairs[1]  # the pair count can only shrink
    final_T = ref["state"].internals()["final_T"]
    for name, a, b, o in (("color", aa[1], pre[1], ref["color"]), ("depth", aa[3], pre[3], ref["depth"]),
                          ("alpha", _alpha(aa, s), _alpha(pre, s), 1.0 - final_T)):
        a, b = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (a, b))
        ea, eo, eb = rel_l1(a, b), rel_l1(a, o), rel_l1(b, o)
        print(f"{scene}: {name} vs pre-compensated {ea:.3e}, vs oracle {eo:.3e} (pre-compensated vs oracle {eb:.3e})")
        assert ea <= 1e-4 and eo <= 1e-4 and eb <= 1e-4, name
    if scene in AR.SMALL:  # and the flag does something: the plain image is far away
        assert rel_l1(plain[1].cpu().numpy(), ref["color"]) > 1e-2
    low = AR.below_visibility(scene, t["inp"]) & (ref["radii"] > 0) & (ref["rho"] <= AR.RHO_MIN)
    if scene in AR.THIN:  # o comp < 1/255: the radius is kept, no pair is emitted
        assert low.sum() >= 3
        tiles = _geometry_arrays(aa[-3], aa[2], P)[1].view(torch.int32).view(P, 2).cpu().numpy()  # {pairs, rect tiles}
        assert (aa[2].cpu().numpy()[low] > 0).all() and (tiles[low, 1] > 0).all()
        assert (tiles[low, 0] == 0).all()
        assert (tiles[(ref["radii"] > 0) & ~low, 0] > 0).mean() > 0.5


# ---- 2. gradients ----

@pytest.mark.parametrize("scene", ALL)
def test_gradient_parity(oracle, gpu, binning, scene):
    from rain_amd.diff_gaussian_rasterization import _C

    t = _reference(oracle, scene)
    ref = t["ref"]
    d, s = _gpu_inputs(t["inp"], t["st"], gpu)
    fw = _forward(d, s, True)
    tile_max = _C.debug_views(fw[-3], fw[-2], fw[-1], fw[0], d["means3D"].shape[0], s["image_width"],
                              s["image_height"])["tile_max"]
    assert int(tile_max.max()) > 64, "the scene must walk more than one 64-pair round"
    with _C.antialiased():
        got = _C.rasterize_gaussians_backward(*_backward_args(d, s, fw, torch.from_numpy(t["dpix"]).to(gpu)))
    torch.cuda.synchronize()
    hidden = ref["radii"] == 0
    low = AR.below_visibility(scene, t["inp"]) & (ref["rho"] <= AR.RHO_MIN)
    _check_grads(scene, got, ref["grads"], hidden | low)
    # the factor's term is a large part of what is compared: without it the bar is missed by far
    base = oracle_run(oracle, ref["inp_comp"], t["st"], dL_dpix=t["dpix"])["grads"]
    if scene in AR.SMALL:
        assert rel_l1(np.asarray(base["dL_dcov3D"], np.float64), ref["grads"]["dL_dcov3D"]) > 1e-2


def test_gradient_parity_depth_alpha(oracle, gpu, binning):
    """small_sh3 with depth and alpha gradients (rasterize_gaussians_backward_depth): the reference comes by
    the trick-scene route (tests/depth_ref.py) on the pre-compensated scene, plus the factor's term with g_o
    taken from the trick runs."""
    from rain_amd.diff_gaussian_rasterization import _C

    t = _reference(oracle, "small_sh3")
    ref, inp, st = t["ref"], t["inp"], t["st"]
    H, W = st["image_height"], st["image_width"]
    if "depth_parts" not in t:
        rng = np.random.default_rng(12)
        dd = rng.standard_normal((1, H, W)).astype(np.float32)
        da = rng.standard_normal((1, H, W)).astype(np.float32)
        inp2, st2 = trick_scene(ref["inp_comp"], st, ref["state"].internals()["depths"])
        zrow = np.asarray(st["viewmatrix"], np.float64).reshape(4, 4)[:3, 2]
        parts = {}
        for key, ch, m in (("depth", 0, dd), ("alpha", 1, da)):
            dtrick = np.zeros((3, H, W), np.float32)
            dtrick[ch] = m[0]
            tr = oracle_run(oracle, inp2, st2, dL_dpix=dtrick)["grads"]
            part = {k: np.zeros_like(ref["grads"][k]) for k in GRAD_NAMES}
            for k in GEOMETRIC:
                part[k] += tr[k]
            part["dL_dmeans3D"] += np.asarray(tr["dL_dcolors"], np.float64)[:, 0:1] * zrow
            parts[key] = AR.finish(ref, inp, st, ref["inp_comp"], ref["comp"], base=part)["grads"]
        t["depth_parts"] = (dd, da, parts)
    dd, da, parts = t["depth_parts"]
    d, s = _gpu_inputs(inp, st, gpu)
    fw = _forward(d, s, True)
    dpix = torch.from_numpy(t["dpix"]).to(gpu)
    gd, ga = torch.from_numpy(dd).to(gpu), torch.from_numpy(da).to(gpu)
    e = torch.Tensor([])
    hidden = ref["radii"] == 0
    for label, md, ma in (("both", gd, ga), ("depth_only", gd, e), ("alpha_only", e, ga)):
        with _C.antialiased():
            got = _C.rasterize_gaussians_backward_depth(*_backward_args(d, s, fw, dpix), md, ma)
        torch.cuda.synchronize()
        want = {k: ref["grads"][k] + (parts["depth"][k] if md.numel() else 0) + (parts["alpha"][k] if ma.numel() else 0)
                for k in GRAD_NAMES}
        _check_grads(f"small_sh3 {label}", got, want, hidden)


# ---- 3. normal and distortion variants ----

@pytest.mark.parametrize("mode", ["normal", "moments", "normal+moments"])
def test_normal_and_distortion_variants_add_up(oracle, gpu, binning, mode):
    """The backward is linear in the output gradients: the anti-aliased backward with colour and normal /
    moment gradients is (a) its colour-only backward plus (b) the plain normal / moment-only backward of the
    pre-compensated scene with dL_dopacity scaled by comp plus (c) the factor's term for (b)'s g_o."""
    from rain_amd.diff_gaussian_rasterization import _C

    t = _reference(oracle, "small_sh3")
    ref, inp, st = t["ref"], t["inp"], t["st"]
    H, W = st["image_height"], st["image_width"]
    d, s = _gpu_inputs(inp, st, gpu)
    dc, _ = _gpu_inputs(ref["inp_comp"], st, gpu)
    near, far = 0.2, 100.0
    rng = np.random.default_rng(13)
    e = torch.Tensor([])
    dn = torch.from_numpy(rng.standard_normal((3, H, W)).astype(np.float32)).to(gpu) if "normal" in mode else e
    dm = torch.from_numpy(rng.standard_normal((2, H, W)).astype(np.float32)).to(gpu) if "moments" in mode else e
    dpix = torch.from_numpy(t["dpix"]).to(gpu)
    with _C.antialiased():
        fw = _C.rasterize_gaussians_dist(*_forward_args(d, s), near, far, True)
        full = _C.rasterize_gaussians_backward_dist(*_backward_args(d, s, fw, dpix), e, e, dn, dm, near, far)
        colour = _C.rasterize_gaussians_backward(*_backward_args(d, s, fw, dpix))
    fwc = _C.rasterize_gaussians_dist(*_forward_args(dc, s), near, far, True)
    assert rel_l1(fw[4].cpu().numpy(), fwc[4].cpu().numpy()) <= 1e-4  # the maps agree
    assert rel_l1(fw[5].cpu().numpy(), fwc[5].cpu().numpy()) <= 1e-4
    only = _C.rasterize_gaussians_backward_dist(*_backward_args(dc, s, fwc, e), e, e, dn, dm, near, far)
    torch.cuda.synchronize()
    only = {k: v.cpu().numpy().astype(np.float64) for k, v in zip(GRAD_NAMES, only)}
    g_o = only["dL_dopacity"].reshape(-1)
    assert np.count_nonzero(g_o) > 1000
    want = {k: v.cpu().numpy().astype(np.float64) + only[k] for k, v in zip(GRAD_NAMES, colour)}
    want["dL_dopacity"] = want["dL_dopacity"] - only["dL_dopacity"] + (g_o * ref["comp"]).reshape(-1, 1)
    for k, v in AR.comp_term(st, inp, g_o).items():
        want[k] = want[k] + v.reshape(want[k].shape)
    _check_grads(f"small_sh3 {mode}", full, want, ref["radii"] == 0)


# ---- 4. off is untouched ----

def test_off_is_untouched_and_no_dilation_is_neutral(oracle, gpu, binning):
    from rain_amd.diff_gaussian_rasterization import _C

    t = _reference(oracle, "small_sh3")
    d, s = _gpu_inputs(t["inp"], t["st"], gpu)
    dpix = torch.from_numpy(t["dpix"]).to(gpu)
    off = _forward(d, s, False)
    bare = _C.rasterize_gaussians(*_forward_args(d, s))
    assert off[0] == bare[0]
    for a, b in zip(off[1:4], bare[1:4]):
        assert torch.equal(a, b)
    # the gradients: equal to the call without the switch exactly as far as that call equals itself (the blend
    # backward sums with float atomics, whose order may differ from run to run: 1e-5 then)
    with _C.antialiased(False):
        g_off = _C.rasterize_gaussians_backward(*_backward_args(d, s, off, dpix))
    g_bare = _C.rasterize_gaussians_backward(*_backward_args(d, s, bare, dpix))
    g_again = _C.rasterize_gaussians_backward(*_backward_args(d, s, bare, dpix))
    for k, a, b, c in zip(GRAD_NAMES, g_off, g_bare, g_again):
        if torch.equal(b, c):
            assert torch.equal(a, b), k
        assert rel_l1(a.cpu().numpy(), b.cpu().numpy()) <= 1e-5, k
    # low_pass = 0: the factor is 1 up to the rounding of det0 / det
    s0 = dict(s, low_pass=0.0)
    a, b = _forward(d, s0, True), _forward(d, s0, False)
    assert torch.equal(a[2], b[2])
    assert rel_l1(a[1].cpu().numpy(), b[1].cpu().numpy()) <= 1e-6
    with _C.antialiased():
        ga = _C.rasterize_gaussians_backward(*_backward_args(d, s0, a, dpix))
    gb = _C.rasterize_gaussians_backward(*_backward_args(d, s0, b, dpix))
    for k, x, y in zip(GRAD_NAMES, ga, gb):
        assert rel_l1(x.cpu().numpy(), y.cpu().numpy()) <= 1e-5, k


# ---- 5. autograd surface ----

def test_gaussian_rasterizer_autograd(oracle, gpu):
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    t = _reference(oracle, "small_sh3")
    d, s = _gpu_inputs(t["inp"], t["st"], gpu)
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    means2D = torch.zeros_like(d["means3D"], requires_grad=True)
    r = GaussianRasterizer(_settings(s), antialiasing=True)
    color, radii, depth, alpha = r.forward_depth(leaves["means3D"], means2D, leaves["opacities"], shs=leaves["shs"],
                                                 scales=leaves["scales"], rotations=leaves["rotations"])
    fw = _forward(d, s, True)
    assert torch.equal(color, fw[1]) and torch.equal(radii, fw[2]) and torch.equal(depth, fw[3])
    plain = GaussianRasterizer(_settings(s))(d["means3D"], means2D.detach(), d["opacities"], shs=d["shs"],
                                             scales=d["scales"], rotations=d["rotations"])[0]
    assert rel_l1(plain.cpu().numpy(), color.detach().cpu().numpy()) > 1e-2
    dpix = torch.from_numpy(t["dpix"]).to(gpu)
    (color * dpix).sum().backward()
    assert not _C.antialiasing_on()
    pairs = (("means3D", "dL_dmeans3D"), ("opacities", "dL_dopacity"), ("shs", "dL_dsh"), ("scales", "dL_dscales"),
             ("rotations", "dL_drotations"))
    for leaf, k in pairs:  # test_gradient_parity's gradients, through autograd
        err = rel_l1(leaves[leaf].grad.cpu().numpy(), t["ref"]["grads"][k])
        assert err <= 1e-4, (leaf, err)
    assert rel_l1(means2D.grad.cpu().numpy(), t["ref"]["grads"]["dL_dmeans2D"]) <= 1e-4
    # forward(): the reference's three outputs, the same image
    c3 = r(d["means3D"], means2D.detach(), d["opacities"], shs=d["shs"], scales=d["scales"], rotations=d["rotations"])
    assert len(c3) == 3 and torch.equal(c3[0], fw[1])
    _c, _r, _d, nmap = r.render_depth_normal(d["means3D"], d["opacities"], shs=d["shs"], scales=d["scales"],
                                              rotations=d["rotations"])
    assert torch.equal(_c, fw[1]) and nmap.shape == (3, s["image_height"], s["image_width"])


def _model(P, sh_degree, active, seed=0, dev="cuda", scale_mult=0.1):
    """test_fused_gpu.py's model at the small-splat scenes' scale."""
    g = GaussianModel(sh_degree, divide_ratio=0.8, device=dev)
    p = synthetic.random_gaussians(P, sh_degree=sh_degree, seed=seed, bench=True)
    p["rotation"] = p["rotation"] * 1.7
    p["scaling"] = p["scaling"] + 0.4 * torch.randn(p["scaling"].shape, generator=torch.Generator().manual_seed(seed))
    p["scaling"] = p["scaling"] + float(np.log(scale_mult))
    g.set_params(p)
    g.active_sh_degree = active
    g.spatial_lr_scale = 4.4
    return g


def _params(g):
    return dict(zip(NAMES, (g._xyz, g._features_dc, g._features_rest, g._opacity, g._scaling, g._rotation)))


def _rl(a, b):
    return rel_l1(a.detach().cpu().numpy(), b.detach().cpu().numpy())


@pytest.mark.parametrize("sh_degree,active,low_pass", [(3, 3, 0.3), (3, 2, 30.0)])
def test_render_routes_agree(gpu, monkeypatch, sh_degree, active, low_pass):
    """render(pipe=PipelineParams(antialiasing=True)) through the getters route and through the raw fast path
    (test_fused_gpu.test_render_raw_fast_path_matches_getters_route's bars), and both differ from the plain
    render."""
    P, W, H = 3000, 128, 96
    cam = cameras.fibonacci_cameras(8, W, H)[5].to("cuda")
    bg = torch.tensor([0.3, 0.1, 0.2], device="cuda")
    gt = torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(9))
    pipe = PipelineParams(antialiasing=True)
    outs = []
    for raw in (False, True):
        monkeypatch.setattr(renderer_mod, "RAW_RENDER", raw)
        g = _model(P, sh_degree, active, seed=4, scale_mult=0.1 if low_pass < 1 else 1.0)
        pkg = render(cam, g, pipe, bg, low_pass=low_pass)
        assert (pkg["render"].grad_fn.__class__.__name__.startswith("RasterizeRawParams")) == raw
        loss, _ = fused_l1_ssim_loss(pkg["render"], gt, 0.2)
        loss.backward()
        outs.append((pkg, {k: v.grad.clone() for k, v in _params(g).items()}))
        with torch.no_grad():
            plain = render(cam, g, PipelineParams(), bg, low_pass=low_pass)["render"]
        assert _rl(plain, pkg["render"]) > 1e-3  # (a saturated image at low_pass 30: 3e-3)
    (pa, ga), (pb, gb) = outs
    assert torch.equal(pa["radii"], pb["radii"])
    assert _rl(pb["render"], pa["render"]) < 1e-6
    assert _rl(pb["depth"], pa["depth"]) < 1e-6
    for k in NAMES:
        assert torch.isfinite(gb[k]).all(), k
        assert float(ga[k].abs().sum()) > 0.0, k
        assert _rl(gb[k], ga[k]) < 1e-4, (k, _rl(gb[k], ga[k]))
    assert _rl(pb["viewspace_points"].grad, pa["viewspace_points"].grad) < 1e-4


# ---- 6. fused step ----

def test_adam_fused_into_backward_matches_separate_step(gpu):
    """test_fused_gpu.py's test of the same name with the flag on (its bars)."""
    P, W, H = 3000, 128, 96
    cam = cameras.fibonacci_cameras(8, W, H)[2].to("cuda")
    bg = torch.zeros(3, device="cuda")
    gt = torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(9))
    models = []
    for fuse in (False, True):
        g = _model(P, 3, 3, seed=4)
        g.training_setup(OptimizationParams())
        for it in range(3):
            color, radii, depth, st = fused.forward(g, cam, bg, 0.3, antialiasing=True)
            assert st.frame.flags & N.RR_FLAG_ANTIALIAS
            _, _, ws = l1_ssim_forward(color, gt, 0.2)
            dimg = l1_ssim_backward(color, gt, 0.2, ws)
            if fuse:
                fused.backward(st, dimg, None, None, adam=g.optimizer.fused_step(g))
            else:
                g.bind_flat_grad()
                fused.backward(st, dimg, {k: v.grad for k, v in _params(g).items()}, None)
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
            assert _rl(x, y) < 1e-4, (m, _rl(x, y))


def _geometry_arrays(geom, radii, P):
    import ctypes

    offs = (ctypes.c_size_t * 5)()
    N.check(N.raster().rr_geometry_layout(P, offs), "layout")
    nb = (P + 255) // 256
    sizes = (48 * P, 8 * P, 4 * P, 8 * nb, 4 * nb)
    return [geom[offs[k]:offs[k] + sizes[k]].clone() for k in range(5)] + [radii.clone()]


@pytest.mark.parametrize("this_aa,next_aa", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("sh_degree,active,low_pass,wh", [(3, 3, 0.3, (128, 96)), (1, 1, 30.0, (100, 75))])
def test_next_frame_preprocess_in_backward_equals_preprocess(gpu, sh_degree, active, low_pass, wh, this_aa, next_aa):
    """test_fused_gpu.py's test of the same name with the flag on this frame, on the next one, or on both:
    geometry arrays and radii bit for bit."""
    P = 3000
    W, H = wh
    cams = [c.to("cuda") for c in cameras.fibonacci_cameras(8, W, H)]
    bg = torch.zeros(3, device="cuda")
    gt = torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(9))
    g = _model(P, sh_degree, active, seed=6, scale_mult=0.1 if low_pass < 1 else 1.0)
    g.training_setup(OptimizationParams())
    for it in range(3):
        color, radii, depth, st = fused.forward(g, cams[it], bg, low_pass, antialiasing=this_aa)
        _, _, ws = l1_ssim_forward(color, gt, 0.2)
        dimg = l1_ssim_backward(color, gt, 0.2, ws)
        nxt = fused.prepare_next(g, cams[it + 3], bg, low_pass, antialiasing=next_aa)
        fused.backward(st, dimg, None, None, adam=g.optimizer.fused_step(g), next_frame=nxt)
        got = _geometry_arrays(nxt.geom, nxt.radii, P)
        _c, ref_radii, _d, ref_st = fused.forward(g, cams[it + 3], bg, low_pass, antialiasing=next_aa)
        ref = _geometry_arrays(ref_st.geom, ref_radii, P)
        other = fused.forward(g, cams[it + 3], bg, low_pass, antialiasing=not next_aa)[0]
        assert _rl(other, _c) > 1e-3  # the next frame's own flag decides
        names = ("splats", "tiles", "depth_keys", "block_sums", "block_wide", "radii")
        vis = ref[5] > 0
        assert vis.any()
        for n, x, y in zip(names, got, ref):
            if n == "splats":  # a culled row's record is never written (nor read): visible rows only
                x, y = x.view(P, 48)[vis].view(torch.float32), y.view(P, 48)[vis].view(torch.float32)
            assert torch.equal(x, y), (it, n)
        c2, r2, d2, _st2 = fused.forward_next(nxt, g)
        assert torch.equal(c2, _c) and torch.equal(d2, _d) and torch.equal(r2, ref_radii)


def test_trainer_next_frame_fusion_matches_unfused(gpu):
    """test_fused_gpu.py's test of the same name with PipelineParams(antialiasing=True) (its bars), and the
    run differs from the plain pipeline's."""
    P, W, H, V = 3000, 128, 96, 6
    cams = [c.to("cuda") for c in cameras.fibonacci_cameras(V, W, H)]
    gts = [torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(20 + i))
           for i in range(V)]
    res = []
    for fuse_next, aa in ((False, True), (True, True), (True, False)):
        g = _model(P, 3, 1, seed=2)
        opt = OptimizationParams(densify_from_iter=2, densification_interval=5, opacity_reset_interval=8)
        g.training_setup(opt)
        t = Trainer(g, cams, gts, opt, PipelineParams(antialiasing=aa), cfg=TrainConfig(c2f=True, seed=3),
                    scene_extent=4.4, fused=True)
        t.fuse_next = fuse_next
        its = list(range(995, 1003))  # the SH degree steps up at 1000
        losses = [t.step(it, sync_loss=True).loss for it in its]
        res.append((g, losses))
    (ga, la), (gb, lb), (_gc, lc) = res
    assert ga.active_sh_degree == gb.active_sh_degree == 2
    assert ga.get_xyz.shape == gb.get_xyz.shape
    for x, y in zip(la, lb):
        assert abs(x - y) <= 1e-5 * abs(y)
    assert abs(lc[0] - lb[0]) > 1e-4 * abs(lb[0])
    for k, x in _params(ga).items():
        y = _params(gb)[k]
        assert _rl(x, y) < 1e-5, (k, _rl(x, y))
    assert torch.equal(ga.denom, gb.denom)
    assert torch.equal(ga.max_radii2D, gb.max_radii2D)


# ---- 7. contributions ----

@pytest.mark.parametrize("scene", ["small_sh3", "small_ragged_bg+thin"])
def test_contributions_are_those_of_the_compensated_frame(oracle, gpu, binning, scene):
    """rr_contributions reads the splat records: a flagged frame's statistics are those of the plain frame
    whose opacities are the flagged frame's compensated ones (taken from its records, so that both frames
    hold the same bits: max_w and count are then equal, the sums equal up to their atomics' order)."""
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    t = _reference(oracle, scene)
    ref = t["ref"]
    d, s = _gpu_inputs(t["inp"], t["st"], gpu)
    P, W, H = d["means3D"].shape[0], s["image_width"], s["image_height"]
    fa = _forward(d, s, True)
    o_eff = _C.debug_views(fa[-3], fa[-2], fa[-1], fa[0], P, W, H)["splats"][:, 7]  # the record's opacity
    vis = fa[2] > 0
    want = ref["inp_comp"]["opacities"].to(gpu).view(-1)
    assert _rl(o_eff[vis], want[vis]) <= 1e-6  # float32(o comp) of the reference, up to the factor's rounding
    dc = dict(d, opacities=torch.where(vis, o_eff, want).view(-1, 1).contiguous())
    kw = lambda x: dict(shs=x.get("shs"), scales=x.get("scales"), rotations=x.get("rotations"))  # noqa: E731
    c1, radii, (sw, sgw, mw, cnt) = GaussianRasterizer(_settings(s), antialiasing=True).contributions(
        d["means3D"], d["opacities"], **kw(d))
    c2, radii2, (sw2, sgw2, mw2, cnt2) = GaussianRasterizer(_settings(s)).contributions(
        dc["means3D"], dc["opacities"], **kw(dc))
    assert torch.equal(radii, radii2) and torch.equal(c1, c2) and torch.equal(c1, fa[1])
    assert int(cnt.sum()) > 0 and int((cnt[vis] > 0).sum()) > 0.5 * int(vis.sum())
    assert torch.equal(cnt, cnt2) and torch.equal(mw, mw2)
    assert rel_l1(sw.cpu().numpy(), sw2.cpu().numpy()) <= 1e-5
    assert rel_l1(sgw.cpu().numpy(), sgw2.cpu().numpy()) <= 1e-5
    # and they are not the plain frame's
    _c3, _r3, (sw3, _g3, _m3, _n3) = GaussianRasterizer(_settings(s)).contributions(d["means3D"], d["opacities"], **kw(d))
    assert rel_l1(sw3.cpu().numpy(), sw.cpu().numpy()) > 1e-2
