"""Absolute-gradient densification statistics (RR_FLAG_ABSGRAD; AbsGS, gsplat's absgrad) on the GPU.

The reference is tests/absgrad_ref.py, a float64 walk of the oracle's tile lists whose signed sums are pinned
to the oracle's dL_dmeans2D by tests/test_absgrad_ref_cpu.py.  Bars: the project's parity bar of 1e-4 relative
L1 against the reference (the absolute sums have no cancellation, so they are better conditioned than the
signed ones already held to it), 1e-5 between GPU runs that differ only in the order of their float atomics,
and test_fused_gpu.py's own bars for the fused step.  Frames are at most 128 x 96."""
import numpy as np
import pytest
import torch

from rain_amd import _native as N
from rain_amd import cameras, fused, synthetic
from rain_amd import renderer as renderer_mod
from rain_amd.gaussian_model import GaussianModel, OptimizationParams
from rain_amd.renderer import PipelineParams, render
from rain_amd.train import TrainConfig, Trainer
from tests import absgrad_ref as AB
from tests import antialias_ref as AR
from tests.common import GRAD_NAMES, rel_l1

pytestmark = pytest.mark.gpu
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


@pytest.fixture(params=[0, 2], ids=["default_binning", "early_stop_split2"])
def binning(request):
    if request.param:
        N.check(N.raster().rr_set_binning_config(request.param, 1), "binning config")
    yield request.param
    N.check(N.raster().rr_set_binning_config(0, 0), "binning config")


_REF = {}


def _reference(oracle, name):
    """Per scene, computed once and left unchanged: inputs, the colour gradient and the reference run."""
    if name not in _REF:
        inp, st, dpix = AB.single_gaussian() if name == "single" else AB.scene(name)
        _REF[name] = dict(inp=inp, st=st, dpix=dpix, ref=AB.reference(oracle, inp, st, dpix))
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


def _same_up_to_atomics(label, on, off):
    """`on` is `off` up to the order of the blend backward's float atomics, which differs between two launches
    (and between the two blend variants, whose waves finish in another order): the project's 1e-5 run-to-run
    bar."""
    for k, a, b in zip(GRAD_NAMES, on, off):
        if a.numel() == 0:
            assert b.numel() == 0
            continue
        err = rel_l1(a.cpu().numpy(), b.cpu().numpy())
        assert err <= 1e-5, (label, k, err)


def _abs_route1(t, gpu):
    """(9-tuple of rasterize_gaussians_backward_abs, the forward) of a reference entry."""
    from rain_amd.diff_gaussian_rasterization import _C

    d, s = _gpu_inputs(t["inp"], t["st"], gpu)
    fw = _C.rasterize_gaussians(*_forward_args(d, s))
    got = _C.rasterize_gaussians_backward_abs(*_backward_args(d, s, fw, torch.from_numpy(t["dpix"]).to(gpu)))
    return got, fw, d, s


# ---- 1. the _C route ----

@pytest.mark.parametrize("scene", list(AB.SCENES))
def test_abs_sums_match_the_reference_and_the_rest_is_untouched(oracle, gpu, binning, scene):
    from rain_amd.diff_gaussian_rasterization import _C

    t = _reference(oracle, scene)
    ref = t["ref"]
    got, fw, d, s = _abs_route1(t, gpu)
    assert len(got) == 9 and not _C.absgrad_on()
    P, W, H = d["means3D"].shape[0], s["image_width"], s["image_height"]
    if scene in ("sh3", "ragged_bg"):  # many 64-pair rounds with odd tails
        tile_max = _C.debug_views(fw[-3], fw[-2], fw[-1], fw[0], P, W, H)["tile_max"]
        assert int(tile_max.max()) > 128 and int(tile_max.max()) % 64 != 0
    dpix = torch.from_numpy(t["dpix"]).to(gpu)
    off = _C.rasterize_gaussians_backward(*_backward_args(d, s, fw, dpix))
    torch.cuda.synchronize()
    assert len(off) == 8
    a = got[8].cpu().numpy()
    assert a.shape == (P, 3) and np.isfinite(a).all()
    assert np.all(a[:, 2] == 0)
    hidden = ref["radii"] <= 0
    assert np.array_equal(fw[2].cpu().numpy(), ref["radii"])
    assert np.abs(a[hidden]).sum() == 0.0
    err = rel_l1(a[:, :2], ref["abs"])
    print(f"{scene}: dL_dmeans2D_abs vs reference, relative L1 {err:.3e}")
    assert err <= 1e-4, err
    # a visible Gaussian no pixel blended gets exactly 0, like the reference
    assert np.all(a[:, :2][ref["abs"] == 0] == 0)
    # A >= |dL_dmeans2D| per component, up to the rounding of two differently ordered fp32 sums
    signed = np.abs(got[0].cpu().numpy()[:, :2])
    assert np.all(a[:, :2] >= signed - 1e-5 * a[:, :2])
    _same_up_to_atomics(scene, got[:8], off)
    # inside the block the 8-tuple entry uses the flag too and returns the same 8 gradients
    with _C.absgrad():
        inside = _C.rasterize_gaussians_backward(*_backward_args(d, s, fw, dpix))
    assert len(inside) == 8
    _same_up_to_atomics(scene + " (inside the block)", inside, off)


# ---- 2. the analytic case ----

def test_single_centred_gaussian(oracle, gpu, binning):
    t = _reference(oracle, "single")
    got, _fw, _d, _s = _abs_route1(t, gpu)
    a = got[8].cpu().numpy()[0, :2].astype(np.float64)
    signed = got[0].cpu().numpy()[0, :2].astype(np.float64)
    print(f"single Gaussian: signed {signed}, abs {a}, reference abs {t['ref']['abs'][0]}")
    assert np.all(a > 0)
    assert np.all(np.abs(signed) <= 1e-3 * a)
    assert rel_l1(a, t["ref"]["abs"][0]) <= 1e-4


# ---- 3. the raw-parameter route ----

def _raw_params(name):
    """The scene's raw parameters with test_fused_gpu.py's perturbations: non-unit quaternions and anisotropic
    scales (the bench scene's splats are isotropic, which leaves the rotation gradient pure rounding noise)."""
    kw = AB.SCENES[name]
    p = synthetic.random_gaussians(kw["P"], sh_degree=kw["sh_degree"], seed=0, bench=True)
    p["rotation"] = p["rotation"] * 1.7
    p["scaling"] = p["scaling"] + 0.4 * torch.randn(p["scaling"].shape, generator=torch.Generator().manual_seed(0))
    return p


def _scene_model(name, dev="cuda"):
    """The GaussianModel of _raw_params(name) and the scene's camera."""
    kw = AB.SCENES[name]
    g = GaussianModel(kw["sh_degree"], divide_ratio=0.8, device=dev)
    g.set_params(_raw_params(name))
    g.active_sh_degree = kw["sh_degree"]
    g.spatial_lr_scale = 4.4
    cam = cameras.fibonacci_cameras(8, kw["W"], kw["H"])[0].to(dev)
    return g, cam


def _model_reference(oracle, name):
    """_reference() of the scene _scene_model(name) renders: the getters' values of its raw parameters (computed
    once and left unchanged)."""
    key = "model:" + name
    if key not in _REF:
        _inp, st, dpix = AB.scene(name)
        act = synthetic.activated(_raw_params(name))
        inp = {k: act[k].float().contiguous() for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        _REF[key] = dict(inp=inp, st=st, dpix=dpix, ref=AB.reference(oracle, inp, st, dpix))
    return _REF[key]


def _params(g):
    return dict(zip(NAMES, (g._xyz, g._features_dc, g._features_rest, g._opacity, g._scaling, g._rotation)))


def _rl(a, b):
    return rel_l1(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def _stats(P, seed=1):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand((P, 1), device="cuda", generator=gen), torch.randint(0, 4, (P, 1), device="cuda",
                                                                            generator=gen).float(),
            torch.randint(0, 12, (P,), device="cuda", generator=gen).float())


@pytest.mark.parametrize("scene", ["sh3", "ragged_bg"])
def test_raw_route_statistics_and_gradients(oracle, gpu, binning, scene):
    t = _model_reference(oracle, scene)
    ref = t["ref"]
    bg = t["st"]["bg"].to(gpu)
    dimg = torch.from_numpy(t["dpix"]).to(gpu)
    P = ref["radii"].shape[0]
    runs = {}
    for on in (False, True):
        g, cam = _scene_model(scene)
        _color, radii, _depth, st = fused.forward(g, cam, bg, 0.3)
        vis = radii.cpu().numpy() > 0
        # (the in-kernel activations may round a radius differently from the oracle's inputs: a few rows at most)
        assert int((vis != (ref["radii"] > 0)).sum()) <= 2
        acc, den, mr = _stats(P)
        # visible rows start at 0, so that their growth is read without the rounding of (acc + x) - acc
        acc = torch.where(torch.from_numpy(vis).to(gpu).view(-1, 1), torch.zeros_like(acc), acc)
        before = acc.clone(), den.clone(), mr.clone()
        grads = {k: torch.empty_like(v) for k, v in _params(g).items()}
        d2 = torch.empty((P, 3), device=gpu)
        dabs = torch.full((P, 3), 7.0, device=gpu) if on else None
        fused.backward(st, dimg, grads, (acc, den, mr), dmeans2D=d2, absgrad=bool(on), dmeans2D_abs=dabs)
        torch.cuda.synchronize()
        runs[on] = dict(grads=grads, d2=d2, dabs=dabs, stats=(acc, den, mr), before=before)
    on, off = runs[True], runs[False]
    a = on["dabs"].cpu().numpy()
    assert np.all(a[:, 2] == 0) and np.abs(a[~vis]).sum() == 0.0
    assert rel_l1(a[:, :2], ref["abs"]) <= 1e-4
    # grad_accum grows by the norm of the absolute sums on visible rows, and not at all elsewhere
    grown = (on["stats"][0] - on["before"][0]).cpu().numpy()[:, 0]
    want = np.linalg.norm(ref["abs"], axis=1)
    err = rel_l1(grown[vis], want[vis])
    print(f"{scene}: grad_accum growth vs |abs| of the reference, relative L1 {err:.3e}")
    assert err <= 1e-4
    assert torch.equal(on["stats"][0][~torch.from_numpy(vis).to(gpu)], on["before"][0][~torch.from_numpy(vis).to(gpu)])
    signed_growth = (off["stats"][0] - off["before"][0]).cpu().numpy()[:, 0]
    assert grown[vis].sum() > 3 * signed_growth[vis].sum()  # and it is not the signed statistic
    # denom + 1 on visible rows, max_radii2D as without the flag
    assert torch.equal(on["stats"][1], on["before"][1] + torch.from_numpy(vis).to(gpu).float().view(-1, 1))
    assert torch.equal(on["stats"][1], off["stats"][1])
    assert torch.equal(on["stats"][2], off["stats"][2])
    # every gradient, the signed dmeans2D included, is the flag-off run's (up to the order of the atomics)
    for k in NAMES:
        x, y = on["grads"][k], off["grads"][k]
        assert float(y.abs().sum()) > 0 and _rl(x, y) <= 1e-5, (k, _rl(x, y))
    assert _rl(on["d2"], off["d2"]) <= 1e-5


def _geometry_arrays(geom, radii, P):
    import ctypes

    offs = (ctypes.c_size_t * 5)()
    N.check(N.raster().rr_geometry_layout(P, offs), "layout")
    nb = (P + 255) // 256
    sizes = (48 * P, 8 * P, 4 * P, 8 * nb, 4 * nb)
    return [geom[offs[k]:offs[k] + sizes[k]].clone() for k in range(5)] + [radii.clone()]


def test_raw_route_with_adam_and_next_frame(oracle, gpu, binning):
    """The flag with the fused Adam step and the next frame's preprocess inside the backward, and with the
    workspace the forward registered: parameters and moments equal the flag-off run's (test_fused_gpu.py's
    bars), the next frame's geometry is the preprocess of the stepped parameters bit for bit, and the
    statistics are the absolute ones."""
    t = _model_reference(oracle, "sh3")
    ref = t["ref"]
    bg = t["st"]["bg"].to(gpu)
    dimg = torch.from_numpy(t["dpix"]).to(gpu)
    P = ref["radii"].shape[0]
    models, accs = [], []
    for on in (False, True):
        g, cam = _scene_model("sh3")
        cam1 = cameras.fibonacci_cameras(8, 128, 96)[3].to("cuda")
        g.training_setup(OptimizationParams())
        acc, den, mr = (torch.zeros((P, 1), device=gpu), torch.zeros((P, 1), device=gpu), torch.zeros((P,), device=gpu))
        cache = fused.BinningCache()
        _color, radii, _depth, st = fused.forward(g, cam, bg, 0.3, cache=cache)
        vis = radii > 0
        assert int((vis.cpu().numpy() != (ref["radii"] > 0)).sum()) <= 2  # (in-kernel activations: see above)
        nxt = fused.prepare_next(g, cam1, bg, 0.3)
        fused.backward(st, dimg, None, (acc, den, mr), adam=g.optimizer.fused_step(g), next_frame=nxt, absgrad=on)
        got = _geometry_arrays(nxt.geom, nxt.radii, P)
        _c, ref_radii, _d, ref_st = fused.forward(g, cam1, bg, 0.3)
        want = _geometry_arrays(ref_st.geom, ref_radii, P)
        nvis = want[5] > 0
        for n, x, y in zip(("splats", "tiles", "depth_keys", "block_sums", "block_wide", "radii"), got, want):
            if n == "splats":  # a culled row's record is never written (nor read): visible rows only
                x, y = x.view(P, 48)[nvis].view(torch.float32), y.view(P, 48)[nvis].view(torch.float32)
            assert torch.equal(x, y), (on, n)
        models.append(g)
        accs.append((acc, den, mr))
    a, b = models
    for k in NAMES:
        x, y = _params(a)[k].detach(), _params(b)[k].detach()
        assert (x - y).abs().max() <= 1e-5 * max(1.0, float(y.abs().max())), (k, float((x - y).abs().max()))
    for pa, pb in zip(a.params(), b.params()):
        sa, sb = a.optimizer.state[pa], b.optimizer.state[pb]
        assert float(sa["step"]) == float(sb["step"]) == 1.0
        for m in ("exp_avg", "exp_avg_sq"):
            x, y = sa[m], sb[m]
            scale = max(float(y.abs().max()), 1e-30)
            assert float((x - y).abs().max()) <= 1e-4 * scale, (m, float((x - y).abs().max()), scale)
            assert _rl(x, y) < 1e-4, (m, _rl(x, y))
    (acc0, den0, mr0), (acc1, den1, mr1) = accs
    assert torch.equal(den0, den1) and torch.equal(mr0, mr1) and torch.equal(den1[:, 0], vis.float())
    assert rel_l1(acc1.cpu().numpy()[:, 0], np.linalg.norm(ref["abs"], axis=1)) <= 1e-4
    assert float(acc1.sum()) > 3 * float(acc0.sum())


# ---- 4. autograd ----

def test_gaussian_rasterizer_autograd(oracle, gpu, binning):
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    t = _reference(oracle, "sh3")
    route1, _fw, d, s = _abs_route1(t, gpu)
    dpix = torch.from_numpy(t["dpix"]).to(gpu)
    res = {}
    for on in (False, True):
        leaves = {k: d[k].clone().requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        means2D = torch.zeros_like(d["means3D"], requires_grad=True)
        r = GaussianRasterizer(_settings(s))
        r.absgrad = on
        color, _radii, _depth = r(leaves["means3D"], means2D, leaves["opacities"], shs=leaves["shs"],
                                  scales=leaves["scales"], rotations=leaves["rotations"])
        (color * dpix).sum().backward()
        assert not _C.absgrad_on()
        res[on] = (means2D, leaves)
    m_off, l_off = res[False]
    m_on, l_on = res[True]
    assert not hasattr(m_off, "absgrad")
    assert m_on.absgrad.shape == m_on.shape
    assert _rl(m_on.absgrad, route1[8]) <= 1e-5  # route 1's tensor, up to the order of the atomics
    assert rel_l1(m_on.absgrad.cpu().numpy()[:, :2], t["ref"]["abs"]) <= 1e-4
    assert _rl(m_on.grad, m_off.grad) <= 1e-5 and _rl(m_on.grad, route1[0]) <= 1e-5  # .grad stays the signed one
    for k in l_on:
        assert _rl(l_on[k].grad, l_off[k].grad) <= 1e-5, k


@pytest.mark.parametrize("raw", [False, True], ids=["getters_route", "raw_route"])
def test_render_leaves_absgrad_on_viewspace_points(oracle, gpu, binning, monkeypatch, raw):
    t = _model_reference(oracle, "sh3")
    monkeypatch.setattr(renderer_mod, "RAW_RENDER", raw)
    bg = t["st"]["bg"].to(gpu)
    dpix = torch.from_numpy(t["dpix"]).to(gpu)
    out = {}
    for on in (False, True):
        g, cam = _scene_model("sh3")
        pkg = render(cam, g, PipelineParams(), bg, absgrad=on)
        assert pkg["render"].grad_fn.__class__.__name__.startswith("RasterizeRawParams") == raw
        (pkg["render"] * dpix).sum().backward()
        out[on] = (pkg["viewspace_points"], {k: v.grad.clone() for k, v in _params(g).items()})
    (v_off, g_off), (v_on, g_on) = out[False], out[True]
    assert not hasattr(v_off, "absgrad")
    assert v_on.absgrad.shape == (t["ref"]["radii"].shape[0], 3)
    assert rel_l1(v_on.absgrad.cpu().numpy()[:, :2], t["ref"]["abs"]) <= 1e-4
    assert float(v_on.absgrad[:, 2].abs().sum()) == 0.0
    assert _rl(v_on.grad, v_off.grad) <= 1e-5
    for k in NAMES:
        assert _rl(g_on[k], g_off[k]) <= 1e-5, k
    # and the model's statistics read it
    vis = pkg["visibility_filter"]
    P = vis.shape[0]
    for g, v, flag in ((GaussianModel(3, device="cuda"), v_on, True), (GaussianModel(3, device="cuda"), v_off, False)):
        g.xyz_gradient_accum, g.denom = torch.zeros((P, 1), device=gpu), torch.zeros((P, 1), device=gpu)
        g.max_radii2D = torch.zeros((P,), device=gpu)
        g.add_densification_stats(v, vis, absgrad=flag)
        src = v.absgrad if flag else v.grad
        want = torch.where(vis, torch.norm(src[:, :2], dim=-1), torch.zeros((), device=gpu))
        assert float(((g.xyz_gradient_accum[:, 0] - want).abs() / want.abs().clamp_min(1e-30)).max()) <= 2.5e-7
        assert torch.equal(g.denom[:, 0], vis.float())


# ---- 5. with anti-aliasing ----

def test_antialiased_frame_sees_the_compensated_opacity(oracle, gpu, binning):
    """The absolute terms of an anti-aliased frame are those of the plain frame whose opacities are
    float32(o comp), comp from tests/antialias_ref.py."""
    from rain_amd.diff_gaussian_rasterization import _C

    inp, st = AR.scene("small_sh3")
    inp_c, _comp = AR.compensated(st, inp)
    H, W = st["image_height"], st["image_width"]
    dpix = torch.from_numpy(np.random.default_rng(5).standard_normal((3, H, W)).astype(np.float32)).to(gpu)
    d, s = _gpu_inputs(inp, st, gpu)
    dc, _ = _gpu_inputs(inp_c, st, gpu)
    with _C.antialiased():
        fa = _C.rasterize_gaussians(*_forward_args(d, s))
        ga = _C.rasterize_gaussians_backward_abs(*_backward_args(d, s, fa, dpix))
        ga_off = _C.rasterize_gaussians_backward(*_backward_args(d, s, fa, dpix))
    fp = _C.rasterize_gaussians(*_forward_args(dc, s))
    gp = _C.rasterize_gaussians_backward_abs(*_backward_args(dc, s, fp, dpix))
    plain = _C.rasterize_gaussians_backward_abs(*_backward_args(d, s, _C.rasterize_gaussians(*_forward_args(d, s)), dpix))
    torch.cuda.synchronize()
    assert torch.equal(fa[2], fp[2])
    err = _rl(ga[8], gp[8])
    print(f"small_sh3: abs sums of the anti-aliased frame vs the pre-compensated plain frame, relative L1 {err:.3e}")
    assert float(gp[8].abs().sum()) > 0 and err <= 1e-4
    assert _rl(plain[8], ga[8]) > 1e-2  # and not those of the plain frame
    _same_up_to_atomics("small_sh3 antialiased", ga[:8], ga_off)  # the AA kernels' other outputs stand


# ---- 6. trainer ----

def _train_model(P, seed):
    g = GaussianModel(3, divide_ratio=0.8, device="cuda")
    g.set_params(synthetic.random_gaussians(P, sh_degree=3, seed=seed, bench=True))
    g.active_sh_degree = 3
    g.spatial_lr_scale = 4.4
    return g


def test_trainer_accumulates_absolute_statistics_and_densifies_on_them(gpu, binning):
    P, W, H, V = 2000, 128, 96, 6
    cams = [c.to("cuda") for c in cameras.fibonacci_cameras(V, W, H)]
    gts = [torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(20 + i))
           for i in range(V)]
    runs, first = {}, {}
    for label, fuse, on in (("fused_on", True, True), ("api_on", False, True), ("fused_off", True, False)):
        g = _train_model(P, 2)
        opt = OptimizationParams(densify_absgrad=on)  # densification starts at 500: none in these steps
        g.training_setup(opt)
        t = Trainer(g, cams, gts, opt, PipelineParams(), cfg=TrainConfig(c2f=False, seed=3), scene_extent=4.4,
                    fused=fuse)
        assert t.options.absgrad is on
        for it in (1, 2, 3):
            assert not t.step(it).densified
            if it == 1:  # formed on the initial parameters, which the three runs share bit for bit
                first[label] = g.xyz_gradient_accum[:, 0].clone()
        torch.cuda.synchronize()
        assert g.get_xyz.shape[0] == P
        runs[label] = (g, t)
    acc = {k: g.xyz_gradient_accum[:, 0].clone() for k, (g, _t) in runs.items()}
    den = {k: g.denom[:, 0].clone() for k, (g, _t) in runs.items()}
    assert torch.equal(den["fused_on"], den["api_on"]) and torch.equal(den["fused_on"], den["fused_off"])
    seen = den["fused_on"] > 0
    assert int(seen.sum()) > P // 4
    err = _rl(acc["fused_on"], acc["api_on"])
    print(f"trainer: fused vs reference-API accumulator, relative L1 {err:.3e}")
    assert err <= 1e-4
    # Every visible row exceeds the flag-off run's.  On one set of parameters this is |sum| <= sum |.|, up to the
    # rounding of two differently ordered fp32 sums: test 1's per-component bound a >= |s| - 1e-5 a, hence
    # |A| (1 + 1e-5) >= |signed| row by row.  The first step of the three runs is formed on the same initial
    # parameters, so it is asserted there exactly so.
    for k in ("fused_on", "api_on"):
        short = (first["fused_off"] - first[k] * (1 + 1e-5)).clamp_min(0)
        print(f"trainer, step 1: {k} below fused_off by at most {float(short.max()):.3e} (mean row "
              f"{float(first['fused_off'].mean()):.3e})")
        assert bool((first[k] * (1 + 1e-5) >= first["fused_off"]).all()), (k, float(short.max()))
        assert int((first[k] > first["fused_off"]).sum()) > int((first["fused_off"] > 0).sum()) // 2, k
    # After three steps the runs are separate trainings whose parameters differ from the second step on by the
    # order of their float atomics, and a row that a single pixel blends has abs == |signed| exactly, so such a row
    # may land on either side by that run-to-run deviation: row by row, the same relative slack plus the project's
    # 1e-5 run-to-run bar taken per row (1e-5 of the mean flag-off row, the bar's relative L1 spread evenly).
    off = acc["fused_off"][seen]
    atol = 1e-5 * float(off.mean())
    for k in ("fused_on", "api_on"):
        deficit = (off - acc[k][seen]).clamp_min(0)
        print(f"trainer: {k} below fused_off on {int((deficit > 0).sum())} of {int(seen.sum())} rows; total shortfall "
              f"{float(deficit.sum()):.3e} of {float(off.sum()):.3e}, largest {float(deficit.max()):.3e} (atol {atol:.3e})")
        assert bool((acc[k][seen] * (1 + 1e-5) + atol >= off).all()), (k, float(deficit.max()))
        assert float(deficit.sum()) <= 1e-5 * float(off.sum()), k
        assert int((acc[k][seen] > off).sum()) > int((off > 0).sum()) // 2, k
        assert float(acc[k].sum()) > 3 * float(acc["fused_off"].sum())
    assert float(acc["fused_on"][~seen].abs().sum()) == 0.0
    # one densify event at a threshold set to the median of the flag-on average
    avg = {k: torch.where(den[k] > 0, acc[k] / den[k], torch.zeros_like(acc[k])) for k in acc}
    thr = float(avg["fused_on"][seen].median())
    n_on, n_off = int((avg["fused_on"] >= thr).sum()), int((avg["fused_off"] >= thr).sum())
    assert n_on >= n_off and n_on >= int(seen.sum()) // 2
    g, t = runs["fused_on"]
    raw = {n: p.detach().clone() for n, p in zip(NAMES, (g._xyz, g._features_dc, g._features_rest, g._opacity,
                                                           g._scaling, g._rotation))}
    # the torch restatement of the selection (gaussian_model.py:339-415) from the accumulators
    grads = g.xyz_gradient_accum / g.denom
    grads[grads.isnan()] = 0.0
    smax = torch.exp(raw["scaling"]).max(dim=1).values
    extent = float(smax.median()) / g.percent_dense  # the clone / split boundary at the median scale: both happen
    sel = torch.norm(grads, dim=-1) >= thr
    assert int(sel.sum()) == n_on
    split = sel & (smax > g.percent_dense * extent)
    clone = sel & (smax <= g.percent_dense * extent)
    op = torch.sigmoid(raw["opacity"]).squeeze(1)
    keep_orig, keep_clone = ~split & (op >= 0.005), clone & (op >= 0.005)
    g.densify_and_prune(thr, 0.005, extent, None, generator=torch.Generator(device="cuda").manual_seed(11))
    A, B = int(keep_orig.sum()), int(keep_clone.sum())
    new_xyz, new_op = g._xyz.detach(), g._opacity.detach()
    assert int(split.sum()) > 0 and B > 0
    assert torch.equal(new_xyz[:A], raw["xyz"][keep_orig])  # the survivors, in order
    assert torch.equal(new_xyz[A:A + B], raw["xyz"][keep_clone])  # the clones of exactly the selected small ones
    # the children of exactly the selected large ones: their parents' opacities, twice
    kids = raw["opacity"][split & (op >= 0.005)]
    assert new_xyz.shape[0] == A + B + 2 * kids.shape[0]
    assert torch.equal(new_op[A + B:], torch.cat([kids, kids]))
