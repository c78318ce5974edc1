"""CPU checks of the contribution-statistics / importance-pruning surface: the library exports and lists
rr_contributions, every argument error comes back as RR_ERR_ARG + a message before any device work (the
pointers below are stand-ins, so a call that got past validation would fault), the Python layers have the
documented signatures and no CPU fallback, OptimizationParams has the documented defaults, the sharded
trainer refuses the option, and prune_mask works on CPU tensors."""
import ctypes
import inspect
import os

import pytest
import torch

from rain_amd import _native as N
from rain_amd import cameras, synthetic
from rain_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C
from rain_amd.gaussian_model import GaussianModel, OptimizationParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_ERR_ARG = 1


def test_symbol_exported_declared_and_listed():
    so = ctypes.CDLL(N.RASTER_LIB)
    header = open(os.path.join(ROOT, "include", "rain_raster.h")).read()
    assert hasattr(so, "rr_contributions"), "librain_raster.so does not export rr_contributions"
    assert "rr_contributions" in N.RASTER_SYMBOLS and "rr_contributions(" in header
    assert "} rr_contrib;" in header and "wraps past 2^32" in header
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert list(N.raster().rr_contributions.argtypes) == [ctypes.POINTER(N.RRFrame), vp, vp, vp, vp, ci, vp, ci, vp, vp]
    assert ctypes.sizeof(N.RRContrib) == 16
    assert [f[0] for f in N.RRContrib._fields_] == ["sum_w", "sum_gw", "max_w", "count"]


def test_rr_contributions_validation_without_gpu():
    L = N.raster()
    f = N.RRFrame(10, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0)
    base = dict(frame=f, radii=16, geom=16, img=16, binning=16, R=5, g=16, acc=0, out=16)

    def call(**kw):
        a = dict(base, **kw)
        return L.rr_contributions(ctypes.byref(a["frame"]) if a["frame"] is not None else None, a["radii"], a["geom"],
                                  a["img"], a["binning"], a["R"], a["g"], a["acc"], a["out"], None)

    def err():
        return L.rr_last_error()

    assert call(frame=None) == RR_ERR_ARG and b"null frame" in err()
    for acc in (0, 1):
        assert call(out=None, acc=acc) == RR_ERR_ARG and b"null output" in err()
        for bad in (4, 8, 17, 24):
            assert call(out=bad, acc=acc) == RR_ERR_ARG and b"16-byte aligned" in err()
        for kw in (dict(radii=None), dict(geom=None), dict(img=None)):
            assert call(acc=acc, **kw) == RR_ERR_ARG and b"null buffer" in err(), kw
        assert call(R=-1, acc=acc) == RR_ERR_ARG and b"num_rendered" in err()
        for bad in (N.RRFrame(-1, 0, 1, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0),
                    N.RRFrame(10, 0, 1, 0, 48, 0.5, 0.4, 1.0, 0.3, 0, 0),
                    N.RRFrame(10, 0, 1, 64, -2, 0.5, 0.4, 1.0, 0.3, 0, 0)):
            assert call(frame=bad, acc=acc) == RR_ERR_ARG and b"bad P / width / height" in err()
        # P == 0: no records, nothing launched, whatever the buffers are
        f0 = N.RRFrame(0, 0, 0, 64, 48, 0.5, 0.4, 1.0, 0.3, 0, 0)
        assert call(frame=f0, acc=acc, radii=None, geom=None, img=None, binning=None, R=0) == 0
        assert call(frame=f0, acc=acc, out=None) == RR_ERR_ARG  # ... but out is still checked


def _settings():
    return GaussianRasterizationSettings(
        image_height=48, image_width=64, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0,
        viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False,
        debug=False, low_pass=0.3)


def test_python_signatures_and_no_cpu_fallback():
    from rain_amd import compact, importance  # noqa: F401  (the CLI module imports)

    assert list(inspect.signature(_C.gaussian_contributions).parameters) == [
        "radii", "geomBuffer", "binningBuffer", "imageBuffer", "num_rendered", "P", "W", "H", "pixel_weight", "out"]
    sig = inspect.signature(_C.gaussian_contributions).parameters
    assert sig["pixel_weight"].default is None and sig["out"].default is None
    sig = inspect.signature(GaussianRasterizer.contributions).parameters
    assert list(sig) == ["self", "means3D", "opacities", "shs", "colors_precomp", "scales", "rotations",
                         "cov3D_precomp", "pixel_weight", "out"]
    assert all(sig[k].default is None for k in list(sig)[3:])
    sig = inspect.signature(importance.accumulate_contributions).parameters
    assert list(sig)[:5] == ["gaussians", "views", "pipe", "background", "pixel_weight_fn"]
    assert sig["pixel_weight_fn"].default is None
    sig = inspect.signature(importance.importance_scores).parameters
    assert list(sig) == ["stats", "gaussians", "kind", "volume_power"]
    assert sig["kind"].default == "weight_volume" and sig["volume_power"].default == 0.1
    assert importance.KINDS == ("weight_volume", "weight", "max_weight", "count")
    sig = inspect.signature(importance.prune_mask).parameters
    assert list(sig) == ["scores", "fraction", "threshold"] and sig["fraction"].default is None
    sig = inspect.signature(GaussianModel.prune_by_importance).parameters
    assert list(sig) == ["self", "scores", "fraction", "threshold"]
    assert sig["fraction"].default is None and sig["threshold"].default is None
    opt = OptimizationParams()
    assert (opt.importance_prune_iterations, opt.importance_prune_fraction, opt.importance_prune_kind) == \
        ((), 0.0, "weight_volume")
    # CPU tensors: refused, not computed some other way
    r = GaussianRasterizer(_settings())
    m = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.contributions(m, torch.zeros(5, 1), shs=torch.zeros(5, 1, 3), scales=m, rotations=torch.zeros(5, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C.gaussian_contributions(torch.zeros(5, dtype=torch.int32), torch.zeros(8, dtype=torch.uint8),
                                  torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8), 3, 5, 64, 48)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r.contributions(m, torch.zeros(5, 1), scales=m, rotations=torch.zeros(5, 4))
    with pytest.raises(ValueError, match="kind must be one of"):
        importance.importance_scores(importance.ContributionStats(torch.zeros(5, 4)), None, kind="volume")


def test_contribution_stats_views_and_scores_on_cpu():
    from rain_amd import importance

    buf = torch.zeros(6, 4)
    buf[:, 0] = torch.tensor([1.0, 2.0, 0.0, 4.0, 0.5, 3.0])
    buf[:, 1] = 2 * buf[:, 0]
    buf[:, 2] = torch.tensor([0.5, 0.9, 0.0, 0.2, 0.1, 0.3])
    buf.view(torch.int32)[:, 3] = torch.tensor([3, 7, 0, 40, 9, 12], dtype=torch.int32)
    st = importance.ContributionStats(buf, 2)
    assert st.count.dtype == torch.int32 and st.count.tolist() == [3, 7, 0, 40, 9, 12]
    assert torch.equal(importance.importance_scores(st, None, "weight"), buf[:, 1])
    assert torch.equal(importance.importance_scores(st, None, "max_weight"), buf[:, 2])
    assert importance.importance_scores(st, None, "count").tolist() == [3.0, 7.0, 0.0, 40.0, 9.0, 12.0]
    g = GaussianModel(0, device="cpu")
    g.set_params(synthetic.random_gaussians(6, sh_degree=0, seed=0, bench=True))
    s = importance.importance_scores(st, g, "weight_volume", volume_power=0.1)
    vol = torch.prod(g.get_scaling.detach(), dim=1)
    q90 = torch.sort(vol).values[5]  # ceil(0.9 * 6) = 6th smallest
    assert torch.allclose(s, buf[:, 1] * torch.clamp(vol / q90, 0, 1) ** 0.1)
    assert s.shape == (6,) and bool(torch.isfinite(s).all())


def test_prune_mask_on_cpu_tensors():
    from rain_amd.importance import prune_mask

    s = torch.tensor([3.0, 1.0, 2.0, 1.0, 5.0, 1.0, 0.5, 4.0])
    for bad in (dict(), dict(fraction=0.5, threshold=1.0)):
        with pytest.raises(ValueError, match="exactly one"):
            prune_mask(s, **bad)
    with pytest.raises(ValueError, match="fraction"):
        prune_mask(s, fraction=1.5)
    # floor(0.375 * 8) = 3 go: the 0.5, then the first two of the three tied 1.0s by index
    m = prune_mask(s, fraction=0.375)
    assert m.dtype == torch.bool and m.tolist() == [False, True, False, True, False, False, True, False]
    for frac in (0.0, 0.1, 0.25, 0.5, 0.6, 0.99, 1.0):
        assert int(prune_mask(s, fraction=frac).sum()) == int(frac * 8)
    tied = torch.zeros(101)
    m = prune_mask(tied, fraction=0.3)  # all equal: exactly 30, the lowest indices
    assert int(m.sum()) == 30 and bool(m[:30].all())
    assert prune_mask(s, threshold=1.0).tolist() == [False, False, False, False, False, False, True, False]
    assert prune_mask(s, threshold=2.5).tolist() == [False, True, True, True, False, True, True, False]
    assert prune_mask(torch.zeros(0), fraction=0.5).shape == (0,)


def test_prune_by_importance_on_a_cpu_model():
    g = GaussianModel(1, device="cpu")
    g.set_params(synthetic.random_gaussians(40, sh_degree=1, seed=0, bench=True))
    g.training_setup(OptimizationParams())
    before = g._xyz.detach().clone()
    scores = torch.arange(40, dtype=torch.float32).flip(0)  # the last rows score lowest
    mask = g.prune_by_importance(scores, fraction=0.25)
    assert int(mask.sum()) == 10 and bool(mask[30:].all())
    assert g._xyz.shape[0] == 30 and torch.equal(g._xyz.detach(), before[:30])
    assert g.denom.shape[0] == 30 and g.max_radii2D.shape[0] == 30 and g.xyz_gradient_accum.shape[0] == 30
    with pytest.raises(ValueError, match="entries"):
        g.prune_by_importance(scores, fraction=0.25)  # stale scores of the old size


def _ref_loss(img, gt, lam):
    return (img - gt).abs().mean()


def test_sharded_trainer_refuses_importance_pruning():
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

    t = trainer(importance_prune_iterations=(6,), importance_prune_fraction=0.3)
    assert not t.sharded
    assert not t.options.prune_at(5) and t.options.prune_at(6)
    t.sharded = True  # what world > 1 (or a forced exchange) sets; no ranks are started
    for it in (1, 6):
        with pytest.raises(ValueError, match="importance_prune_iterations needs the single-GPU step"):
            t.step(it)
    t0 = trainer()  # the defaults pass, sharded or not, and never prune
    t0.sharded = True
    o0 = resolve_options(t0.opt, t0.pipe, t0.sharded)
    assert not any(o0.prune_at(it) for it in (0, 1, 6, 30_000))
    t1 = trainer(importance_prune_iterations=(6,))  # no fraction: nothing to remove
    assert not t1.options.prune_at(6)
