"""Trainer with the depth-distortion term (OptimizationParams.lambda_dist): the fused step and the
autograd step agree over a few steps, alone and together with lambda_normal (the bars of
test_geom_loss_gpu.py's same comparison), and with lambda_dist = 0 the step is bitwise today's."""
import pytest
import torch

from rain_amd import cameras
from rain_amd.gaussian_model import OptimizationParams
from rain_amd.train import TrainConfig, Trainer
from tests.test_geom_loss_gpu import _model, _params, rel_l1

pytestmark = pytest.mark.gpu

# alone over the NDC depth (a narrow range of m, hence 2DGS's large weight), and together with the
# depth-normal consistency over the metric depth
CONFIGS = {
    "dist_ndc": dict(lambda_dist=100.0, dist_near=0.2, dist_far=100.0),
    "dist_metric+normal": dict(lambda_dist=0.05, dist_near=0.0, dist_far=0.0, lambda_normal=0.05,
                               lambda_normal_from_iter=1),
}


def _trainer(use_fused, P=8_000, W=128, H=96, V=6, steps=5, drop_attr=False, **kw):
    cams = [c.to("cuda") for c in cameras.fibonacci_cameras(V, W, H)]
    gts = [torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(10 + i)) for i in range(V)]
    g = _model(P, seed=2, sh_degree=3)
    # no densify / prune or opacity reset inside the window
    opt = OptimizationParams(densify_from_iter=500, lambda_dist_from_iter=1, **kw)
    if drop_attr:  # an OptimizationParams from before the term existed
        for name in ("lambda_dist", "lambda_dist_from_iter", "dist_near", "dist_far"):
            delattr(opt, name)
    g.training_setup(opt)
    t = Trainer(g, cams, gts, opt, cfg=TrainConfig(c2f=False, seed=3), scene_extent=4.4, fused=use_fused)
    assert t.fused == use_fused
    losses = [t.step(it, sync_loss=True).loss for it in range(1, steps + 1)]
    return g, losses, t


@pytest.mark.parametrize("config", list(CONFIGS))
def test_trainer_fused_matches_autograd_with_lambda_dist(gpu, config):
    kw = CONFIGS[config]
    (ga, la, _ta), (gb, lb, _tb) = _trainer(False, **kw), _trainer(True, **kw)
    for x, y in zip(la, lb):
        assert abs(x - y) <= 1e-5 * abs(y), (la, lb)
    for k, x in _params(ga).items():
        y = _params(gb)[k]
        e = rel_l1(x, y)
        print(f"\n{config}: {k} fused vs autograd rel L1 {e:.3e}")
        assert e < 1e-5, (k, e)
    # the term is in the loss and moves the positions
    off = dict(kw, lambda_dist=0.0)
    g0, l0, _t0 = _trainer(True, **off)
    assert all(a != b for a, b in zip(lb, l0))
    assert not torch.equal(gb._xyz, g0._xyz)
    assert rel_l1(gb._xyz, g0._xyz) > 1e-7


class _CallLog:
    """A loaded library behind a proxy that records the name of every entry point called."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn):
            return fn

        def call(*args):
            self._log.append(name)
            return fn(*args)

        return call


@pytest.mark.parametrize("use_fused", [True, False], ids=["fused", "autograd"])
def test_zero_lambda_dist_is_todays_step(gpu, monkeypatch, use_fused):
    """With lambda_dist = 0 two steps equal those of a Trainer whose OptimizationParams has no such
    attribute: the same native calls in the same order (none of the new entry points), bitwise the
    same first loss (the forward and the loss have no atomics), and the same parameters and Adam
    moments after two steps.  That last comparison cannot be bitwise: the blend backward's float
    atomics make two runs of the very same trainer differ in the last bits (measured on an MI355X:
    the attribute-less trainer against itself differs by up to 8.9e-10 relative L1 per parameter
    group, the lambda_dist = 0 one from it by up to 7.9e-10), so it holds at 1e-5, the bar between runs that differ only in the order of their float
    atomics, and the attribute-less trainer is run twice to show that spread beside it."""
    from rain_amd import _native as N

    raster, loss_lib = N.raster(), N.loss_lib()
    logs = []

    def run(**kw):
        log = []
        monkeypatch.setattr(N, "_raster", _CallLog(raster, log))
        monkeypatch.setattr(N, "_loss", _CallLog(loss_lib, log))
        out = _trainer(use_fused, steps=2, **kw)
        logs.append(log)
        return out

    (ga, la, _ta) = run(drop_attr=True)
    (ga2, la2, _ta2) = run(drop_attr=True)
    (gb, lb, _tb) = run(lambda_dist=0.0)
    assert logs[0] == logs[1] == logs[2] and len(logs[0]) > 4
    assert not any("dist" in name for name in logs[2])
    assert la[0] == la2[0] == lb[0]
    assert abs(lb[1] - la[1]) <= 1e-5 * abs(la[1])
    for k, x in _params(ga).items():
        spread, diff = rel_l1(_params(ga2)[k], x), rel_l1(_params(gb)[k], x)
        print(f"\n{k}: lambda_dist=0 vs no attribute {diff:.3e}; no attribute, run to run {spread:.3e}")
        assert diff <= 1e-5 and spread <= 1e-5, (k, diff, spread)
    for pa, pb in zip(ga.params(), gb.params()):
        for m in ("exp_avg", "exp_avg_sq"):
            assert rel_l1(gb.optimizer.state[pb][m], ga.optimizer.state[pa][m]) <= 1e-5, m


def test_trainer_refuses_lambda_dist_on_sharded_paths(gpu):
    for use_fused in (True, False):
        g, _l, t = _trainer(use_fused, steps=0, lambda_dist=0.1)
        t.sharded = True  # what world > 1 (or a forced exchange) sets; no ranks are started
        with pytest.raises(ValueError, match="lambda_dist > 0 needs the single-GPU step"):
            t.step(1)
