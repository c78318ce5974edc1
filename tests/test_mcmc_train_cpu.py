"""The MCMC training loop (Trainer._step_mcmc, rain_amd/mcmc.py's torch path) on CPU tensors, with the CPU
oracle as the rasterizer (tests/oracle_c.py, monkeypatched in for the HIP `_C`, as in tests/test_train_cpu.py)."""
import pytest
import torch

import rain_amd.diff_gaussian_rasterization as dgr
from oracle.loss_ref import l1_loss, ssim
from rain_amd import cameras, mcmc, synthetic
from rain_amd.gaussian_model import GaussianModel, OptimizationParams, inverse_sigmoid
from rain_amd.renderer import PipelineParams
from rain_amd.train import TrainConfig, Trainer
from tests import oracle_c

P0, CAP, ITERS = 300, 340, 12
MIN_OPACITY = 0.005
# relocation clamps a copy's opacity at exactly min_opacity and stores its logit in fp32; the logit's
# rounding (half an ulp of 5.3, 2.4e-7) moves the opacity read back by 2.4e-7 * (1 - 0.005) relative, and the
# fp32 sigmoid adds a few ulps (6e-8 each): "not dead" is checked with that allowance, 1e-6 relative
ROUND_TRIP = 1e-6


def _ref_loss(img, gt, lam):
    return (1.0 - lam) * l1_loss(img, gt) + lam * (1.0 - ssim(img, gt))


@pytest.fixture
def cpu_rasterizer(monkeypatch, oracle):
    monkeypatch.setattr(dgr, "_C", oracle_c)
    return oracle_c


def mcmc_opt():
    return OptimizationParams(densify_strategy="mcmc", cap_max=CAP, densify_from_iter=2, densification_interval=3,
                              iterations=30_000)


def make_model(device="cpu"):
    g = GaussianModel(1, divide_ratio=0.8, device=device)
    prm = synthetic.random_gaussians(P0, sh_degree=1, seed=0, bench=True)
    gen = torch.Generator().manual_seed(7)
    low = torch.rand(40, 1, generator=gen) * 0.004 + 0.0005  # 40 rows start dead: opacity in [0.0005, 0.0045]
    prm["opacity"] = prm["opacity"].clone()
    prm["opacity"][torch.arange(40) * 7] = inverse_sigmoid(low)
    g.set_params(prm)
    g.active_sh_degree = 1
    g.spatial_lr_scale = 4.4
    return g


def dead_rows(g):
    return int((torch.sigmoid(g._opacity.detach()) < MIN_OPACITY * (1.0 - ROUND_TRIP)).sum())


def step_counts(g):
    return [float(g.optimizer.state[p]["step"]) if len(g.optimizer.state.get(p, {})) else 0.0 for p in g.params()]


def run_schedule(g, tr):
    """ITERS iterations; returns per iteration (P, densified, dead rows after the step, step counts)."""
    log = []
    for it in range(1, ITERS + 1):
        before = g.get_xyz.shape[0]
        info = tr.step(it)
        P = g.get_xyz.shape[0]
        assert info.num_gaussians == P
        log.append((before, P, info.densified, dead_rows(g), step_counts(g)))
    return log


def check_schedule(g, log):
    events = [it for it in range(1, ITERS + 1) if 2 < it and it % 3 == 0]
    assert [it for it, row in enumerate(log, 1) if row[2]] == events == [3, 6, 9, 12]
    counts = [0.0] * 6
    for it, (before, P, densified, dead, steps) in enumerate(log, 1):
        assert P <= CAP
        if densified:
            assert before <= P <= int(1.05 * before) and P == min(CAP, int(1.05 * before))
            assert dead == 0, f"iteration {it}: {dead} dead rows right after the event"
        else:
            assert P == before
            counts = [c + 1.0 for c in counts]
        assert steps == counts, f"iteration {it}: step counts {steps}"  # no Adam step on an event iteration
    assert log[0][3] > 0  # the scene starts with dead rows (iteration 1 is no event)
    assert log[-1][1] == CAP  # 300 -> 315 -> 330 -> 340
    for p in g.params():
        assert p.shape[0] == CAP and bool(torch.isfinite(p).all())
        st = g.optimizer.state[p]
        assert st["exp_avg"].shape == p.shape and bool(torch.isfinite(st["exp_avg"]).all())
        assert bool(torch.isfinite(st["exp_avg_sq"]).all())
    assert g.xyz_gradient_accum.shape == (CAP, 1) and g.max_radii2D.shape == (CAP,)


def scene(n=3, W=48, H=40):
    cams = cameras.fibonacci_cameras(n, W, H)
    gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(10 + i)) for i in range(n)]
    return cams, gts


def _run():
    cams, gts = scene()
    g = make_model()
    opt = mcmc_opt()
    g.training_setup(opt)
    tr = Trainer(g, cams, gts, opt, PipelineParams(), TrainConfig(c2f=False, seed=5), scene_extent=4.4,
                 loss_fn=_ref_loss)
    return g, run_schedule(g, tr)


def test_mcmc_schedule_growth_cap_and_step_counts(cpu_rasterizer):
    g, log = _run()
    check_schedule(g, log)
    # same seeds, same run: parameters, moments and sizes are identical
    g2, log2 = _run()
    assert [r[:4] for r in log] == [r[:4] for r in log2]
    for p, q in zip(g.params(), g2.params()):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(g.optimizer.state[p]["exp_avg"], g2.optimizer.state[q]["exp_avg"])


def test_relocate_and_add_new_on_a_cpu_model():
    g = make_model()
    g.training_setup(mcmc_opt())
    for p in g.params():  # non-zero moments, as after some training
        g.optimizer.state[p]["step"] = torch.tensor(3.0)
        g.optimizer.state[p]["exp_avg"] = torch.full_like(p, 0.5)
        g.optimizer.state[p]["exp_avg_sq"] = torch.full_like(p, 0.25)
    before = {n: p.detach().clone() for n, p in zip("xyz f_dc f_rest opacity scaling rotation".split(), g.params())}
    dead = torch.sigmoid(before["opacity"]).reshape(-1) <= MIN_OPACITY
    gen = torch.Generator().manual_seed(3)
    assert g.relocate_gs(generator=gen) == int(dead.sum()) == 40
    assert dead_rows(g) == 0
    # a relocated row sits where its source sits; rows that took no part are bitwise unchanged
    xyz = g._xyz.detach()
    moved = (xyz != before["xyz"]).any(dim=1)
    assert bool((~moved | dead).all()) and int(moved.sum()) > 0
    zeroed = (g.optimizer.state[g._xyz]["exp_avg"] == 0).all(dim=1)
    assert bool(zeroed[dead].all()) and 40 < int(zeroed.sum()) <= 80  # the destinations and their sources
    untouched = ~zeroed
    for n, p in zip(before, g.params()):
        assert torch.equal(p.detach()[untouched], before[n][untouched]), n
        assert bool((g.optimizer.state[p]["exp_avg_sq"][untouched] == 0.25).all())
    # only a copy clamped at min_opacity can read back as dead again (ROUND_TRIP above)
    again = int((torch.sigmoid(g._opacity.detach()) <= MIN_OPACITY).sum())
    assert g.relocate_gs(generator=gen) == again and again <= 80
    assert g.add_new_gs(CAP, generator=gen) == 15 and g.get_xyz.shape[0] == 315
    assert g.add_new_gs(316, generator=gen) == 1 and g.add_new_gs(316, generator=gen) == 0
    assert bool((g.optimizer.state[g._scaling]["exp_avg"][300:] == 0).all())
    assert mcmc.add_new(g, 10, generator=gen) == 0  # a cap below the current size adds nothing
