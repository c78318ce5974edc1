"""Per-Gaussian blend-contribution statistics (rr_contributions) and importance pruning on the GPU.

The reference is tests/contrib_ref.py, a numpy walk of the oracle's forward state pinned against the
oracle's own backward by tests/test_contrib_ref_cpu.py.  Bars: the project's parity bar of 1e-4 relative
L1 against the reference, 1e-5 between GPU results that differ only in the order of their float atomics
or in the float evaluation of the same sums; max_w and count are integer atomics and compared bitwise."""
import ctypes
import math

import numpy as np
import pytest
import torch

from rain_amd import _native as N
from rain_amd import cameras, importance, synthetic
from rain_amd.gaussian_model import GaussianModel, OptimizationParams
from rain_amd.renderer import PipelineParams
from rain_amd.train import TrainConfig, Trainer
from tests.common import make_scene, oracle_run, rel_l1
from tests.contrib_ref import contributions_ref, precomp_scene
# the depth file's scenes, binning fixture (default, and early-stop split 2) and helpers
from tests.test_depth_grad_gpu import (SCENES, _assert_multi_round, _backward_args, _forward, _gpu_inputs,  # noqa: F401
                                       _settings, binning)

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(oracle, name):
    """Per scene, computed once and left unchanged: the inputs, a seeded pixel-weight map of both signs,
    and the reference statistics of the oracle's frame."""
    if name not in _REF:
        inp, st = make_scene(**SCENES[name])
        H, W = st["image_height"], st["image_width"]
        g = np.random.default_rng(17).standard_normal((H, W)).astype(np.float32)
        run = oracle_run(oracle, inp, st)
        _REF[name] = dict(inp=inp, st=st, g=g, radii=run["radii"],
                          stats=contributions_ref(run["state"].internals(), W, H, g))
    return _REF[name]


def _stats(fw, P, W, H, g=None, out=None):
    from rain_amd.diff_gaussian_rasterization import _C

    nr, _c, radii, _d, geom, binb, img = fw
    return _C.gaussian_contributions(radii, geom, binb, img, nr, P, W, H, pixel_weight=g, out=out)


def _np(stats):
    return [t.cpu().numpy() for t in stats]


def _frame_of(ref, dev, inp=None):
    d, s = _gpu_inputs(inp or ref["inp"], ref["st"], dev)
    P, H, W = d["means3D"].shape[0], s["image_height"], s["image_width"]
    return d, s, P, W, H


@pytest.mark.parametrize("scene", list(SCENES))
def test_parity_and_exact_zeros(oracle, gpu, binning, scene):
    ref = _reference(oracle, scene)
    d, s, P, W, H = _frame_of(ref, gpu)
    fw = _forward(d, s)
    _assert_multi_round(fw, P, W, H)
    g = torch.from_numpy(ref["g"]).to(gpu)
    stats = _stats(fw, P, W, H, g)
    sum_w, sum_gw, max_w, count = _np(stats)
    assert count.dtype == np.int32 and all(a.shape == (P,) for a in (sum_w, sum_gw, max_w, count))
    r = ref["stats"]
    errs = dict(sum_w=rel_l1(sum_w, r["sum_w"]), sum_gw=rel_l1(sum_gw, r["sum_gw"]), max_w=rel_l1(max_w, r["max_w"]),
                count=rel_l1(count.astype(np.float64), r["count"].astype(np.float64)))
    radii = fw[2].cpu().numpy()
    vis = radii > 0
    assert np.array_equal(vis, ref["radii"] > 0)
    print(f"\n{scene}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) +
          f"; {int((vis & (count == 0)).sum())} of {int(vis.sum())} visible Gaussians have count == 0"
          f" (reference: {int((vis & (r['count'] == 0)).sum())})")
    for k, v in errs.items():
        assert v < 1e-4, (k, v)
    # every record of an invisible Gaussian is exactly zero, bit for bit
    raw = stats[0]._base  # the four are views of one [P,4] buffer
    assert raw is not None and tuple(raw.shape) == (P, 4)
    bits = raw.view(torch.int32).cpu().numpy()
    assert not bits[~vis].any()
    assert (max_w >= 0).all() and max_w.max() <= 0.99 and (count >= 0).all()
    assert np.array_equal(count > 0, max_w > 0) and np.array_equal(count > 0, sum_w > 0)
    # without a map g == 1: sum_gw is sum_w (up to the order of the atomics), the rest is unchanged
    one = _np(_stats(fw, P, W, H))
    assert rel_l1(one[1], one[0]) < 1e-5 and rel_l1(one[0], sum_w) < 1e-5
    assert np.array_equal(one[2], max_w) and np.array_equal(one[3], count)


@pytest.mark.parametrize("scene", list(SCENES))
def test_gpu_against_its_own_backward_and_alpha_map(oracle, gpu, binning, scene):
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    ref = _reference(oracle, scene)
    inp = ref["inp"] if "colors_precomp" in ref["inp"] else precomp_scene(ref["inp"])
    d, s, P, W, H = _frame_of(ref, gpu, inp)
    fw = _forward(d, s)
    _assert_multi_round(fw, P, W, H)
    g = torch.from_numpy(ref["g"]).to(gpu)
    sum_w, sum_gw, _m, _c = _stats(fw, P, W, H, g)
    dpix = g.reshape(1, H, W).repeat(3, 1, 1).contiguous()
    grads = _C.rasterize_gaussians_backward(*_backward_args(d, s, fw, dpix))
    d_colors = grads[1]
    for ch in range(3):
        e = rel_l1(sum_gw.cpu().numpy(), d_colors[:, ch].cpu().numpy())
        print(f"\n{scene}: sum_gw vs dL_dcolors[:, {ch}] {e:.3e}")
        assert e < 1e-5
    with torch.no_grad():
        _col, _rad, _dep, alpha = GaussianRasterizer(_settings(s)).forward_depth(
            d["means3D"], torch.zeros_like(d["means3D"]), d["opacities"], shs=None,
            colors_precomp=d["colors_precomp"], scales=d.get("scales"), rotations=d.get("rotations"),
            cov3D_precomp=d.get("cov3D_precomp"))
    total, a_total = float(sum_w.double().sum()), float(alpha.double().sum())
    print(f"{scene}: sum of sum_w {total:.6f} vs summed alpha map {a_total:.6f}")
    assert abs(total - a_total) < 1e-5 * a_total


@pytest.mark.parametrize("scene", list(SCENES))
def test_determinism_and_phase_independence(oracle, gpu, scene):
    ref = _reference(oracle, scene)
    d, s, P, W, H = _frame_of(ref, gpu)
    g = torch.from_numpy(ref["g"]).to(gpu)
    runs = []
    try:
        for split in (0, 0, 2):
            N.check(N.raster().rr_set_binning_config(split, 1 if split else 0), "binning config")
            fw = _forward(d, s)
            _assert_multi_round(fw, P, W, H)
            runs.append(_np(_stats(fw, P, W, H, g)))
    finally:
        N.check(N.raster().rr_set_binning_config(0, 0), "binning config")
    base = runs[0]
    for other, what in ((runs[1], "second run"), (runs[2], "early-stop split 2")):
        assert np.array_equal(other[2].view(np.int32), base[2].view(np.int32)), f"max_w differs: {what}"
        assert np.array_equal(other[3], base[3]), f"count differs: {what}"
        for k in (0, 1):
            assert rel_l1(other[k], base[k]) < 1e-5, (k, what)


def test_accumulate_two_cameras_and_poisoned_buffer(oracle, gpu, binning):
    from rain_amd.diff_gaussian_rasterization import _C

    frames = []
    for cam_index in (0, 3):
        inp, st = make_scene(**dict(SCENES["sh3"], cam_index=cam_index))
        d, s = _gpu_inputs(inp, st, gpu)
        frames.append((d, s))
    P, H, W = frames[0][0]["means3D"].shape[0], frames[0][1]["image_height"], frames[0][1]["image_width"]
    g = torch.from_numpy(np.random.default_rng(5).standard_normal((H, W)).astype(np.float32)).to(gpu)
    fws = [_forward(d, s) for d, s in frames]
    _assert_multi_round(fws[0], P, W, H)
    single = [[t.clone() for t in _stats(fw, P, W, H, g)] for fw in fws]
    assert not torch.equal(single[0][3], single[1][3])  # two different views
    buf = torch.zeros((P, 4), dtype=torch.float32, device=gpu)
    for fw in fws:
        acc = _stats(fw, P, W, H, g, out=buf)
    assert acc[0]._base is buf
    assert torch.equal(acc[3], single[0][3] + single[1][3])
    assert torch.equal(acc[2], torch.maximum(single[0][2], single[1][2]))
    for k in (0, 1):
        assert rel_l1(acc[k].cpu().numpy(), (single[0][k].double() + single[1][k].double()).cpu().numpy()) < 1e-5
    # accumulate == 0 writes every record: a buffer full of NaN bits comes back as the single-view result
    nr, _c, radii, _d, geom, binb, img = fws[0]
    poison = torch.full((P, 4), float("nan"), dtype=torch.float32, device=gpu)
    poison.view(torch.int32).fill_(-1)
    frame = _C._frame(P, 0, 0, W, H, 1.0, 1.0, 1.0, 0.3, False, False)
    N.check(N.raster().rr_contributions(ctypes.byref(frame), _C._ptr(radii), _C._ptr(geom), _C._ptr(img),
                                        _C._ptr(binb), int(nr), _C._ptr(g), 0, _C._ptr(poison), N.stream_of(radii)),
            "rr_contributions")
    assert torch.equal(poison[:, 2], single[0][2]) and torch.equal(poison.view(torch.int32)[:, 3], single[0][3])
    assert bool(torch.isfinite(poison[:, :3]).all())
    for k in (0, 1):
        assert rel_l1(poison[:, k].cpu().numpy(), single[0][k].cpu().numpy()) < 1e-5


def test_no_gaussians(gpu):
    from rain_amd.diff_gaussian_rasterization import GaussianRasterizer, _C

    inp, st = make_scene(P=10, W=64, H=48, sh_degree=1)
    d, s = _gpu_inputs({k: v[:0] for k, v in inp.items()}, st, gpu)
    fw = _forward(d, s)
    stats = _stats(fw, 0, 64, 48)
    assert [tuple(t.shape) for t in stats] == [(0,)] * 4 and stats[3].dtype == torch.int32
    color, radii, stats = GaussianRasterizer(_settings(s)).contributions(
        d["means3D"], d["opacities"], shs=d["shs"], scales=d["scales"], rotations=d["rotations"])
    assert tuple(color.shape) == (3, 48, 64) and radii.numel() == 0 and all(t.numel() == 0 for t in stats)
    # a frame with Gaussians but none in view: every record zero, nothing walked
    behind = dict(inp, means3D=3.0 * st["campos"][None, :] + 0.01 * inp["means3D"])  # the camera looks at the origin
    d, s = _gpu_inputs(behind, st, gpu)
    fw = _forward(d, s)
    assert fw[0] == 0
    stats = _stats(fw, 10, 64, 48)
    assert all(not bool(t.any()) for t in stats)


def _walled_model(P=2000, seed=4):
    """A random model whose Gaussian 0 sits at the origin inside a closed shell of large opaque splats
    (rows 1..700): no camera outside the shell sees it."""
    p = synthetic.random_gaussians(P, sh_degree=1, seed=seed, bench=True)
    gen = torch.Generator().manual_seed(seed)
    n_wall = 700
    v = torch.randn(n_wall, 3, generator=gen)
    p["xyz"][1:1 + n_wall] = 0.3 * v / v.norm(dim=1, keepdim=True)
    p["scaling"][1:1 + n_wall] = math.log(0.08)
    p["opacity"][1:1 + n_wall] = 8.0
    p["xyz"][0] = 0.0
    p["scaling"][0] = math.log(0.02)
    p["opacity"][0] = 2.0
    g = GaussianModel(1, divide_ratio=0.8, device="cuda")
    g.set_params(p)
    g.active_sh_degree = 1
    g.spatial_lr_scale = 4.4
    return g


def _trainer(g, opt, use_fused=True, V=4, W=128, H=96):
    cams = [c.to("cuda") for c in cameras.fibonacci_cameras(V, W, H)]
    gts = [torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(10 + i)) for i in range(V)]
    g.training_setup(opt)
    return Trainer(g, cams, gts, opt, cfg=TrainConfig(c2f=False, seed=3), scene_extent=4.4, fused=use_fused)


def _rows(g):
    tensors = dict(xyz=g._xyz, f_dc=g._features_dc, f_rest=g._features_rest, opacity=g._opacity, scaling=g._scaling,
                   rotation=g._rotation, grad_accum=g.xyz_gradient_accum, denom=g.denom, max_radii2D=g.max_radii2D)
    for group in g.optimizer.param_groups:
        state = g.optimizer.state[group["params"][0]]
        tensors["exp_avg_" + group["name"]] = state["exp_avg"]
        tensors["exp_avg_sq_" + group["name"]] = state["exp_avg_sq"]
    return tensors


def test_importance_scores_and_pruning(gpu):
    g = _walled_model()
    P = g.get_xyz.shape[0]
    opt = OptimizationParams(densify_from_iter=500)
    t = _trainer(g, opt)
    assert math.isfinite(t.step(1, sync_loss=True).loss)  # Adam moments and densification statistics exist
    bg = torch.zeros(3, device=gpu)
    stats = importance.accumulate_contributions(g, t.cams, PipelineParams(), bg)
    assert stats.views_seen == 4 and tuple(stats.buffer.shape) == (P, 4)
    assert int(stats.count[0]) == 0 and float(stats.sum_w[0]) == 0.0  # the walled-in Gaussian is never blended
    assert int((stats.count > 0).sum()) > P // 4
    scores = {}
    for kind in importance.KINDS:
        sc = importance.importance_scores(stats, g, kind=kind)
        assert tuple(sc.shape) == (P,) and sc.dtype == torch.float32 and bool(torch.isfinite(sc).all()), kind
        scores[kind] = sc
    assert float(scores["weight_volume"].max()) > 0 and bool((scores["weight_volume"] <= scores["weight"]).all())
    # a weighted accumulation: a mask that keeps the left half of every image
    half = importance.accumulate_contributions(
        g, t.cams, PipelineParams(), bg,
        pixel_weight_fn=lambda view, image: (torch.arange(image.shape[2], device=image.device) < image.shape[2] // 2)
        .float().expand(image.shape[1], image.shape[2]))
    assert torch.equal(half.count, stats.count) and torch.equal(half.max_w, stats.max_w)
    assert bool((half.sum_gw <= half.sum_w * (1 + 1e-5) + 1e-7).all()) and float(half.sum_gw.sum()) < \
        0.9 * float(half.sum_w.sum())
    before = {k: v.detach().clone() for k, v in _rows(g).items()}
    assert len(before) == 9 + 12
    mask = g.prune_by_importance(scores["weight_volume"], fraction=0.5)
    keep = P - (P // 2)
    assert int(mask.sum()) == P // 2 and bool(mask[0]), "the walled-in Gaussian must be among the pruned"
    after = _rows(g)
    for k, v in after.items():
        assert v.shape[0] == keep, (k, tuple(v.shape))
        assert torch.equal(v.detach(), before[k][~mask]), k
    info = t.step(2, sync_loss=True)
    assert math.isfinite(info.loss) and info.num_gaussians == keep
    # threshold form: everything that is never blended goes
    g2 = _walled_model()
    g2.training_setup(opt)
    st2 = importance.accumulate_contributions(g2, t.cams, PipelineParams(), bg)
    dead = int((st2.count == 0).sum())
    m2 = g2.prune_by_importance(importance.importance_scores(st2, g2, "count"), threshold=0.5)
    assert int(m2.sum()) == dead and g2.get_xyz.shape[0] == P - dead and bool(m2[0])


@pytest.mark.parametrize("use_fused", [True, False], ids=["fused", "autograd"])
def test_training_hook(gpu, monkeypatch, use_fused):
    calls = []
    real = importance.accumulate_contributions

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(importance, "accumulate_contributions", counted)
    P = 2000

    def run(**kw):
        g = GaussianModel(1, divide_ratio=0.8, device="cuda")
        g.set_params(synthetic.random_gaussians(P, sh_degree=1, seed=2, bench=True))
        g.spatial_lr_scale = 4.4
        t = _trainer(g, OptimizationParams(densify_from_iter=500, **kw), use_fused=use_fused)
        assert t.fused == use_fused
        out = []
        for it in range(1, 13):
            info = t.step(it, sync_loss=True)
            out.append((info.loss, info.num_gaussians, g.get_xyz.shape[0]))
        return out

    pruned = run(importance_prune_iterations=(6,), importance_prune_fraction=0.3)
    assert len(calls) == 1
    keep = P - int(0.3 * P)
    assert [n for _l, n, _r in pruned] == [P] * 5 + [keep] * 7 and [r for _l, _n, r in pruned] == [P] * 5 + [keep] * 7
    assert all(math.isfinite(l) for l, _n, _r in pruned)
    del calls[:]
    plain = run()
    assert not calls, "the default parameters must never enter the importance path"
    assert [n for _l, n, _r in plain] == [P] * 12 and all(math.isfinite(l) for l, _n, _r in plain)
    # the same first step (no atomics in the forward or the loss)
    assert plain[0][0] == pruned[0][0]


def test_compact_cli(gpu, tmp_path):
    """python -m rain_amd.compact, in process: a .ply in, the lowest-scoring 60 % removed, a .ply out."""
    from rain_amd import compact

    g = _walled_model()
    P = g.get_xyz.shape[0]
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    g.save_ply(src)
    compact.main(["--ply", src, "--out", dst, "--fraction", "0.6", "--kind", "max_weight", "--sh_degree", "1",
                  "--num_cams", "4", "--width", "128", "--height", "96"])
    out = GaussianModel(1, device="cuda")
    out.load_ply(dst)
    assert out.get_xyz.shape[0] == P - int(0.6 * P)
    # the kept rows are rows of the input, in order, and the walled-in Gaussian (at the origin) is not one of them
    kept = out._xyz.detach()
    assert not bool((kept.abs().sum(dim=1) == 0).any())
    match = (g._xyz.detach()[:, None, :] == kept[None, :, :]).all(dim=2)
    idx = match.float().argmax(dim=0)
    assert bool(match.any(dim=0).all()) and bool((idx[1:] > idx[:-1]).all())
    assert torch.equal(out._opacity.detach(), g._opacity.detach()[idx])
