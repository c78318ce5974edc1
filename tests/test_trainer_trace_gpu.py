"""The fused training step's host-side decisions, pinned call by call.

Recording wrappers over rain_amd.fused.forward / forward_next / prepare_next / backward (each calls through)
log, per iteration, which forward ran with which frame options, whether the next frame was prepared, and what
the backward was handed: gradients, statistics, the fused Adam block, the next frame, absgrad and the aux map
gradients.  With StepInfo's view and densified flag (and low_pass while the schedule has read the initial
number of Gaussians only) that is the trace; tests/golden/trainer_trace.json holds it for six option sets.
num_gaussians is left out: after a densify on the GPU it depends on the order of float atomics near the
threshold.  Only Trainer's constructor, step() and fuse_next are used, so the file does not follow the
trainer's internals.  `python tests/test_trainer_trace_gpu.py [FILE]` writes the golden file (needs the GPU)."""
import inspect
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rain_amd import cameras, fused, synthetic  # noqa: E402
from rain_amd.gaussian_model import GaussianModel, OptimizationParams  # noqa: E402
from rain_amd.renderer import PipelineParams  # noqa: E402
from rain_amd.train import TrainConfig, Trainer  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_trace.json")
P, W, H, V = 2000, 64, 48, 6  # 4 x 3 tiles
MAPS = ("dL_ddepth", "dL_dalpha", "dL_dnormal", "dL_dmoments")

_EVENTS = dict(densify_from_iter=2, densification_interval=5, opacity_reset_interval=8)
_A_ITS = list(range(1, 13)) + list(range(995, 1004))
# name: (OptimizationParams fields, PipelineParams fields, fuse_next, iterations)
CASES = {
    # next-frame hand-off, a pending frame consumed and one dropped (the jump to 995), densify at 5, 10, 995
    # and 1000, reset at 8 and 1000, the SH degree stepping up at 1000
    "a_default": (_EVENTS, {}, True, _A_ITS),
    "b_normal_then_dist": (dict(lambda_normal=0.05, lambda_normal_from_iter=3, lambda_dist=0.1,
                                lambda_dist_from_iter=5), {}, True, list(range(1, 8))),
    "c_antialias_absgrad": (dict(densify_absgrad=True, densify_until_iter=3), dict(antialiasing=True), True,
                            list(range(1, 5))),
    "d_importance_prune": (dict(importance_prune_iterations=(3,), importance_prune_fraction=0.3), {}, True,
                           list(range(1, 6))),
    # events at 3 and 6
    "e_mcmc": (dict(densify_strategy="mcmc", cap_max=2200, densify_from_iter=1, densification_interval=3), {}, True,
               list(range(1, 8))),
    "f_default_no_fuse_next": (_EVENTS, {}, False, _A_ITS),
}

_SCENE = {}


def _scene():
    if not _SCENE:
        _SCENE["cams"] = [c.to("cuda") for c in cameras.fibonacci_cameras(V, W, H)]
        _SCENE["gts"] = [torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(40 + i))
                         for i in range(V)]
    return _SCENE["cams"], _SCENE["gts"]


def _summary(name, a):
    if name == "forward":
        return dict(normal=bool(a["normal"]), dist=None if a["dist"] is None else list(a["dist"]),
                    antialiasing=bool(a["antialiasing"]))
    if name == "prepare_next":
        return dict(antialiasing=bool(a["antialiasing"]))
    if name == "backward":
        return dict(grads=a["grads"] is not None, stats=a["stats"] is not None, adam=a["adam"] is not None,
                    next_frame=a["next_frame"] is not None, absgrad=bool(a["absgrad"]),
                    maps=[m for m in MAPS if a[m] is not None])
    return {}


def _trace(case, patch):
    """Run one case and return its trace; `patch` is a pytest.MonkeyPatch."""
    opt_kw, pipe_kw, fuse_next, its = CASES[case]
    calls = []
    for name in ("forward", "forward_next", "prepare_next", "backward"):
        real = getattr(fused, name)

        def wrapper(*args, _name=name, _real=real, _sig=inspect.signature(real), **kw):
            bound = _sig.bind(*args, **kw)
            bound.apply_defaults()
            calls.append([_name, _summary(_name, bound.arguments)])
            return _real(*args, **kw)

        patch.setattr(fused, name, wrapper)
    cams, gts = _scene()
    g = GaussianModel(3, divide_ratio=0.8, device="cuda")
    g.set_params(synthetic.random_gaussians(P, sh_degree=3, seed=2, bench=True))
    g.active_sh_degree = 1
    g.spatial_lr_scale = 4.4
    opt = OptimizationParams(**opt_kw)
    g.training_setup(opt)
    cfg = TrainConfig(seed=3)
    t = Trainer(g, cams, gts, opt, PipelineParams(**pipe_kw), cfg=cfg, scene_extent=4.4, fused=True)
    t.fuse_next = fuse_next
    trace = []
    for it in its:
        del calls[:]
        info = t.step(it)
        row = dict(it=it, calls=list(calls), view=info.view, densified=bool(info.densified))
        if it < cfg.c2f_every_step:  # from there on the schedule has read a densified model's size
            row["low_pass"] = info.low_pass
        trace.append(row)
    torch.cuda.synchronize()
    return json.loads(json.dumps(trace))


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_step_decisions(gpu, monkeypatch, case):
    with open(GOLDEN) as f:
        golden = json.load(f)[case]
    trace = _trace(case, monkeypatch)
    assert len(trace) == len(golden)
    for got, want in zip(trace, golden):
        assert got == want, f"{case}, iteration {want['it']}: got {got}, golden {want}"


if __name__ == "__main__":
    out = {}
    for name in sorted(CASES):
        with pytest.MonkeyPatch.context() as mp:
            out[name] = _trace(name, mp)
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": [\n' + ",\n".join("  " + json.dumps(r) for r in v) + "\n ]"
                                  for k, v in out.items()) + "\n}\n")
