#!/usr/bin/env python3
"""Cost of the depth-distortion term (rr_forward_render_dist / rr_backward_aux_dist and
rain_amd/csrc/geom_loss.hip rl_dist_*) on the bench scene (1M Gaussians, 1920x1080, SH degree 3).

1. HIP-event time of the new loss's calls on one rendered frame's alpha / moment maps:
   rl_dist_forward (k_dist_fwd + k_dist_finalize), rl_dist_backward (k_dist_bwd) and
   rl_dist_forward_backward (the training step's form), with the bytes they have to move.
2. A full Trainer.step with the term off, with lambda_dist on, with lambda_normal on and with both,
   alternated in windows.
3. The blend forward's and the blend backward's kernel time per frame in each mode (plain, depth,
   normal, moments, normal + moments) on one model and the same views, from the library's stage events.

    python tools/dist_loss_cost.py [--out profiles/dist_loss_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# bytes per pixel (fp32 maps): the forward reads A, M1, M2; the backward reads them and writes dA, dM1, dM2
FWD_BYTES = 4 * 3
BWD_BYTES = 4 * 3 + 4 * 3


def _time(fn, reps, rounds):
    import torch

    for _ in range(5):
        fn()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(round(1000.0 * e0.elapsed_time(e1) / reps, 2))  # us per call
    return out


def main():
    import torch

    from rain_amd import _native, fused, synthetic
    from rain_amd.cameras import fibonacci_cameras
    from rain_amd.gaussian_model import GaussianModel, OptimizationParams
    from rain_amd.loss import distortion_loss_backward, distortion_loss_forward, distortion_loss_forward_backward
    from rain_amd.renderer import PipelineParams, render
    from rain_amd.train import TrainConfig, Trainer

    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--steps", type=int, default=60, help="Trainer steps per timed window")
    ap.add_argument("--windows", type=int, default=3, help="timed windows per configuration")
    ap.add_argument("--lambda-dist", type=float, default=100.0)
    ap.add_argument("--lambda-normal", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("dist_loss_cost.py: no HIP device", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    cams = [c.to(dev) for c in fibonacci_cameras(200, W, H)][:a.views]
    bg = torch.zeros(3, device=dev)
    pipe = PipelineParams()
    extent = 4.0 * 1.1

    def model(seed):
        g = GaussianModel(3, divide_ratio=0.8, device=dev)
        g.set_params(synthetic.random_gaussians(a.points, sh_degree=3, seed=seed, bench=True, device=dev))
        g.active_sh_degree = 3
        g.spatial_lr_scale = extent
        return g

    gt_model = model(1)
    with torch.no_grad():
        gts = [render(c, gt_model, pipe, bg)["render"].clamp(0.0, 1.0).contiguous() for c in cams]
    del gt_model
    out = {"scene": dict(points=a.points, width=W, height=H, sh_degree=3, views=len(cams))}

    # 1. the loss's launches, on one rendered frame
    g = model(0)
    with torch.no_grad():
        _image, _radii, _depth, st = fused.forward(g, cams[0], bg, 0.3, dist=(0.2, 100.0))
        alpha = fused.accumulated_alpha(st)
    moments = st.moments
    acc = torch.zeros_like(alpha)
    calls = {
        "rl_dist_forward": lambda: distortion_loss_forward(alpha, moments, a.lambda_dist),
        "rl_dist_backward": lambda: distortion_loss_backward(alpha, moments, a.lambda_dist),
        "rl_dist_forward_backward": lambda: distortion_loss_forward_backward(alpha, moments, a.lambda_dist),
        "rl_dist_forward_backward_accumulate": lambda: distortion_loss_forward_backward(alpha, moments, a.lambda_dist,
                                                                                        d_alpha=acc),
    }
    us = {}
    for _rep in range(2):  # two passes over the calls: the spread between them is the noise
        for name, fn in calls.items():
            us.setdefault(name, []).extend(_time(fn, 50, 2))
    npix = H * W
    both = min(us["rl_dist_forward_backward"])
    out["launches"] = {
        "us_per_call": us, "pixels": npix, "bytes_per_pixel": {"k_dist_fwd": FWD_BYTES, "k_dist_bwd": BWD_BYTES},
        "forward_backward_GBps": round((FWD_BYTES + BWD_BYTES) * npix / (both * 1e-6) / 1e9, 1),
    }
    del g, st, alpha, moments, acc

    # 2. the step (bench.py's iterations: after warm-up, before a densify)
    def trainer(lam_t, lam_n):
        gm = model(0)
        opt = OptimizationParams(lambda_dist=lam_t, lambda_dist_from_iter=1, lambda_normal=lam_n,
                                 lambda_normal_from_iter=1)
        gm.training_setup(opt)
        return Trainer(gm, cams, gts, opt, pipe, TrainConfig(seed=0), scene_extent=extent)

    configs = {"off": trainer(0.0, 0.0), "lambda_dist": trainer(a.lambda_dist, 0.0),
               "lambda_normal": trainer(0.0, a.lambda_normal), "both": trainer(a.lambda_dist, a.lambda_normal)}
    it = {k: 801 for k in configs}

    def run(k, n):
        t = configs[k]
        for _ in range(n):
            if it[k] % 100 == 0:  # stay off the densify iterations
                it[k] += 1
            t.step(it[k])
            it[k] += 1

    for k in configs:  # warm-up
        run(k, 10)
    torch.cuda.synchronize()
    ms = {k: [] for k in configs}
    for _w in range(a.windows):
        for k in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(k, a.steps)
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(round(e0.elapsed_time(e1) / a.steps, 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out["step"] = {"ms_per_step": ms, "steps_per_window": a.steps, "lambda_dist": a.lambda_dist,
                   "lambda_normal": a.lambda_normal,
                   "median_delta_ms_vs_off": {k: round(med[k] - med["off"], 4) for k in configs if k != "off"}}

    del configs
    # 3. the two blends per frame in each mode, on ONE untrained model and the same views (the trainers
    # above diverge under their different losses, so their kernel times are not comparable): stage
    # events, both forward phases summed, gradients written out, random map gradients
    g = model(0)
    names = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
    params = dict(zip(names, (g._xyz, g._features_dc, g._features_rest, g._opacity, g._scaling, g._rotation)))
    grads = {k: torch.empty_like(v) for k, v in params.items()}
    gen = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda c: torch.randn((c, H, W), device=dev, generator=gen) / (H * W)  # noqa: E731
    dpix, dd, da, dn, dm = rnd(3), rnd(1), rnd(1), rnd(3), rnd(2)
    modes = {
        "plain": (dict(), dict()),
        "depth": (dict(), dict(dL_ddepth=dd, dL_dalpha=da)),
        "normal": (dict(normal=True), dict(dL_ddepth=dd, dL_dalpha=da, dL_dnormal=dn)),
        "moments": (dict(dist=(0.2, 100.0)), dict(dL_ddepth=dd, dL_dalpha=da, dL_dmoments=dm)),
        "normal+moments": (dict(normal=True, dist=(0.2, 100.0)),
                           dict(dL_ddepth=dd, dL_dalpha=da, dL_dnormal=dn, dL_dmoments=dm)),
    }
    kern = {k: {"blend_fwd": [], "blend_bwd": []} for k in modes}
    views = cams[:10]

    def frames(fkw, bkw):
        with torch.no_grad():
            for c in views:
                _img, _r, _d, st = fused.forward(g, c, bg, 0.3, **fkw)
                fused.backward(st, dpix, grads, **bkw)

    for _round in range(2):  # two rounds over the modes: the spread between them is the noise
        for k, (fkw, bkw) in modes.items():
            frames(fkw, bkw)  # warm-up
            torch.cuda.synchronize()
            _native.Profiler.collect()
            with _native.Profiler(["blend_fwd", "blend_bwd"]):
                frames(fkw, bkw)
            torch.cuda.synchronize()
            got = _native.Profiler.collect()
            for s_ in ("blend_fwd", "blend_bwd"):
                kern[k][s_].append(round(got[s_][0] / len(views), 4))
    out["kernels_ms_per_frame"] = kern
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
