#!/usr/bin/env python3
"""Cost of the geometry loss (rain_amd/csrc/geom_loss.hip) on the bench scene (1M Gaussians,
1920x1080, SH degree 3).

1. HIP-event time of its calls on one rendered frame's depth / alpha / normal maps, beside the
   L1+SSIM loss's: rl_geom_forward (k_geom_fwd + k_geom_finalize), rl_geom_backward (k_geom_bwd),
   rl_geom_forward_backward (k_geom_fwd + k_geom_bwd, the training step's form), and
   rl_l1_ssim_forward / _backward / _forward_backward.  The bytes each call has to move (computed
   from the shapes below) over its time, against the library's streaming copy on the same device.
2. A full Trainer.step with lambda_normal = 0 and with lambda_normal > 0, alternated in windows.

    python tools/geom_loss_cost.py [--out profiles/geom_loss_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# bytes per pixel each launch has to move (fp32 maps, no gt_depth): the forward reads D, A, N and
# writes the seven workspace planes; the backward reads D, A and the seven planes (neighbours come
# from cache) and writes dD, dA, dN
FWD_BYTES = 4 * (1 + 1 + 3) + 4 * 7
BWD_BYTES = 4 * (1 + 1) + 4 * 7 + 4 * (1 + 1 + 3)


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
        out.append(1000.0 * e0.elapsed_time(e1) / reps)  # us per call
    return out


def _copy_GBps(dev):
    """read + write bytes / time of the library's float4 streaming copy (1 GiB buffers)."""
    import torch

    from rain_amd import _native

    L = _native.train_lib()
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    st = _native.stream_of(a)

    def copy():
        if L.rt_stream_copy(b.data_ptr(), a.data_ptr(), a.numel() * 4, st) != 0:
            raise RuntimeError(L.rt_last_error().decode())

    us = min(_time(copy, 10, 3))
    return 2 * (1 << 30) / (us * 1e-6) / 1e9


def main():
    import torch

    from rain_amd import fused, synthetic
    from rain_amd.cameras import fibonacci_cameras
    from rain_amd.gaussian_model import GaussianModel, OptimizationParams
    from rain_amd.loss import (geometry_loss_backward, geometry_loss_forward, geometry_loss_forward_backward,
                               l1_ssim_backward, l1_ssim_forward, l1_ssim_forward_backward)
    from rain_amd.renderer import PipelineParams, render
    from rain_amd.train import TrainConfig, Trainer

    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--steps", type=int, default=100, help="Trainer steps per timed window")
    ap.add_argument("--windows", type=int, default=3, help="timed windows per configuration")
    ap.add_argument("--lambda-normal", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("geom_loss_cost.py: no HIP device", file=sys.stderr)
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

    # 1. the launches, on one rendered frame
    g = model(0)
    with torch.no_grad():
        image, _radii, depth, st = fused.forward(g, cams[0], bg, 0.3, normal=True)
        alpha = fused.accumulated_alpha(st)
    normal = st.normal
    tx, ty = st.frame.tan_fovx, st.frame.tan_fovy
    lam = a.lambda_normal
    gloss, gparts, gws = geometry_loss_forward(depth, alpha, normal, tx, ty, lam)
    gout = (torch.empty_like(depth), torch.empty_like(alpha), torch.empty_like(normal))
    _l, _p, sws = l1_ssim_forward(image, gts[0], 0.2)
    calls = {
        "rl_geom_forward": lambda: geometry_loss_forward(depth, alpha, normal, tx, ty, lam),
        "rl_geom_backward": lambda: geometry_loss_backward(depth, alpha, normal, tx, ty, lam, 0.0, None, 0.1, gws,
                                                           out=gout),
        "rl_geom_forward_backward": lambda: geometry_loss_forward_backward(depth, alpha, normal, tx, ty, lam, out=gout),
        "rl_l1_ssim_forward": lambda: l1_ssim_forward(image, gts[0], 0.2),
        "rl_l1_ssim_backward": lambda: l1_ssim_backward(image, gts[0], 0.2, sws),
        "rl_l1_ssim_forward_backward": lambda: l1_ssim_forward_backward(image, gts[0], 0.2),
    }
    us = {}
    for rep in range(2):  # two passes over the calls: the spread between them is the noise
        for name, fn in calls.items():
            us.setdefault(name, []).extend(round(v, 2) for v in _time(fn, 50, 2))
    copy = _copy_GBps(dev)
    npix = H * W
    both = min(us["rl_geom_forward_backward"])
    out["launches"] = {
        "us_per_call": us,
        "valid_pixels": int(gparts[3].item()),
        "pixels": npix,
        "bytes_per_pixel": {"k_geom_fwd": FWD_BYTES, "k_geom_bwd": BWD_BYTES},
        "forward_backward_bytes": (FWD_BYTES + BWD_BYTES) * npix,
        "forward_backward_GBps": round((FWD_BYTES + BWD_BYTES) * npix / (both * 1e-6) / 1e9, 1),
        "backward_GBps": round(BWD_BYTES * npix / (min(us["rl_geom_backward"]) * 1e-6) / 1e9, 1),
        "measured_copy_GBps": round(copy, 1),
        "forward_backward_share_of_copy": round((FWD_BYTES + BWD_BYTES) * npix / (both * 1e-6) / 1e9 / copy, 3),
    }
    del g, st, image, depth, alpha, normal, gws, sws, gout

    # 2. the step, with and without the term (bench.py's iterations: after warm-up, before a densify)
    def trainer(lam_n):
        gm = model(0)
        opt = OptimizationParams(lambda_normal=lam_n, lambda_normal_from_iter=1)
        gm.training_setup(opt)
        return Trainer(gm, cams, gts, opt, pipe, TrainConfig(seed=0), scene_extent=extent)

    configs = {"lambda_normal_0": trainer(0.0), "lambda_normal_on": trainer(lam)}
    it = {k: 801 for k in configs}
    ms = {k: [] for k in configs}
    for k, t in configs.items():  # warm-up
        for _ in range(10):
            t.step(it[k])
            it[k] += 1
    torch.cuda.synchronize()
    for _w in range(a.windows):
        for k, t in configs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                if it[k] % 100 == 0:  # stay off the densify iterations
                    it[k] += 1
                t.step(it[k])
                it[k] += 1
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(round(e0.elapsed_time(e1) / a.steps, 4))
    out["step"] = {"ms_per_step": ms, "steps_per_window": a.steps, "lambda_normal": lam,
                   "median_delta_ms": round(statistics.median(ms["lambda_normal_on"]) -
                                            statistics.median(ms["lambda_normal_0"]), 4)}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
