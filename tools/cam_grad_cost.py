#!/usr/bin/env python3
"""Cost of the camera-pose gradients on the bench scene (1M Gaussians, 1920x1080, SH degree 3): the
time of the per-Gaussian backward stage (RR_STAGE_GAUSS_BWD: the kernel and, with camera gradients, the
one-workgroup final pass) of the depth / alpha backward (rr_backward_aux, the baseline: its code is
unchanged) and of the camera backward (rr_backward_camera), on the same frames, one process.  HIP
events recorded by the library (rr_profile_*); the gradients are written out (no fused Adam step), so
the model does not change.  After a warm-up over every view, each view gives one sample per mode, in
alternating order; the medians are reported.

    python tools/cam_grad_cost.py [--views 24] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from rain_amd import _native, fused, synthetic
    from rain_amd.cameras import fibonacci_cameras
    from rain_amd.gaussian_model import GaussianModel

    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    cams = [c.to(dev) for c in fibonacci_cameras(200, W, H)][:a.views]
    g = GaussianModel(3, device=dev)
    g.set_params(synthetic.random_gaussians(a.points, sh_degree=3, seed=0, bench=True, device=dev))
    g.active_sh_degree = 3
    bg = torch.zeros(3, device=dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    dpix = torch.randn(3, H, W, device=dev, generator=gen) / (3 * H * W)
    dd = torch.randn(1, H, W, device=dev, generator=gen) / (H * W)
    da = torch.randn(1, H, W, device=dev, generator=gen) / (H * W)
    names = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
    params = (g._xyz, g._features_dc, g._features_rest, g._opacity, g._scaling, g._rotation)
    grads = {k: torch.empty_like(p) for k, p in zip(names, params)}
    fo = dict(dtype=torch.float32, device=dev)
    cg = (torch.empty((4, 4), **fo), torch.empty((4, 4), **fo), torch.empty((3,), **fo))
    modes = {"depth_alpha": {}, "camera": dict(cam_grads=cg)}

    def sample(c, kw, profile):
        with torch.no_grad():
            _color, _radii, _depth, st = fused.forward(g, c, bg, 0.3)
        if not profile:
            fused.backward(st, dpix, grads, dL_ddepth=dd, dL_dalpha=da, **kw)
            torch.cuda.synchronize()
            return None
        _native.Profiler.collect()
        with _native.Profiler(["gauss_bwd"]):
            fused.backward(st, dpix, grads, dL_ddepth=dd, dL_dalpha=da, **kw)
        torch.cuda.synchronize()
        ms, n = _native.Profiler.collect()["gauss_bwd"]
        return ms / max(n, 1)

    for c in cams:  # warm-up of both modes' kernels on every view
        for kw in modes.values():
            sample(c, kw, False)
    ms = {m: [] for m in modes}
    for i, c in enumerate(cams):
        order = list(modes) if i % 2 == 0 else list(modes)[::-1]
        for m in order:
            ms[m].append(sample(c, modes[m], True))
    med = {m: statistics.median(v) for m, v in ms.items()}
    out = {"scene": dict(points=a.points, width=W, height=H, sh_degree=3, views=len(cams)),
           "stage": "gauss_bwd", "samples_per_mode": len(cams),
           "median_ms": {m: round(v, 4) for m, v in med.items()},
           "min_ms": {m: round(min(v), 4) for m, v in ms.items()},
           "max_ms": {m: round(max(v), 4) for m, v in ms.items()},
           "camera_minus_depth_alpha_ms": round(med["camera"] - med["depth_alpha"], 4),
           "camera_over_depth_alpha": round(med["camera"] / med["depth_alpha"], 4)}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
