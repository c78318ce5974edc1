#!/usr/bin/env python3
"""Kernel time of the two backward kernels in their three modes on the bench scene (1M Gaussians,
1920x1080, SH degree 3): plain (rr_backward), depth / alpha (rr_backward_aux) and depth / alpha /
normal (rr_backward_aux_normal).  HIP events recorded by the library (rr_profile_*), one stage
selected per loop; every frame is rendered with the aux normal map so that all three modes walk the
same lists, and the gradients are written out (no fused Adam step), so the model does not change.

    python tools/normal_cost.py [--views 10] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from rain_amd import _native, fused, synthetic
    from rain_amd.cameras import fibonacci_cameras
    from rain_amd.gaussian_model import GaussianModel

    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=10)
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
    dn = torch.randn(3, H, W, device=dev, generator=gen) / (3 * H * W)
    names = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
    params = (g._xyz, g._features_dc, g._features_rest, g._opacity, g._scaling, g._rotation)
    grads = {k: torch.empty_like(p) for k, p in zip(names, params)}
    modes = {"plain": {}, "depth_alpha": dict(dL_ddepth=dd, dL_dalpha=da),
             "depth_alpha_normal": dict(dL_ddepth=dd, dL_dalpha=da, dL_dnormal=dn)}

    def loop(kw, stage):
        for c in cams:
            with torch.no_grad():
                _color, _radii, _depth, st = fused.forward(g, c, bg, 0.3, normal=True)
            if stage is None:
                fused.backward(st, dpix, grads, **kw)
            else:
                with _native.Profiler([stage]):
                    fused.backward(st, dpix, grads, **kw)
        torch.cuda.synchronize()

    out = {"scene": dict(points=a.points, width=W, height=H, sh_degree=3, views=len(cams)), "ms_per_launch": {}}
    for rep in range(2):  # two rounds over the modes: the spread between them is the noise
        for mode, kw in modes.items():
            loop(kw, None)  # warm-up of this mode's kernels
            for stage in ("blend_bwd", "gauss_bwd"):
                _native.Profiler.collect()
                loop(kw, stage)
                ms, n = _native.Profiler.collect()[stage]
                out["ms_per_launch"].setdefault(mode, {}).setdefault(stage, []).append(round(ms / max(n, 1), 4))
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
