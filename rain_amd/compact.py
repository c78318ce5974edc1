"""Compaction of a trained model by blend-contribution importance (rain_amd.importance).

    python -m rain_amd.compact --ply in.ply --out out.ply --fraction 0.6 [--kind weight_volume]
        [--num_cams 32 --width 800 --height 800 --radius 4.0] [--antialiasing]

Scores every Gaussian over synthetic Fibonacci-sphere cameras (rain_amd.cameras, as
rain_amd.render_views; the function API of rain_amd.importance takes any camera list), removes the
lowest-scoring `--fraction` (or every score below `--threshold`) and writes the rest with rain_amd.ply.
"""
from __future__ import annotations

import argparse

import torch


def main(argv=None):
    from . import importance
    from .cameras import fibonacci_cameras
    from .gaussian_model import GaussianModel, OptimizationParams
    from .renderer import PipelineParams

    ap = argparse.ArgumentParser(description="prune a trained model by per-Gaussian blend contributions")
    ap.add_argument("--ply", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--fraction", type=float, default=None, help="share of the Gaussians to remove")
    ap.add_argument("--threshold", type=float, default=None, help="remove every score below this")
    ap.add_argument("--kind", choices=importance.KINDS, default="weight_volume")
    ap.add_argument("--sh_degree", type=int, default=3)
    ap.add_argument("--num_cams", type=int, default=32)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--radius", type=float, default=4.0)
    ap.add_argument("--white_background", action="store_true")
    ap.add_argument("--antialiasing", action="store_true",
                    help="score the anti-aliased render (PipelineParams.antialiasing)")
    a = ap.parse_args(argv)
    if (a.fraction is None) == (a.threshold is None):
        ap.error("give exactly one of --fraction / --threshold")
    dev = torch.device("cuda", torch.cuda.current_device())
    g = GaussianModel(a.sh_degree, device=dev)
    g.load_ply(a.ply)
    g.training_setup(OptimizationParams())  # prune_points goes through the optimizer's parameter groups
    bg = torch.tensor([1.0, 1.0, 1.0] if a.white_background else [0.0, 0.0, 0.0], device=dev)
    cams = [c.to(dev) for c in fibonacci_cameras(a.num_cams, a.width, a.height, radius=a.radius)]
    before = g.get_xyz.shape[0]
    stats = importance.accumulate_contributions(g, cams, PipelineParams(antialiasing=a.antialiasing), bg)
    scores = importance.importance_scores(stats, g, kind=a.kind)
    g.prune_by_importance(scores, fraction=a.fraction, threshold=a.threshold)
    g.save_ply(a.out)
    print(f"compact: {before} -> {g.get_xyz.shape[0]} Gaussians ({a.kind}, {stats.views_seen} views) -> {a.out}")


if __name__ == "__main__":
    main()
