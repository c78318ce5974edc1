"""Per-Gaussian importance from blend contributions, for compaction (no reference counterpart).

How much each Gaussian is used: over a set of views, the rasterizer's statistics kernel
(include/rain_raster.h rr_contributions) accumulates for every Gaussian i its blend weight
w_i(p) = alpha_i(p) T_i(p) over the pixels it was blended into: the sum, a weighted sum, the maximum
and the hit count.  From these:

* ``weight_volume``  LightGaussian's global significance: sum_gw * clamp(V / V_q90, 0, 1) ** volume_power,
                     V = prod(scales);
* ``weight``         sum_gw alone (with a pixel_weight_fn: error- or mask-weighted use);
* ``max_weight``     max_p w_i, the RadSplat / Mini-Splatting criterion;
* ``count``          pixels hit, the dead-splat test.

``prune_mask`` turns scores into the rows to remove, ``GaussianModel.prune_by_importance`` removes them,
``python -m rain_amd.compact`` does both for a .ply, and OptimizationParams.importance_prune_iterations
does it inside the single-GPU training loop.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from .diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer

KINDS = ("weight_volume", "weight", "max_weight", "count")


@dataclass
class ContributionStats:
    """Statistics accumulated over `views_seen` views; `buffer` is the [P,4] float32 array of rr_contrib
    records (count through its bits)."""
    buffer: torch.Tensor
    views_seen: int = 0

    @property
    def sum_w(self):
        return self.buffer[:, 0]

    @property
    def sum_gw(self):
        return self.buffer[:, 1]

    @property
    def max_w(self):
        return self.buffer[:, 2]

    @property
    def count(self):
        return self.buffer.view(torch.int32)[:, 3]


@torch.no_grad()
def accumulate_contributions(gaussians, views, pipe, background, pixel_weight_fn=None, low_pass=0.3):
    """One render plus one statistics launch per view, all into one buffer.  pixel_weight_fn(view, image)
    -> [H,W] (optional) weights the pixels of sum_gw, e.g. a per-pixel error map or a mask; without it
    sum_gw is sum_w.  pipe.antialiasing is honoured."""
    P = gaussians.get_xyz.shape[0]
    buf = torch.zeros((P, 4), dtype=torch.float32, device=gaussians.get_xyz.device)
    stats = ContributionStats(buf, 0)
    means3D, opacity, shs = gaussians.get_xyz, gaussians.get_opacity, gaussians.get_features
    scales = rotations = cov3D = None
    if pipe is not None and pipe.compute_cov3D_python:
        cov3D = gaussians.get_covariance(1.0)
    else:
        scales, rotations = gaussians.get_scaling, gaussians.get_rotation
    for view in views:
        settings = GaussianRasterizationSettings(
            image_height=int(view.image_height), image_width=int(view.image_width),
            tanfovx=math.tan(view.FoVx * 0.5), tanfovy=math.tan(view.FoVy * 0.5), bg=background, scale_modifier=1.0,
            viewmatrix=view.world_view_transform, projmatrix=view.full_proj_transform,
            sh_degree=gaussians.active_sh_degree, campos=view.camera_center, prefiltered=False,
            debug=bool(pipe is not None and pipe.debug), low_pass=low_pass)
        # pipe.antialiasing: the statistics are then those of the anti-aliased render (rr_contributions reads
        # the splat records, which hold the compensated opacities)
        r = GaussianRasterizer(settings, antialiasing=bool(getattr(pipe, "antialiasing", False)))
        kw = dict(shs=shs, scales=scales, rotations=rotations, cov3D_precomp=cov3D)
        if pixel_weight_fn is None:
            r.contributions(means3D, opacity, out=buf, **kw)
        else:
            # the weights may depend on the rendered image: render, then the statistics of that frame
            from .diff_gaussian_rasterization import _C, _absent_as_empty, _forward_args

            sh_, col_, sc_, rot_, cov_ = _absent_as_empty(shs, None, scales, rotations, cov3D)
            nr, color, radii, _d, geom, binning, img = _C.rasterize_gaussians(
                *_forward_args(settings, means3D, col_, opacity, sc_, rot_, cov_, sh_))
            g = pixel_weight_fn(view, color)
            _C.gaussian_contributions(radii, geom, binning, img, nr, P, settings.image_width, settings.image_height,
                                      pixel_weight=g.to(torch.float32), out=buf)
        stats.views_seen += 1
    return stats


def importance_scores(stats, gaussians, kind="weight_volume", volume_power=0.1):
    """[P] float32 scores (higher = more important) of one of KINDS."""
    if kind not in KINDS:
        raise ValueError(f"importance_scores: kind must be one of {KINDS} (got {kind!r})")
    if kind == "weight":
        return stats.sum_gw.clone()
    if kind == "max_weight":
        return stats.max_w.clone()
    if kind == "count":
        return stats.count.to(torch.float32)
    with torch.no_grad():
        vol = torch.prod(gaussians.get_scaling.detach(), dim=1)
        if vol.numel() == 0:
            return stats.sum_gw.clone()
        # the 90th-percentile volume: the k-th smallest, k = ceil(0.9 P)
        q90 = torch.kthvalue(vol, max(1, math.ceil(0.9 * vol.numel()))).values
        return stats.sum_gw * torch.clamp(vol / q90, 0.0, 1.0) ** volume_power


def prune_mask(scores, fraction=None, threshold=None):
    """Boolean [P] mask of the Gaussians to remove: exactly one of `fraction` (the floor(fraction P)
    lowest scores, ties broken by index: the lower index goes first) or `threshold` (every score
    below it)."""
    if (fraction is None) == (threshold is None):
        raise ValueError("prune_mask: give exactly one of fraction / threshold")
    scores = scores.detach().reshape(-1)
    P = scores.shape[0]
    if threshold is not None:
        return scores < threshold
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError(f"prune_mask: fraction must be in [0, 1] (got {fraction})")
    k = int(math.floor(float(fraction) * P))
    mask = torch.zeros(P, dtype=torch.bool, device=scores.device)
    if k > 0:
        order = torch.sort(scores, stable=True).indices  # stable: equal scores stay in index order
        mask[order[:k]] = True
    return mask
