"""Reference for the per-Gaussian blend-contribution statistics (rr_contributions), in numpy from the
oracle's forward state alone.

`contributions_ref` walks every tile's depth-ordered list of the oracle's internals() front to back, all
of a tile's pixels at once: alpha with the reference's float32 expressions (forward.cu:329-338: power
from the conic and the pixel offset, power > 0 skipped, alpha = min(0.99, opacity exp(power)), alpha <
1/255 skipped), a pair counted at a pixel while its list index is below that pixel's n_contrib (the
forward's last contributor, which already holds its saturation stop), T the running product of
1 - alpha over the counted pairs (float64), w = alpha T.

`oracle_sums` is what pins it (tests/test_contrib_ref_cpu.py): the oracle's backward with colors_precomp
gives dL_dcolors[i, c] = sum_p w_i(p) dL_dpix[c, p], so dL_dpix = (g, 1, 0) leaves sum_gw in channel 0
and sum_w in channel 1 (the trick of tests/depth_ref.py)."""
from __future__ import annotations

import numpy as np
import torch

from tests.common import oracle_run


def contributions_ref(internals, W, H, g=None):
    """dict(sum_w, sum_gw, max_w [P] float64, count [P] int64) of the oracle frame `internals`; g: [H,W]
    pixel weights (None: 1)."""
    point_list, ranges = internals["point_list"], internals["ranges"]
    n_contrib = internals["n_contrib"].astype(np.int64)
    xy, co = internals["xy"].astype(np.float32), internals["conic_opacity"].astype(np.float32)
    P = xy.shape[0]
    gmap = np.ones((H, W), np.float64) if g is None else np.asarray(g, np.float64).reshape(H, W)
    sum_w, sum_gw, max_w = np.zeros(P), np.zeros(P), np.zeros(P)
    count = np.zeros(P, np.int64)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    f32 = np.float32
    for ty in range(gy):
        for tx in range(gx):
            lo, hi = (int(v) for v in ranges[ty * gx + tx])
            ys, xs = np.meshgrid(np.arange(ty * 16, min(ty * 16 + 16, H)), np.arange(tx * 16, min(tx * 16 + 16, W)),
                                 indexing="ij")
            ys, xs = ys.ravel(), xs.ravel()
            last = n_contrib[ys, xs]
            n = min(hi - lo, int(last.max()) if last.size else 0)
            if n <= 0:
                continue
            ids = point_list[lo:lo + n].astype(np.int64)
            dx = xy[ids, 0][:, None] - xs.astype(f32)[None, :]
            dy = xy[ids, 1][:, None] - ys.astype(f32)[None, :]
            cx, cy, cz, op = (co[ids, k][:, None] for k in range(4))
            power = f32(-0.5) * (cx * dx * dx + cz * dy * dy) - cy * dx * dy
            with np.errstate(over="ignore"):
                alpha = np.minimum(f32(0.99), op * np.exp(power, dtype=f32))
            act = (power <= 0) & (alpha >= f32(1.0 / 255.0)) & (np.arange(n)[:, None] < last[None, :])
            a = np.where(act, alpha, f32(0)).astype(np.float64)
            T = np.cumprod(1.0 - a, axis=0)
            T = np.concatenate([np.ones((1, a.shape[1])), T[:-1]], axis=0)  # in front of each pair
            w = a * T
            # a Gaussian is in a tile's list once: plain indexed updates
            sum_w[ids] += w.sum(axis=1)
            sum_gw[ids] += (w * gmap[ys, xs][None, :]).sum(axis=1)
            max_w[ids] = np.maximum(max_w[ids], w.max(axis=1))
            count[ids] += act.sum(axis=1)
    return dict(sum_w=sum_w, sum_gw=sum_gw, max_w=max_w, count=count)


def precomp_scene(inp, seed=7):
    """The scene with precomputed colours instead of SH (same geometry, same blend lists)."""
    P = inp["means3D"].shape[0]
    inp2 = {k: v for k, v in inp.items() if k not in ("shs", "colors_precomp")}
    inp2["colors_precomp"] = torch.rand((P, 3), generator=torch.Generator().manual_seed(seed))
    return inp2


def oracle_sums(oracle, inp, st, g, nthreads=0):
    """(sum_gw, sum_w, the run) from the oracle's backward of the precomputed-colour scene with
    dL_dpix = (g, 1, 0)."""
    H, W = st["image_height"], st["image_width"]
    dpix = np.zeros((3, H, W), np.float32)
    dpix[0] = np.asarray(g, np.float32).reshape(H, W)
    dpix[1] = 1.0
    run = oracle_run(oracle, precomp_scene(inp), st, dL_dpix=dpix, nthreads=nthreads)
    dc = np.asarray(run["grads"]["dL_dcolors"], np.float64)
    return dc[:, 0], dc[:, 1], run
