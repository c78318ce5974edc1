"""Reference for the absolute-gradient densification statistics (include/rain_raster.h RR_FLAG_ABSGRAD), in
float64 numpy from the oracle's forward state alone.

`mean2d_sums` is the tile walk of tests/contrib_ref.py (every tile's depth-ordered list of the oracle's
internals() front to back, all of a tile's pixels at once, alpha by the reference's float32 expressions, a
pair counted at a pixel while its list index is below that pixel's n_contrib), extended with the blend
backward's per-pixel terms.  With w_j = alpha_j T_j, c_j the pair's colour and dpix the pixel's output
gradient,

    dL/dalpha_k = T_k (c_k . dpix) - (sum_{j>k} w_j (c_j . dpix) + T_final (bg . dpix)) / (1 - alpha_k)

(the derivative of C = sum_j w_j c_j + T_final bg; like the reference, with no mask for the 0.99 clamp), and
the two mean terms of oracle/raster_oracle.c:608-613,

    dL/dG = opacity dL/dalpha,   gdx = G dx,   gdy = G dy        (dx, dy = mean - pixel)
    term_x = dL/dG (-gdx conic.x - gdy conic.y) 0.5 W
    term_y = dL/dG (-gdy conic.z - gdx conic.y) 0.5 H

It returns both the signed sums over a Gaussian's pixels (the oracle's dL_dmeans2D: what pins this walk,
tests/test_absgrad_ref_cpu.py) and the sums of their magnitudes (what RR_FLAG_ABSGRAD accumulates)."""
from __future__ import annotations

import math

import numpy as np
import torch

from tests.common import make_scene

# the three scenes of the parity checks, and a precomputed-colour / precomputed-covariance one
SCENES = {
    "sh3": dict(P=2000, W=128, H=96, sh_degree=3),
    "ragged_bg": dict(P=2000, W=100, H=75, sh_degree=1, bg=(1.0, 0.5, 0.25)),
    "large": dict(P=300, W=40, H=24, sh_degree=0, scale_mult=3.0),
    "precomp": dict(P=1500, W=96, H=80, sh_degree=3, precomp_colors=True, precomp_cov=True),
}


def scene(name):
    """(inp, st, dL_dpix): make_scene of SCENES[name] and a random colour gradient [3,H,W]."""
    inp, st = make_scene(**SCENES[name])
    H, W = st["image_height"], st["image_width"]
    dpix = np.random.default_rng(5).standard_normal((3, H, W)).astype(np.float32)
    return inp, st, dpix


def mean2d_sums(internals, colors, bg, dL_dpix, W, H):
    """(signed [P,2], absolute [P,2]) float64 sums of the per-pixel dL/dmeans2D terms of the oracle frame
    `internals`; colors [P,3]: the Gaussians' colours (internals()["rgb"], or the precomputed ones);
    bg [3]; dL_dpix [3,H,W]."""
    point_list, ranges = internals["point_list"], internals["ranges"]
    n_contrib = internals["n_contrib"].astype(np.int64)
    xy, co = internals["xy"].astype(np.float32), internals["conic_opacity"].astype(np.float32)
    P = xy.shape[0]
    col = np.asarray(colors, np.float64).reshape(P, 3)
    bg = np.asarray(bg, np.float64).reshape(3)
    dp = np.asarray(dL_dpix, np.float64).reshape(3, H, W)
    signed, absolute = np.zeros((P, 2)), np.zeros((P, 2))
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
                G = np.exp(power, dtype=f32)
                alpha = np.minimum(f32(0.99), op * G)
            act = (power <= 0) & (alpha >= f32(1.0 / 255.0)) & (np.arange(n)[:, None] < last[None, :])
            a = np.where(act, alpha, f32(0)).astype(np.float64)
            Tn = np.cumprod(1.0 - a, axis=0)  # behind each pair; the last row is T_final
            T = np.concatenate([np.ones((1, a.shape[1])), Tn[:-1]], axis=0)  # in front of each pair
            dpx = dp[:, ys, xs]  # [3, pixels]
            cd = col[ids] @ dpx  # c_j . dpix  [n, pixels]
            wcd = a * T * cd
            behind = np.cumsum(wcd[::-1], axis=0)[::-1] - wcd  # sum_{j>k} w_j (c_j . dpix)
            tail = behind + Tn[-1][None, :] * (bg @ dpx)[None, :]
            dL_dalpha = T * cd - tail / (1.0 - a)
            dL_dG = op.astype(np.float64) * dL_dalpha
            G64 = np.where(act, G, f32(0)).astype(np.float64)
            gdx, gdy = G64 * dx.astype(np.float64), G64 * dy.astype(np.float64)
            cx64, cy64, cz64 = (v.astype(np.float64) for v in (cx, cy, cz))
            term_x = np.where(act, dL_dG * (-gdx * cx64 - gdy * cy64) * (0.5 * W), 0.0)
            term_y = np.where(act, dL_dG * (-gdy * cz64 - gdx * cy64) * (0.5 * H), 0.0)
            # a Gaussian is in a tile's list once: plain indexed updates
            signed[ids, 0] += term_x.sum(axis=1)
            signed[ids, 1] += term_y.sum(axis=1)
            absolute[ids, 0] += np.abs(term_x).sum(axis=1)
            absolute[ids, 1] += np.abs(term_y).sum(axis=1)
    return signed, absolute


def scene_colors(run, inp):
    """The per-Gaussian colours the blend used: the precomputed ones, or the oracle's SH evaluation."""
    if "colors_precomp" in inp:
        return inp["colors_precomp"].numpy()
    return run["state"].internals()["rgb"]


def reference(oracle, inp, st, dL_dpix):
    """The oracle run of the scene (forward and backward) with "signed" and "abs" [P,2] added."""
    from tests.common import oracle_run

    run = oracle_run(oracle, inp, st, dL_dpix=dL_dpix)
    H, W = st["image_height"], st["image_width"]
    run["signed"], run["abs"] = mean2d_sums(run["state"].internals(), scene_colors(run, inp), st["bg"].numpy(),
                                            dL_dpix, W, H)
    return run


def single_gaussian(W=33, H=25, sigma=0.05, z=4.0, opacity=0.8):
    """The analytic case: one isotropic Gaussian on the optical axis of an identity-view camera, which for odd
    W and H projects exactly onto the centre of pixel ((W-1)/2, (H-1)/2); black background, a constant
    precomputed colour.  With dL_dpix = 1 the per-pixel pulls are antisymmetric about that pixel, so the
    signed sums cancel and the absolute sums do not.  Returns (inp, st, dL_dpix)."""
    from rain_amd import cameras

    fovx = 0.6911112
    fovy = cameras.focal2fov(cameras.fov2focal(fovx, W), H)
    cam = cameras.Camera(R=np.eye(3), T=np.zeros(3), FoVx=fovx, FoVy=fovy, image_width=W, image_height=H)
    inp = dict(means3D=torch.tensor([[0.0, 0.0, z]]), opacities=torch.tensor([[opacity]]),
               colors_precomp=torch.tensor([[0.9, 0.6, 0.3]]), scales=torch.full((1, 3), sigma),
               rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]))
    st = dict(image_height=H, image_width=W, tanfovx=math.tan(fovx * 0.5), tanfovy=math.tan(fovy * 0.5),
              bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=cam.world_view_transform.float().contiguous(),
              projmatrix=cam.full_proj_transform.float().contiguous(), sh_degree=0,
              campos=cam.camera_center.float().contiguous(), prefiltered=False, debug=False, low_pass=0.3)
    return inp, st, np.ones((3, H, W), np.float32)
