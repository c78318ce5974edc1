"""Reference for the depth-moment maps' gradients, from the existing oracle alone.

The trick of tests/depth_ref.py again: rendering the same geometry with colors_precomp =
[m_i, 1, m_i^2] (m_i = m(z_i) the mapped view depth) over a zero background makes channel 0 the
first moment M1 = sum alpha_i T_i m_i, channel 1 the accumulated alpha and channel 2 the second
moment M2 = sum alpha_i T_i m_i^2.  The oracle's backward of that run with dL_dpix = (dL/dM1, 0,
dL/dM2) gives the moment term's gradient of every geometric input; what it leaves in dL_dcolors is
(dL/dm_i, ., dL/d(m_i^2)), so dL/dz_i = (dc0 + 2 m_i dc2) dm/dz, which reaches means3D through
z = (mean, 1) . view[:, 2].  dL_dsh and dL_dcolors get nothing from the moments."""
from __future__ import annotations

import numpy as np
import torch

from tests.common import GRAD_NAMES, oracle_run
from tests.depth_ref import GEOMETRIC

# the two mappings: 2DGS's NDC depth between near and far, and the metric depth
MAPPINGS = {"ndc": (0.2, 100.0), "metric": (0.0, 0.0)}


def mapped_depth(z, near, far):
    """float64 (m(z), dm/dz) of include/rain_raster.h's two mappings.  Gaussians the preprocess
    culled carry depth 0 in the oracle's arrays and are in no blend list: they get m = dm/dz = 0."""
    z = np.asarray(z, np.float64)
    seen = z > 0.0
    if near == 0.0 and far == 0.0:
        return np.where(seen, z, 0.0), seen.astype(np.float64)
    s = far / (far - near)
    zs = np.where(seen, z, 1.0)
    return np.where(seen, s * (1.0 - near / zs), 0.0), np.where(seen, s * near / (zs * zs), 0.0)


def dist_scene(inp, st, z, near, far):
    """The scene with colours [m_i, 1, m_i^2] and a zero background (same geometry, same lists)."""
    P = inp["means3D"].shape[0]
    m, _ = mapped_depth(z, near, far)
    col = torch.zeros((P, 3), dtype=torch.float32)
    col[:, 0] = torch.from_numpy(m.astype(np.float32))
    col[:, 1] = 1.0
    col[:, 2] = torch.from_numpy((m * m).astype(np.float32))
    inp2 = {k: v for k, v in inp.items() if k not in ("shs", "colors_precomp")}
    inp2["colors_precomp"] = col
    return inp2, dict(st, bg=torch.zeros(3, dtype=torch.float32))


def dist_part(oracle, inp, st, z, dmom, near, far, like=None, nthreads=0):
    """The moment term's contribution to each of the eight gradients for dL/d(M1, M2) = dmom [2,H,W]
    (float64 arrays shaped like `like`'s, default the trick run's), and the trick run itself."""
    H, W = st["image_height"], st["image_width"]
    inp2, st2 = dist_scene(inp, st, z, near, far)
    dtrick = np.zeros((3, H, W), np.float32)
    dtrick[0], dtrick[2] = dmom[0], dmom[1]
    tr = oracle_run(oracle, inp2, st2, dL_dpix=dtrick, nthreads=nthreads)
    like = tr["grads"] if like is None else like
    part = {k: np.zeros_like(np.asarray(like[k], np.float64)) for k in GRAD_NAMES}
    for k in GEOMETRIC:
        part[k] += tr["grads"][k]
    m, dmdz = mapped_depth(z, near, far)
    dc = np.asarray(tr["grads"]["dL_dcolors"], np.float64)
    dz = (dc[:, 0] + 2.0 * m * dc[:, 2]) * dmdz
    zrow = np.asarray(st["viewmatrix"], np.float64).reshape(4, 4)[:3, 2]
    part["dL_dmeans3D"] += dz[:, None] * zrow
    return part, tr
