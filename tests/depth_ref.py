"""Reference for the depth / accumulated-alpha gradients, from the existing oracle alone.

Rendering with colors_precomp = [z_i, 1, 0] and a zero background makes channel 0 the depth map
D = sum alpha_i T_i z_i and channel 1 the accumulated alpha A = 1 - T_final.  The oracle's backward
of that "trick run" with dL_dpix = (dL/dD, dL/dA, 0) is therefore the depth and alpha gradient of
every geometric input; what it leaves in dL_dcolors[:, 0] is dL/dz_i, which reaches means3D through
z = (mean, 1) . view[:, 2].  The full reference is the colour run's gradients plus these
(dL_dsh and dL_dcolors come from the colour run only)."""
from __future__ import annotations

import numpy as np
import torch

GEOMETRIC = ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")


def trick_scene(inp, st, z):
    """The scene with colours [z_i, 1, 0] and a zero background (same geometry, same blend lists)."""
    P = inp["means3D"].shape[0]
    col = torch.zeros((P, 3), dtype=torch.float32)
    col[:, 0] = torch.as_tensor(np.asarray(z), dtype=torch.float32)
    col[:, 1] = 1.0
    inp2 = {k: v for k, v in inp.items() if k not in ("shs", "colors_precomp")}
    inp2["colors_precomp"] = col
    return inp2, dict(st, bg=torch.zeros(3, dtype=torch.float32))
