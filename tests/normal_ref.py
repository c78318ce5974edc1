"""Reference for the aux normal map's gradients, from the existing oracle plus float64 autograd.

The trick of tests/depth_ref.py again: rendering the same geometry with colors_precomp = n_i (the
Gaussians' view-space unit normals) over a zero background makes the three channels the normal map
N = sum alpha_i T_i n_i.  The oracle's backward of that run with dL_dpix = dL/dN gives the normal
term's alpha-path gradients in its geometric outputs (GEOMETRIC) and dL/dn_i in dL_dcolors.  n_i is
computed here in float64 torch from (scales, rotations, viewmatrix, means3D) the way gaussian_normal
(rain_amd/csrc/rr_common.hpp) does — the axis index k (from the float32 scales, strict comparisons)
and the flip towards the camera are constants — so autograd of (n . dL/dn_i).sum() with respect to
the rotations is the direct term dL_drotations gains.  Scales, means3D and the camera get nothing
from n_i.  The full reference is the colour run, plus the depth and alpha parts, plus this."""
from __future__ import annotations

import numpy as np
import torch

from tests.common import GRAD_NAMES, make_scene, oracle_run
from tests.depth_ref import GEOMETRIC, trick_scene

# the GPU tests' scenes (tests/test_normal_grad_gpu.py); tests/test_normal_ref_cpu.py asserts their
# input conditions
SCENES = {
    "sh3": dict(P=3000, W=128, H=96, sh_degree=3),
    "ragged_bg": dict(P=2000, W=100, H=75, sh_degree=1, bg=(1.0, 0.5, 0.25)),
    "low_pass_300": dict(P=800, W=160, H=120, sh_degree=3, low_pass=300.0),
}


def perturb(inp):
    """make_scene gives isotropic scales and unit quaternions (k = 0 everywhere, |nv| = 1): spread the
    scales and un-normalise the quaternions."""
    P = inp["means3D"].shape[0]
    g = torch.Generator().manual_seed(5)
    out = dict(inp)
    out["scales"] = (inp["scales"] * torch.exp(0.4 * torch.randn((P, 3), generator=g))).float().contiguous()
    out["rotations"] = (inp["rotations"] * (0.7 + 0.8 * torch.rand((P, 1), generator=g))).float().contiguous()
    return out


def perturbed_scene(**kw):
    inp, st = make_scene(**kw)
    return perturb(inp), st


def smallest_axis(scales):
    """k of gaussian_normal on the float32 scales: strict comparisons, ties keep the lower index."""
    s = scales.float()
    k = torch.zeros(s.shape[0], dtype=torch.long)
    k[s[:, 1] < s[:, 0]] = 1
    cur = torch.where(k == 0, s[:, 0], s[:, 1])
    k[s[:, 2] < cur] = 2
    return k


def normal_terms(scales, rotations, viewmatrix, means3D):
    """float64 (nv [P,3] before the flip, p_view [P,3], k [P]); differentiable in `rotations`."""
    q = rotations.double()
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
        torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
        torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], 1)  # [P, row, col]
    k = smallest_axis(scales)
    n_w = R[torch.arange(q.shape[0]), :, k]  # column k
    M = torch.as_tensor(viewmatrix).double().reshape(4, 4)  # flat m[4 j + i]: V[i][j] = M[j][i]
    nv = n_w @ M[:3, :3]
    p_view = torch.as_tensor(means3D).double() @ M[:3, :3] + M[3, :3]
    return nv, p_view, k


def normals64(scales, rotations, viewmatrix, means3D):
    """n_i [P,3] float64 by gaussian_normal's steps 1-5; sign and k are constants."""
    nv, p_view, _k = normal_terms(scales, rotations, viewmatrix, means3D)
    sign = torch.where((nv.detach() * p_view).sum(-1) > 0, -1.0, 1.0).double()
    nv = nv * sign[:, None]
    ln = nv.norm(dim=-1, keepdim=True)
    return torch.where(ln > 0, nv / ln.clamp_min(1e-300), torch.zeros_like(nv))


def normal_scene(inp, st):
    """The scene with colours n_i and a zero background (same geometry, same blend lists)."""
    n = normals64(inp["scales"], inp["rotations"], st["viewmatrix"], inp["means3D"])
    inp2 = {k: v for k, v in inp.items() if k not in ("shs", "colors_precomp")}
    inp2["colors_precomp"] = n.float().contiguous()
    return inp2, dict(st, bg=torch.zeros(3, dtype=torch.float32))


def normal_part(oracle, inp, st, dn, nthreads=0):
    """The normal term's contribution to each of the eight gradients for dL/dN = dn [3,H,W]."""
    inp2, st2 = normal_scene(inp, st)
    tr = oracle_run(oracle, inp2, st2, dL_dpix=np.asarray(dn, np.float32), nthreads=nthreads)
    part = {k: np.zeros_like(np.asarray(tr["grads"][k], np.float64)) for k in GRAD_NAMES}
    sh = inp.get("shs")
    part["dL_dsh"] = np.zeros(tuple(sh.shape) if sh is not None else (inp["means3D"].shape[0], 0, 3), np.float64)
    for k in GEOMETRIC:
        part[k] += tr["grads"][k]
    rot = inp["rotations"].double().clone().requires_grad_()
    n = normals64(inp["scales"], rot, st["viewmatrix"], inp["means3D"])
    dL_dn = torch.from_numpy(np.asarray(tr["grads"]["dL_dcolors"], np.float64))
    (g,) = torch.autograd.grad((n * dL_dn).sum(), rot)
    part["dL_drotations"] += g.numpy()
    return part, tr


def full_reference(oracle, inp, st, dpix, dd, da, dn):
    """The colour run's gradients and the depth, alpha and normal parts (the backward is linear in
    the output gradients, so every combination of present maps is a sum of these)."""
    H, W = st["image_height"], st["image_width"]
    col = oracle_run(oracle, inp, st, dL_dpix=dpix)
    internals = col["state"].internals()
    inp2, st2 = trick_scene(inp, st, internals["depths"])
    zrow = np.asarray(st["viewmatrix"], np.float64).reshape(4, 4)[:3, 2]
    colour = {k: np.asarray(col["grads"][k], np.float64) for k in GRAD_NAMES}
    parts = {}
    for key, ch, m in (("depth", 0, dd), ("alpha", 1, da)):
        dtrick = np.zeros((3, H, W), np.float32)
        dtrick[ch] = m[0]
        tr = oracle_run(oracle, inp2, st2, dL_dpix=dtrick)["grads"]
        part = {k: np.zeros_like(v) for k, v in colour.items()}
        for k in GEOMETRIC:
            part[k] += tr[k]
        part["dL_dmeans3D"] += np.asarray(tr["dL_dcolors"], np.float64)[:, 0:1] * zrow
        parts[key] = part
    parts["normal"], _tr = normal_part(oracle, inp, st, dn)
    return dict(col=col, internals=internals, colour=colour, parts=parts)
