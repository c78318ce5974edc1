"""MCMC densification ("3D Gaussian Splatting as Markov Chain Monte Carlo", Kheradmand et al.,
NeurIPS 2024; gsplat's MCMCStrategy; include/rain_train.h rt_mcmc_*).

The set of Gaussians evolves under a hard cap instead of a gradient threshold:

* relocate_dead   dead Gaussians (opacity <= min_opacity) become copies of live ones drawn in
                  proportion to their opacity, in place; source and copies get the closed-form
                  opacity / scale correction of relocation_values, which keeps the rendered
                  result of N coincident copies close to the one Gaussian's;
* add_new         the set grows by 5 % per event up to `cap_max`, the new rows drawn the same way;
* step            the optimizer block: L1 regularisers on opacity and scale, Adam, and a small
                  covariance-shaped noise on the positions of low-opacity Gaussians.

No gradient statistic, no split, no prune and no opacity reset.  On HIP tensors with FusedAdam every
function runs the native kernels (rain_amd/csrc/mcmc.hip: parameters and moments are updated in
place, the tensors keep their identity); on CPU tensors with torch.optim.Adam a plain-torch path
with the same semantics runs, so the training loop can be exercised without a GPU.  Relocated rows
(sources and destinations) restart with zero Adam moments: gsplat clears the sources' only.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _native as N

N_MAX = N.RT_MCMC_N_MAX
MULTINOMIAL_MAX = 1 << 24  # torch.multinomial's limit on the number of categories
GATE_K, GATE_X0 = 100.0, 0.005
_FLT_EPSILON = 1.1920928955078125e-07
_KINDS = {"xyz": N.RT_GROUP_XYZ, "scaling": N.RT_GROUP_SCALING, "opacity": N.RT_GROUP_OPACITY}
_GEOMETRY = ("xyz", "opacity", "scaling", "rotation")


def _correction(opacity: torch.Tensor, ratio: torch.Tensor):
    """(o', coeff) in float64 for activated opacities o and copy counts N = ratio (clamped to 1..N_MAX):
    o' = 1 - (1 - o)^(1/N), coeff = o / D, D = sum_{a=1..N} sum_{k<a} C(a-1,k) (-1)^k o'^(k+1) / sqrt(k+1)."""
    o = opacity.to(torch.float64).reshape(-1)
    n = ratio.to(torch.int64).reshape(-1).clamp(1, N_MAX)
    on = 1.0 - torch.pow(1.0 - o, 1.0 / n.to(torch.float64))
    k = torch.arange(N_MAX, dtype=torch.float64, device=o.device)
    # binom[a-1, k] = C(a-1, k); rows a > N and columns k >= a contribute nothing
    binom = torch.tensor([[math.comb(a, j) for j in range(N_MAX)] for a in range(N_MAX)], dtype=torch.float64,
                         device=o.device)
    term = (-1.0) ** k * on[:, None] ** (k + 1.0) / torch.sqrt(k + 1.0)       # [n, k]
    inner = term @ binom.T                                                     # [n, a-1]
    rows = (torch.arange(N_MAX, device=o.device)[None, :] < n[:, None]).to(torch.float64)
    D = (inner * rows).sum(dim=1)
    one = n == 1  # exact: o' = o, coeff = 1
    return torch.where(one, o, on), torch.where(one, torch.ones_like(o), o / D)


def relocation_values(opacity: torch.Tensor, scale: torch.Tensor, ratio: torch.Tensor):
    """(new_opacity, new_scale) of a Gaussian with activated `opacity` [n] and `scale` [n,3] that is to
    stand `ratio` [n] times in the same place (the paper's eq. 9), in float64 on the inputs' device;
    the opacity is not clamped.  The formula's documentation and the CPU path of relocate()."""
    on, coeff = _correction(opacity, ratio)
    return on.reshape(opacity.shape), scale.to(torch.float64) * coeff.reshape((-1,) + (1,) * (scale.dim() - 1))


def _groups(model):
    """(name, parameter, optimizer state or None) of every parameter group."""
    out = []
    for group in model.optimizer.param_groups:
        p = group["params"][0]
        st = model.optimizer.state.get(p, None)
        out.append((group["name"], p, st if st is not None and "exp_avg" in st else None))
    return out


def _native_path(model) -> bool:
    return model._xyz.device.type == "cuda" and hasattr(model.optimizer, "fused_step")


@torch.no_grad()
def relocate(model, src: torch.Tensor, dst: torch.Tensor, min_opacity: float = 0.005):
    """Rows dst[j] become copies of rows src[j] in every parameter group, in place, with the relocation
    correction and zero moments (include/rain_train.h rt_mcmc_relocate).  `dst` must hold distinct rows
    and share none with `src`."""
    n = int(src.numel())
    if n == 0:
        return
    P = model._xyz.shape[0]
    src = src.to(torch.int64).contiguous()
    dst = dst.to(torch.int64).contiguous()
    if _native_path(model):
        L = N.train_lib()
        structs, keep = [], []
        for name, p, st in _groups(model):
            width = math.prod(p.shape[1:])
            if width == 0:
                continue
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise RuntimeError("rain_amd.mcmc: parameters must be contiguous float32")
            m = st["exp_avg"] if st is not None else None
            v = st["exp_avg_sq"] if st is not None else None
            if st is not None and not (m.is_contiguous() and v.is_contiguous()):
                raise RuntimeError("rain_amd.mcmc: optimizer moments must be contiguous")
            keep.append((p, m, v))
            structs.append(N.RTMcmcGroup(p.data_ptr(), m.data_ptr() if m is not None else None,
                                         v.data_ptr() if v is not None else None, width,
                                         _KINDS.get(name, N.RT_GROUP_OTHER)))
        ws = torch.empty((L.rt_mcmc_workspace_bytes(P),), dtype=torch.uint8, device=model._xyz.device)
        arr = (N.RTMcmcGroup * len(structs))(*structs)
        N.check_rt(L.rt_mcmc_relocate(P, src.data_ptr(), dst.data_ptr(), n, float(min_opacity), arr, len(structs),
                                      ws.data_ptr(), ws.numel(), N.stream_of(model._xyz)), "rt_mcmc_relocate")
        return
    counts = torch.bincount(src, minlength=P)
    on, coeff = _correction(torch.sigmoid(model._opacity.detach().to(torch.float64)), counts + 1)
    xc = on.clamp(float(min_opacity), 1.0 - _FLT_EPSILON)
    new_op = torch.log(xc / (1.0 - xc)).to(torch.float32)[:, None]
    new_sc = (model._scaling.detach().to(torch.float64) + torch.log(coeff)[:, None]).to(torch.float32)
    is_src = counts > 0
    for name, p, st in _groups(model):
        d = p.data
        d[dst] = d[src]
        if name == "opacity":
            d[dst] = new_op[src]
            d[is_src] = new_op[is_src]
        elif name == "scaling":
            d[dst] = new_sc[src]
            d[is_src] = new_sc[is_src]
        if st is not None:
            for mom in (st["exp_avg"], st["exp_avg_sq"]):
                mom[dst] = 0.0
                mom[is_src] = 0.0


def _check_categories(n: int):
    if n > MULTINOMIAL_MAX:
        raise ValueError(f"rain_amd.mcmc: torch.multinomial takes at most 2^24 categories, got {n} Gaussians to "
                         "draw from")


@torch.no_grad()
def relocate_dead(model, min_opacity: float = 0.005, generator=None) -> int:
    """Relocate every dead Gaussian (sigmoid(opacity) <= min_opacity) onto a live one drawn in proportion
    to its opacity.  Returns the number relocated (0 when none is dead or none alive)."""
    op = torch.sigmoid(model._opacity.detach()).reshape(-1)
    dead = op <= min_opacity
    n_dead = int(dead.sum())
    if n_dead == 0 or n_dead == op.numel():
        return 0
    _check_categories(op.numel() - n_dead)
    alive_idx = (~dead).nonzero(as_tuple=True)[0]
    src = alive_idx[torch.multinomial(op[alive_idx], n_dead, replacement=True, generator=generator)]
    relocate(model, src, dead.nonzero(as_tuple=True)[0], min_opacity)
    return n_dead


@torch.no_grad()
def add_new(model, cap_max: int, generator=None, min_opacity: float = 0.005) -> int:
    """Grow the set by 5 % (at most to `cap_max`): the new rows are copies of rows drawn in proportion to
    their opacity, appended through densification_postfix (zero moments, statistics resized), then
    relocated like the dead.  Returns the number added."""
    P = model._xyz.shape[0]
    n_new = max(0, min(int(cap_max), int(1.05 * P)) - P)
    if n_new == 0:
        return 0
    _check_categories(P)
    src = torch.multinomial(torch.sigmoid(model._opacity.detach()).reshape(-1), n_new, replacement=True,
                            generator=generator)
    model.densification_postfix(model._xyz.detach()[src], model._features_dc.detach()[src],
                                model._features_rest.detach()[src], model._opacity.detach()[src],
                                model._scaling.detach()[src], model._rotation.detach()[src])
    relocate(model, src, P + torch.arange(n_new, device=src.device), min_opacity)
    return n_new


def _advance(optimizer, p):
    """FusedAdam.step's book-keeping for one parameter: create the state, advance the step count and
    return (group, state, bias_correction1, bias_correction2_sqrt)."""
    group = next(g for g in optimizer.param_groups if any(q is p for q in g["params"]))
    state = optimizer.state[p]
    if len(state) == 0:
        state["step"] = torch.tensor(0.0, dtype=torch.float32)
        state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
    stp = state["step"]
    if stp.device.type != "cpu":
        stp = state["step"] = stp.detach().to("cpu", torch.float32)
    stp += 1.0
    k = float(stp.item())
    b1, b2 = group["betas"]
    return group, state, 1.0 - math.pow(b1, k), math.sqrt(1.0 - math.pow(b2, k))


def _xyz_lr(model) -> float:
    return float(next(g["lr"] for g in model.optimizer.param_groups if g["name"] == "xyz"))


@torch.no_grad()
def step(model, noise: torch.Tensor | None, noise_lr: float, opacity_reg: float, scale_reg: float,
         do_adam: bool = True):
    """The MCMC iteration's optimizer block (include/rain_train.h rt_mcmc_step) on the gradients in
    the parameters' .grad: the regularisers' gradients lambda_o d mean(sigmoid(opacity)) and
    lambda_s d mean(exp(scaling)), one Adam step of every group (skipped without `do_adam`: step counts
    then stay), then xyz += Sigma (noise * gate * noise_lr * lr_xyz) with the updated parameters, `noise`
    being [P,3] standard normals (None: no noise).  HIP: one launch for the four geometry groups and
    one rt_adam_step for f_dc / f_rest.  CPU: torch, adding the regularisers into .grad."""
    noise_scale = float(noise_lr) * _xyz_lr(model)
    params = dict(xyz=model._xyz, f_dc=model._features_dc, f_rest=model._features_rest, opacity=model._opacity,
                  scaling=model._scaling, rotation=model._rotation)
    P = model._xyz.shape[0]
    if noise is not None and (tuple(noise.shape) != (P, 3) or noise.dtype != torch.float32
                              or noise.device != model._xyz.device):
        raise ValueError("rain_amd.mcmc.step: noise must be a float32 [P, 3] tensor on the model's device")
    if do_adam and any(p.grad is None for p in params.values()):
        raise RuntimeError("rain_amd.mcmc.step: every parameter needs a gradient (do_adam)")
    if not _native_path(model):
        if do_adam:
            if opacity_reg:
                s = torch.sigmoid(model._opacity.detach())
                model._opacity.grad += (opacity_reg / P) * s * (1.0 - s)
            if scale_reg:
                model._scaling.grad += (scale_reg / (3.0 * P)) * torch.exp(model._scaling.detach())
            model.optimizer.step()
        if noise is not None:
            from .gaussian_model import build_scaling_rotation

            o = torch.sigmoid(model._opacity.detach())
            gate = torch.sigmoid(-GATE_K * (o - GATE_X0))
            Lm = build_scaling_rotation(torch.exp(model._scaling.detach()), model._rotation.detach())
            cov = Lm @ Lm.transpose(1, 2)
            model._xyz.data += torch.bmm(cov, (noise * gate * noise_scale).unsqueeze(-1)).squeeze(-1)
        return
    L = N.train_lib()
    opt = model.optimizer
    a = N.RTMcmcStepArgs()
    a.P = P
    a.do_adam = int(bool(do_adam))
    keep, sh = [], []
    betas = None
    for name, p in params.items():
        if not p.is_contiguous() or p.dtype != torch.float32:
            raise RuntimeError("rain_amd.mcmc: parameters must be contiguous float32")
        if not do_adam:
            if name in _GEOMETRY:
                getattr(a, name).param = p.data_ptr()
            continue
        g = p.grad
        if g.is_sparse or not g.is_contiguous() or g.dtype != torch.float32:
            raise RuntimeError("rain_amd.mcmc: gradients must be dense contiguous float32")
        group, state, bc1, bc2s = _advance(opt, p)
        b = (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]))
        if betas is None:
            betas = b
        elif betas != b:
            raise RuntimeError("rain_amd.mcmc.step: all groups must share betas and eps")
        m, v = state["exp_avg"], state["exp_avg_sq"]
        keep.append((g, m, v))
        if name in _GEOMETRY:
            sg = getattr(a, name)
            sg.param, sg.grad, sg.exp_avg, sg.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            sg.lr, sg.bias_correction1, sg.bias_correction2_sqrt = float(group["lr"]), bc1, bc2s
        elif p.numel() > 0:
            sh.append(N.RTAdamGroup(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                                    float(group["lr"]), bc1, bc2s))
    if betas is not None:
        a.beta1, a.beta2, a.eps = betas
    a.opacity_reg, a.scale_reg = float(opacity_reg), float(scale_reg)
    if noise is not None:
        noise = noise.contiguous()
        a.noise = noise.data_ptr()
    a.noise_scale = noise_scale
    a.gate_k, a.gate_x0 = GATE_K, GATE_X0
    stream = N.stream_of(model._xyz)
    N.check_rt(L.rt_mcmc_step(ctypes.byref(a), stream), "rt_mcmc_step")
    if sh:
        arr = (N.RTAdamGroup * len(sh))(*sh)
        N.check_rt(L.rt_adam_step(arr, len(sh), betas[0], betas[1], betas[2], stream), "rt_adam_step")
