"""The depth-normal consistency + depth loss of include/rain_loss.h (rl_geom_*) in plain torch:
dtype-generic and autograd-differentiable.  It is the reference the HIP kernels are held to, and
it makes their test inputs.

    ok = A >= alpha_min,  z = D / A where ok,  r(p) = (((2x+1)/W - 1) tanfovx, ((2y+1)/H - 1) tanfovy, 1),
    P = z r;  interior pixels with ok at p and its four axis neighbours:
    t_u = P(x+1,y) - P(x-1,y),  t_v = P(x,y+1) - P(x,y-1),  c = t_v x t_u,  valid = |c|^2 > 0,  n_d = c / |c|
    L_n = (1/HW) sum_valid (A - N . n_d),   L_d = (1/HW) sum_{ok, gt > 0} |z - gt|
    loss = lambda_normal L_n + lambda_depth L_d

The masks are constants of the forward.  A term is evaluated only when its weight is non-zero and
its map is given (otherwise it, and for the normal term the valid count, is 0).
"""
import math

import torch

SHAPES = [(3, 3), (2, 9), (5, 7), (37, 53), (64, 96), (130, 257)]  # (H, W) of the GPU tests
TANFOV = (0.7, 0.45)


def rays(H, W, tanfovx, tanfovy, dtype, device):
    xs = ((2 * torch.arange(W, dtype=dtype, device=device) + 1) / W - 1) * tanfovx
    ys = ((2 * torch.arange(H, dtype=dtype, device=device) + 1) / H - 1) * tanfovy
    return torch.stack([xs[None, :].expand(H, W), ys[:, None].expand(H, W),
                        torch.ones((H, W), dtype=dtype, device=device)])


def depth_normal(D, A, tanfovx, tanfovy, alpha_min=0.1):
    """(n_d [3,H-2,W-2], valid [H-2,W-2] bool, P [3,H,W], ok [H,W]) of the definition; H, W >= 3."""
    H, W = D.shape[-2:]
    D2, A2 = D.reshape(H, W), A.reshape(H, W)
    ok = A2 >= alpha_min
    z = torch.where(ok, D2 / torch.where(ok, A2, torch.ones_like(A2)), torch.zeros_like(D2))
    P = z[None] * rays(H, W, tanfovx, tanfovy, D.dtype, D.device)
    t_u = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    t_v = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    c = torch.cross(t_v, t_u, dim=0)
    c2 = (c * c).sum(0)
    all5 = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1]
    valid = all5 & (c2 > 0)
    n_d = c / torch.sqrt(torch.where(valid, c2, torch.ones_like(c2)))[None]
    return n_d, valid, P, ok


def geometry_loss_ref(D, A, N, tanfovx, tanfovy, lambda_normal, lambda_depth=0.0, gt_depth=None, alpha_min=0.1):
    """Returns (loss, L_n, L_d, number of valid pixels (int))."""
    H, W = D.shape[-2:]
    D2, A2 = D.reshape(H, W), A.reshape(H, W)
    zero = torch.zeros((), dtype=D.dtype, device=D.device)
    L_n, L_d, n_valid = zero, zero, 0
    if lambda_normal != 0 and N is not None and H >= 3 and W >= 3:
        n_d, valid, _P, _ok = depth_normal(D, A, tanfovx, tanfovy, alpha_min)
        term = A2[1:-1, 1:-1] - (N.reshape(3, H, W)[:, 1:-1, 1:-1] * n_d).sum(0)
        L_n = torch.where(valid, term, torch.zeros_like(term)).sum() / (H * W)
        n_valid = int(valid.sum().item())
    if lambda_depth != 0 and gt_depth is not None:
        ok = A2 >= alpha_min
        z = torch.where(ok, D2 / torch.where(ok, A2, torch.ones_like(A2)), torch.zeros_like(D2))
        gt = gt_depth.reshape(H, W).to(D.dtype)
        m = ok & (gt > 0)
        L_d = torch.where(m, (z - gt).abs(), torch.zeros_like(z)).sum() / (H * W)
    return lambda_normal * L_n + lambda_depth * L_d, L_n, L_d, n_valid


def make_inputs(H, W, kind="smooth", seed=0):
    """float64 CPU maps (D [1,H,W], A [1,H,W], N [3,H,W], gt_depth [1,H,W]).
    smooth: z = plane + sinusoid + 0.1 uniform noise, inside [2.5, 4.5]; A uniform in [0.3, 0.99];
    N = random unit vectors x A x U[0.5, 1].  holes: the same with one rectangle and about 3 % of
    scattered pixels of A exactly 0 (far from alpha_min: every precision picks the same masks).
    gt_depth = z +- U[0.05, 0.35] (away from the kink of |.|), 10 % of it 0 (no measurement)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W)
    f64 = torch.float64
    y, x = torch.meshgrid(torch.arange(H, dtype=f64), torch.arange(W, dtype=f64), indexing="ij")
    u, v = x / max(W - 1, 1), y / max(H - 1, 1)
    z = 3.4 + 0.5 * (u - 0.5) - 0.4 * (v - 0.5) + 0.3 * torch.sin(2 * math.pi * (1.5 * u + v)) \
        + 0.1 * torch.rand((H, W), generator=g, dtype=f64)
    assert 2.5 < float(z.min()) and float(z.max()) < 4.5
    A = 0.3 + 0.69 * torch.rand((H, W), generator=g, dtype=f64)
    n = torch.randn((3, H, W), generator=g, dtype=f64)
    n = n / n.norm(dim=0, keepdim=True)
    if kind == "holes":
        A[H // 3:H // 3 + max(H // 4, 1), W // 2:W // 2 + max(W // 4, 1)] = 0.0
        A[torch.rand((H, W), generator=g, dtype=f64) < 0.03] = 0.0
    elif kind != "smooth":
        raise ValueError(kind)
    N = n * A[None] * (0.5 + 0.5 * torch.rand((H, W), generator=g, dtype=f64))[None]
    sign = torch.where(torch.rand((H, W), generator=g, dtype=f64) < 0.5, -1.0, 1.0)
    gt = z + sign * (0.05 + 0.3 * torch.rand((H, W), generator=g, dtype=f64))
    gt[torch.rand((H, W), generator=g, dtype=f64) < 0.1] = 0.0
    D = z * A
    return D[None].contiguous(), A[None].contiguous(), N.contiguous(), gt[None].contiguous()


def rel_l1(a, b):
    """sum |a - b| / sum |b| (b the reference)."""
    return float((a.double() - b.double()).abs().sum() / b.double().abs().sum())


_CACHE = {}


def reference(H, W, kind, lambda_normal, lambda_depth, dtype=torch.float64, seed=0):
    """The reference's loss parts and gradients for make_inputs(H, W, kind, seed), computed once per
    argument set: dict(loss, L_n, L_d, valid, dD, dA, dN) of CPU tensors in `dtype` (read-only)."""
    key = (H, W, kind, float(lambda_normal), float(lambda_depth), dtype, seed)
    if key not in _CACHE:
        D, A, N, gt = (t.to(dtype) for t in make_inputs(H, W, kind, seed))
        D.requires_grad_(), A.requires_grad_(), N.requires_grad_()
        loss, L_n, L_d, nv = geometry_loss_ref(D, A, N, TANFOV[0], TANFOV[1], lambda_normal, lambda_depth, gt)
        if loss.requires_grad:
            loss.backward()
        zeros = torch.zeros_like
        _CACHE[key] = dict(loss=loss.detach(), L_n=torch.as_tensor(L_n).detach(), L_d=torch.as_tensor(L_d).detach(),
                           valid=nv, dD=D.grad if D.grad is not None else zeros(D),
                           dA=A.grad if A.grad is not None else zeros(A),
                           dN=N.grad if N.grad is not None else zeros(N))
    return _CACHE[key]
