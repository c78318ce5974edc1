"""Second reference for the fused L1+SSIM loss (rain_amd/csrc/loss.hip, include/rain_loss.h): what
the forward kernel STORES and how the backward uses it, written out in torch in the dtype of its
inputs (float64 for the reference proper, float32 for the reference's own rounding error).

    m1, m2, e11, e22, e12 = blur(x), blur(y), blur(x²), blur(y²), blur(xy)      (11x11 window, zero padding)
    A = 2 m1 m2 + C1,  B = 2 (e12 - m1 m2) + C2,  Cd = m1² + m2² + C1,  Dd = (e11 - m1²) + (e22 - m2²) + C2
    S = A B / (Cd Dd)
    dS/dm1 = 2 m2 (B - A) / (Cd Dd) - 2 m1 S (1/Cd - 1/Dd),  dS/de11 = -S / Dd,  dS/de12 = 2 A / (Cd Dd)
    G1, G11, G12 = -λ/(CHW) · dS/d{m1, e11, e12}                                 (the workspace maps)
    dimg = blur(G1) + 2 x blur(G11) + y blur(G12) + (1-λ) sign(x-y)/(CHW)

The blur is the oracle's (oracle/loss_ref.py: depthwise conv2d with the 2-D window).  Pinned per
pixel to autograd over oracle/loss_ref.py by tests/test_loss_ref_cpu.py; used by
tests/test_loss_edges_gpu.py to judge the forward's maps and the backward's dimg separately.
Test infrastructure only.
"""
import torch
import torch.nn.functional as F

from oracle.loss_ref import l1_loss, ssim, window_2d

_C1 = 0.01 ** 2
_C2 = 0.03 ** 2


def loss_maps(img, gt, lam):
    """img, gt: [C,H,W] CPU tensors of one dtype.  Returns a dict in that dtype: loss, l1, ssim
    (scalars), maps [3,C,H,W] = (G1, G11, G12), dimg [C,H,W], S [C,H,W]."""
    C, H, W = img.shape
    n = C * H * W
    w = window_2d(11, C, img)

    def blur(t):
        return F.conv2d(t.unsqueeze(0), w, padding=5, groups=C).squeeze(0)

    x, y = img, gt
    m1, m2, e11, e22, e12 = blur(x), blur(y), blur(x * x), blur(y * y), blur(x * y)
    m1s, m2s, m12 = m1 * m1, m2 * m2, m1 * m2
    A = 2 * m12 + _C1
    B = 2 * (e12 - m12) + _C2
    Cd = m1s + m2s + _C1
    Dd = (e11 - m1s) + (e22 - m2s) + _C2
    S = A * B / (Cd * Dd)
    dm1 = 2 * m2 * (B - A) / (Cd * Dd) - 2 * m1 * S * (1 / Cd - 1 / Dd)
    de11 = -S / Dd
    de12 = 2 * A / (Cd * Dd)
    k = -lam / n
    maps = torch.stack([k * dm1, k * de11, k * de12], 0)
    dimg = blur(maps[0]) + 2 * x * blur(maps[1]) + y * blur(maps[2]) + (1 - lam) / n * torch.sign(x - y)
    l1 = (x - y).abs().mean()
    s = S.mean()
    return dict(loss=(1 - lam) * l1 + lam * (1 - s), l1=l1, ssim=s, maps=maps, dimg=dimg, S=S)


def autograd_reference(img, gt, lam):
    """(loss, dLoss/dimg) by autograd over oracle/loss_ref.py in float64."""
    x = img.double().clone().requires_grad_(True)
    y = gt.double()
    loss = (1 - lam) * l1_loss(x, y) + lam * (1 - ssim(x, y))
    loss.backward()
    return loss.detach(), x.grad


KINDS = ("random", "equal", "const", "both_black", "black_vs_random", "out_of_range", "checker_vs_inverse", "smooth")


def make_inputs(kind, C, H, W, seed=None):
    """(img, gt) float32 CPU tensors of one input kind.  `random` is the construction of
    tests/test_loss_gpu.py; `impulse@y,x` is gt plus 0.5 at one pixel of every channel."""
    g = torch.Generator().manual_seed(H * W if seed is None else seed)
    img = torch.rand((C, H, W), generator=g)
    gt = img * 0.7 + 0.3 * torch.rand((C, H, W), generator=g)
    if kind == "random":
        return img, gt
    if kind == "equal":
        return img, img.clone()
    if kind == "const":
        return torch.full((C, H, W), 0.5), torch.full((C, H, W), 0.25)
    if kind == "both_black":
        return torch.zeros((C, H, W)), torch.zeros((C, H, W))
    if kind == "black_vs_random":
        return torch.zeros((C, H, W)), gt
    if kind == "out_of_range":
        return img * 2.5 - 0.5, gt
    if kind == "checker_vs_inverse":
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        ck = ((yy + xx) % 2).float().expand(C, H, W).contiguous()
        return ck, 1.0 - ck
    if kind == "smooth":
        ramp = (torch.arange(W, dtype=torch.float32) / max(W - 1, 1)).expand(C, H, W).contiguous()
        return ramp, 0.9 * ramp + 0.05
    if kind.startswith("impulse@"):
        py, px = (int(v) for v in kind[len("impulse@"):].split(","))
        x = gt.clone()
        x[:, py, px] += 0.5
        return x, gt
    raise ValueError(kind)
