"""CPU checks of the fused L1+SSIM loss's surface: librain_loss.so exports the rl_l1_ssim_* symbols
that include/rain_loss.h declares, every argument error of the C ABI comes back as a code + message
before any device work (the pointers below are stand-ins), and the Python wrappers refuse a gt or
workspace that does not fit img instead of passing raw pointers on."""
import ctypes
import os

import pytest
import torch

from rain_amd import _native as N
from rain_amd import loss as loss_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1SSIM = ["rl_l1_ssim_forward", "rl_l1_ssim_backward", "rl_l1_ssim_forward_backward", "rl_workspace_bytes"]


def nb(C, H, W):
    return C * ((W + 63) // 64) * ((H + 31) // 32)


def test_symbols_exported_declared_and_listed():
    so = ctypes.CDLL(N.LOSS_LIB)
    header = open(os.path.join(ROOT, "include", "rain_loss.h")).read()
    for name in L1SSIM:
        assert hasattr(so, name), f"librain_loss.so does not export {name}"
        assert name in N.LOSS_SYMBOLS
        assert f"{name}(" in header
    L = N.loss_lib()
    assert len(L.rl_workspace_bytes.argtypes) == 3
    assert len(L.rl_l1_ssim_forward.argtypes) == 12
    assert len(L.rl_l1_ssim_backward.argtypes) == 11
    assert len(L.rl_l1_ssim_forward_backward.argtypes) == 14


@pytest.mark.parametrize("C,H,W", [(3, 1, 1), (1, 11, 11), (3, 33, 65), (4, 33, 65), (3, 1, 152900), (1, 1, 262145),
                                   (3, 1080, 1920), (3, 2160, 3840)])
def test_workspace_size(C, H, W):
    L = N.loss_lib()
    got = L.rl_workspace_bytes(C, H, W)
    assert got >= 12 * C * H * W + 8 * nb(C, H, W)
    assert got < 12 * C * H * W + 8 * nb(C, H, W) + 4096  # maps + partials, not a multiple of them


def test_validation_errors_without_gpu():
    L = N.loss_lib()
    C, H, W = 3, 37, 70
    win = loss_mod._window_host()
    base = dict(img=1, gt=1, C=C, H=H, W=W, win=win, ws=1, wsb=1 << 20, loss=1, parts=1, gl=1, dimg=1)

    def fwd(**kw):
        a = dict(base, **kw)
        return L.rl_l1_ssim_forward(a["img"], a["gt"], a["C"], a["H"], a["W"], 0.2, a["win"], a["ws"], a["wsb"],
                                    a["loss"], a["parts"], None)

    def bwd(**kw):
        a = dict(base, **kw)
        return L.rl_l1_ssim_backward(a["img"], a["gt"], a["C"], a["H"], a["W"], 0.2, a["win"], a["ws"], a["gl"],
                                     a["dimg"], None)

    def both(**kw):
        a = dict(base, **kw)
        return L.rl_l1_ssim_forward_backward(a["img"], a["gt"], a["C"], a["H"], a["W"], 0.2, a["win"], a["ws"],
                                             a["wsb"], a["loss"], a["parts"], a["gl"], a["dimg"], None)

    def err():
        return L.rl_last_error()

    calls = ((fwd, b"rl_l1_ssim_forward:"), (bwd, b"rl_l1_ssim_backward:"), (both, b"rl_l1_ssim_forward_backward:"))
    for call, who in calls:
        for kw in (dict(img=None), dict(gt=None), dict(win=None), dict(ws=None)):
            assert call(**kw) == 1 and err().startswith(who) and b"bad argument" in err(), (who, kw, err())
        for kw in (dict(C=0), dict(H=0), dict(W=0), dict(C=-1), dict(H=-3), dict(W=-1)):
            assert call(**kw) == 1 and err().startswith(who) and b"bad argument" in err(), (who, kw, err())
        # one channel plane of 2^30 bytes: past the buffer descriptors' range
        assert call(C=1, H=16384, W=16384, wsb=1 << 62) == 1 and err().startswith(who) and b"2^30" in err(), err()
    for call, who in (calls[0], calls[2]):
        need = L.rl_workspace_bytes(C, H, W)
        assert call(wsb=need - 1) == 3 and err().startswith(who) and b"workspace too small" in err()
        assert call(wsb=0) == 3
        assert call(loss=None) == 1 and b"bad argument" in err()
    for call, who in (calls[1], calls[2]):
        for kw in (dict(gl=None), dict(dimg=None)):
            assert call(**kw) == 1 and err().startswith(who) and b"bad argument" in err(), kw


WRAPPERS = {
    "l1_ssim_forward": lambda img, gt: loss_mod.l1_ssim_forward(img, gt, 0.2),
    "l1_ssim_backward": lambda img, gt: loss_mod.l1_ssim_backward(img, gt, 0.2,
                                                                  torch.zeros(1 << 16, dtype=torch.uint8)),
    "l1_ssim_forward_backward": lambda img, gt: loss_mod.l1_ssim_forward_backward(img, gt, 0.2),
    "fused_l1_ssim_loss": lambda img, gt: loss_mod.fused_l1_ssim_loss(img, gt, 0.2),
}


@pytest.mark.parametrize("name", list(WRAPPERS))
def test_wrappers_refuse_mismatched_arguments(name):
    """Shape and dtype errors are raised before the device is looked at, so CPU tensors reach them."""
    call = WRAPPERS[name]
    x = torch.zeros(3, 8, 9)
    for bad in (torch.zeros(3, 8, 10), torch.zeros(3, 9, 8), torch.zeros(1, 8, 9), torch.zeros(3, 8, 9, 1)):
        with pytest.raises(RuntimeError, match=rf"{name}: gt must have img's shape"):
            call(x, bad)
    for dt in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(RuntimeError, match=rf"{name}: gt must be a float32"):
            call(x, x.to(dt))
        with pytest.raises(RuntimeError, match=rf"{name}: img must be a float32"):
            call(x.to(dt), x)
    with pytest.raises(RuntimeError, match=rf"{name}: img must be a \[C,H,W\]"):
        call(torch.zeros(8, 9), torch.zeros(8, 9))
    with pytest.raises(RuntimeError, match=rf"{name}: img must be one non-empty"):
        call(torch.zeros(3, 0, 9), torch.zeros(3, 0, 9))
    # well-formed CPU tensors: refused for their device, after everything else
    with pytest.raises(RuntimeError, match=rf"{name}: img must be on a HIP device"):
        call(x, x.clone())


def test_leading_dimensions():
    x = torch.zeros(1, 3, 8, 9)
    with pytest.raises(RuntimeError, match=r"fused_l1_ssim_loss: img must be a \[C,H,W\]"):
        loss_mod.fused_l1_ssim_loss(x, x)
    with pytest.raises(RuntimeError, match="HIP device"):  # a leading 1 is accepted by the low-level calls
        loss_mod.l1_ssim_forward(x, x, 0.2)
    with pytest.raises(RuntimeError, match="l1_ssim_forward: img must be one non-empty"):
        loss_mod.l1_ssim_forward(torch.zeros(2, 3, 8, 9), torch.zeros(2, 3, 8, 9), 0.2)


def test_backward_refuses_short_workspace():
    L = N.loss_lib()
    x = torch.zeros(3, 8, 9)
    need = L.rl_workspace_bytes(3, 8, 9)
    with pytest.raises(RuntimeError, match=rf"l1_ssim_backward: ws must be .* at least {need} bytes"):
        loss_mod.l1_ssim_backward(x, x, 0.2, torch.zeros(need - 1, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="l1_ssim_backward: ws must be"):
        loss_mod.l1_ssim_backward(x, x, 0.2, None)
    with pytest.raises(RuntimeError, match="HIP device"):  # long enough: the device is what is left to refuse
        loss_mod.l1_ssim_backward(x, x, 0.2, torch.zeros(need, dtype=torch.uint8))
