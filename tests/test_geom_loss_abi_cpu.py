"""CPU checks of the geometry loss's surface: librain_loss.so exports the rl_geom_* symbols that
include/rain_loss.h declares, the Python layers exist with the documented signatures, CPU tensors
are refused, and every argument error comes back as a code + message before any device work (the
pointers below are stand-ins)."""
import ctypes
import inspect
import os

import pytest
import torch

from rain_amd import _native as N
from rain_amd import loss as loss_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = ["rl_geom_workspace_bytes", "rl_geom_forward", "rl_geom_backward", "rl_geom_forward_backward"]


def test_symbols_exported_declared_and_listed():
    so = ctypes.CDLL(N.LOSS_LIB)
    header = open(os.path.join(ROOT, "include", "rain_loss.h")).read()
    for name in GEOM:
        assert hasattr(so, name), f"librain_loss.so does not export {name}"
        assert name in N.LOSS_SYMBOLS
        assert f"{name}(" in header
    L = N.loss_lib()
    assert len(L.rl_geom_forward.argtypes) == 16
    assert len(L.rl_geom_backward.argtypes) == 17
    assert len(L.rl_geom_forward_backward.argtypes) == 20


def test_workspace_size():
    L = N.loss_lib()
    assert L.rl_geom_workspace_bytes(0, 5) == 0 and L.rl_geom_workspace_bytes(5, -1) == 0
    assert L.rl_geom_workspace_bytes(3, 3) >= 7 * 9 * 4
    assert L.rl_geom_workspace_bytes(1080, 1920) >= 7 * 1080 * 1920 * 4
    assert L.rl_geom_workspace_bytes(1080, 1920) < 8 * 1080 * 1920 * 4


def test_python_surface_exists():
    for name in ("geometry_loss_forward", "geometry_loss_backward", "geometry_loss_forward_backward",
                 "fused_geometry_loss"):
        assert callable(getattr(loss_mod, name))
    p = inspect.signature(loss_mod.fused_geometry_loss).parameters
    assert list(p) == ["depth", "alpha", "normal", "tanfovx", "tanfovy", "lambda_normal", "lambda_depth", "gt_depth",
                       "alpha_min"]
    assert p["lambda_depth"].default == 0.0 and p["gt_depth"].default is None and p["alpha_min"].default == 0.1
    from rain_amd.gaussian_model import OptimizationParams

    opt = OptimizationParams()
    assert opt.lambda_normal == 0.0 and opt.lambda_normal_from_iter == 7000
    assert OptimizationParams(lambda_normal=0.05).lambda_normal == 0.05


def test_cpu_tensors_are_refused():
    D, A, Nm = torch.ones(1, 4, 5), torch.ones(1, 4, 5), torch.zeros(3, 4, 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        loss_mod.fused_geometry_loss(D, A, Nm, 0.5, 0.4)
    with pytest.raises(RuntimeError, match="HIP device"):
        loss_mod.fused_l1_ssim_loss(torch.zeros(3, 4, 5), torch.zeros(3, 4, 5))
    for fn in (loss_mod.geometry_loss_forward, loss_mod.geometry_loss_forward_backward):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(D, A, Nm, 0.5, 0.4, 0.05)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_mod.geometry_loss_backward(D, A, Nm, 0.5, 0.4, 0.05, 0.0, None, 0.1, torch.zeros(8, dtype=torch.uint8))


def test_validation_errors_without_gpu():
    L = N.loss_lib()
    H, W = 6, 8
    big = 1 << 20
    base = dict(D=1, A=1, N=1, gt=1, H=H, W=W, ln=0.05, ld=0.5, ws=1, wsb=big, loss=1, parts=1, gl=1, dD=1, dA=1, dN=1)

    def head(a):
        return (a["D"], a["A"], a["N"], a["gt"], a["H"], a["W"], 0.5, 0.4, 0.1, a["ln"], a["ld"])

    def fwd(**kw):
        a = dict(base, **kw)
        return L.rl_geom_forward(*head(a), a["ws"], a["wsb"], a["loss"], a["parts"], None)

    def bwd(**kw):
        a = dict(base, **kw)
        return L.rl_geom_backward(*head(a), a["ws"], a["gl"], a["dD"], a["dA"], a["dN"], None)

    def both(**kw):
        a = dict(base, **kw)
        return L.rl_geom_forward_backward(*head(a), a["ws"], a["wsb"], a["loss"], a["parts"], a["gl"], a["dD"],
                                          a["dA"], a["dN"], None)

    def err():
        return L.rl_last_error()

    for call, who in ((fwd, b"rl_geom_forward:"), (bwd, b"rl_geom_backward:"), (both, b"rl_geom_forward_backward:")):
        for kw in (dict(D=None), dict(A=None), dict(ws=None)):
            assert call(**kw) == 1 and err().startswith(who) and b"null" in err(), (who, kw, err())
        for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(W=-1)):
            assert call(**kw) == 1 and err().startswith(who) and b"positive" in err(), (who, kw, err())
        assert call(N=None) == 1 and err().startswith(who) and b"lambda_normal" in err()
        assert call(gt=None) == 1 and err().startswith(who) and b"lambda_depth" in err()
    for call in (fwd, both):
        assert call(wsb=L.rl_geom_workspace_bytes(H, W) - 1) == 3 and b"workspace too small" in err()
        assert call(wsb=0) == 3
        assert call(loss=None) == 1 and b"null" in err()
    for call in (bwd, both):
        for kw in (dict(gl=None), dict(dD=None), dict(dA=None), dict(dN=None)):
            assert call(**kw) == 1 and b"null" in err(), kw
