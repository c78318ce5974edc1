"""CPU checks of rain_amd/_raster_driver.py, the one home of the render ABI's call protocols: a stand-in
library records (name, args) and returns scripted codes, the tensors are CPU tensors and the stream is None.
Argument counts are compared with the argtypes of the real library."""
import ctypes
import itertools

import pytest
import torch

from rain_amd import _native as N
from rain_amd import _raster_driver as driver
from rain_amd import fused, sharded
from rain_amd.diff_gaussian_rasterization import _C

P, W, H = 300, 64, 48
QUERIES = {"rr_camera_grad_scratch_bytes": 4242, "rr_backward_workspace_bytes": 1234, "rr_binning_bytes": 7777}


class StandIn:
    """Records every call; an entry point returns the next scripted code (0 when the script is over) after
    filling its `need` / pair-count outputs, a size query its QUERIES value."""

    def __init__(self, codes=(), need=0, num_rendered=11, num_pairs=7):
        self.calls, self.codes = [], list(codes)
        self.need, self.num_rendered, self.num_pairs = need, num_rendered, num_pairs

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name in QUERIES:
                return QUERIES[name]
            outs = {"rr_forward": (10, 11, 12), "rr_forward_from_geometry": (9, 10, 11),
                    "rr_forward_geometry": (8, 9, None)}.get(name)
            if outs is not None:
                args[outs[0]]._obj.value, args[outs[1]]._obj.value = self.num_rendered, self.num_pairs
                if outs[2] is not None:
                    args[outs[2]]._obj.value = self.need
            return self.codes.pop(0) if self.codes else 0

        return call

    def entries(self):
        return [(n, a) for n, a in self.calls if n not in QUERIES]


def _check_count(name, args):
    assert len(args) == len(getattr(N.raster(), name).argtypes), name


def _value(p):
    """The address in a c_void_p argument (None: NULL); a plain number as it is."""
    return p.value if isinstance(p, ctypes.c_void_p) else p


def _frame_parts():
    frame = N.RRFrame(P, 0, 1, W, H, 0.5, 0.4, 1.0, 0.3, 0, 0, N.RR_FLAG_RAW_PARAMS)
    _keep, cam = driver.camera_block(torch.zeros(3), torch.eye(4), torch.eye(4), torch.zeros(3))
    gs = driver.raw_gaussians(torch.zeros(P, 3), torch.zeros(P, 1, 3), torch.zeros(P, 1), torch.zeros(P, 3),
                              torch.zeros(P, 4), torch.zeros(P, 0, 3))
    bufs = dict(radii=torch.zeros(P, dtype=torch.int32), geom=torch.zeros(64, dtype=torch.uint8),
                img=torch.zeros(32, dtype=torch.uint8))
    return frame, cam, gs, bufs


MAPS = dict(dL_ddepth=torch.zeros(1, H, W), dL_dalpha=torch.zeros(1, H, W), dL_dnormal=torch.zeros(3, H, W),
            dL_dmoments=torch.zeros(2, H, W))
PATTERNS = list(itertools.product((False, True), repeat=4))  # (depth, alpha, normal, moments) present
# all 16 without the camera gradients; with them the four the driver's callers do not refuse
CASES = [(p, False) for p in PATTERNS] + [(p, True) for p in PATTERNS if not (p[2] or p[3])]


@pytest.mark.parametrize("present,camera", CASES, ids=["".join("danm"[i] if b else "-" for i, b in enumerate(p)) +
                                                       ("+camera" if c else "") for p, c in CASES])
def test_backward_dispatch(present, camera):
    frame, cam, gs, b = _frame_parts()
    maps = [t if on else None for t, on in zip(MAPS.values(), present)]
    dpix, binning = torch.zeros(3, H, W), torch.zeros(16, dtype=torch.uint8)
    ws, grads = torch.zeros(QUERIES["rr_backward_workspace_bytes"], dtype=torch.uint8), N.RRGrads()
    cg = (torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(3)) if camera else None
    L = StandIn()
    driver.backward(L, frame, cam, gs, b["radii"], b["geom"], b["img"], binning, 5, dpix, *maps, (0.25, 9.0), ws,
                    grads, cg, None, "label")
    (name, args), = L.entries()
    _check_count(name, args)
    assert name == ("rr_backward_camera" if camera else "rr_backward_aux_dist" if any(present) else "rr_backward")
    assert [_value(a) for a in args[3:9]] == [b["radii"].data_ptr(), b["geom"].data_ptr(), b["img"].data_ptr(),
                                              binning.data_ptr(), 5, dpix.data_ptr()]
    n_maps = 2 if camera else 4 if any(present) else 0
    assert [_value(a) for a in args[9:9 + n_maps]] == [None if m is None else m.data_ptr() for m in maps[:n_maps]]
    tail = 9 + n_maps
    if name == "rr_backward_aux_dist":
        assert tuple(args[tail:tail + 2]) == ((0.25, 9.0) if present[3] else (0.0, 0.0))
        tail += 2
    assert (_value(args[tail]), args[tail + 1]) == (ws.data_ptr(), ws.numel()) and args[tail + 2]._obj is grads
    assert args[-1] is None  # the stream
    if camera:
        assert [n for n, _ in L.calls] == ["rr_camera_grad_scratch_bytes", "rr_backward_camera"]
        assert L.calls[0][1] == (P,)
        out = args[tail + 3]._obj
        assert (out.dL_dviewmatrix, out.dL_dprojmatrix, out.dL_dcampos) == tuple(t.data_ptr() for t in cg)
        assert out.scratch and out.scratch_bytes == QUERIES["rr_camera_grad_scratch_bytes"]
    else:
        assert len(L.calls) == 1


def test_backward_reports_a_failure_with_its_label():
    frame, cam, gs, b = _frame_parts()
    with pytest.raises(RuntimeError, match="^some label: "):
        driver.backward(StandIn(codes=[1]), frame, cam, gs, b["radii"], b["geom"], b["img"], None, 0,
                        torch.zeros(3, H, W), None, None, None, None, None, torch.zeros(8, dtype=torch.uint8),
                        N.RRGrads(), None, None, "some label")


@pytest.mark.parametrize("from_geometry", [False, True], ids=["rr_forward", "rr_forward_from_geometry"])
def test_one_call_render(from_geometry):
    frame, cam, gs, b = _frame_parts()
    first, second = ("rr_forward_from_geometry", "rr_forward_render_geometry") if from_geometry else \
        ("rr_forward", "rr_forward_render")
    color, depth = torch.zeros(3, H, W), torch.zeros(1, H, W)

    def run(L, cache):
        return driver.render_one_call(L, frame, cam, None if from_geometry else gs, b["radii"], b["geom"], b["img"],
                                      cache, color, depth, None, "one call")

    # the first call succeeds: nothing follows it
    cache = driver.BinningCache()
    cache.buf = torch.zeros(100, dtype=torch.uint8)
    L = StandIn()
    binning, num_rendered, num_pairs = run(L, cache)
    (name, args), = L.calls
    _check_count(name, args)
    assert name == first and binning is cache.buf and (num_rendered, num_pairs) == (11, 7)
    i = 3 if from_geometry else 4  # geom, its size, img, its size, binning, its size
    assert [_value(args[i]), args[i + 1], _value(args[i + 2]), args[i + 3], _value(args[i + 4]), args[i + 5]] == \
        [b["geom"].data_ptr(), b["geom"].numel(), b["img"].data_ptr(), b["img"].numel(), cache.buf.data_ptr(), 100]
    # the pairs outgrew the buffer: exactly one stage-2 call on a grown buffer, which the cache keeps
    L = StandIn(codes=[N.RR_INCOMPLETE], need=5000)
    binning, num_rendered, num_pairs = run(L, cache)
    assert [n for n, _ in L.calls] == [first, second]
    name, args = L.calls[1]
    _check_count(name, args)
    j = 5 if from_geometry else 6
    assert binning.numel() >= 5000 and binning is cache.buf
    assert (_value(args[j]), args[j + 1], args[j + 2]) == (binning.data_ptr(), binning.numel(), 7)
    assert (_value(args[j + 3]), _value(args[j + 4]), args[j + 5]) == (color.data_ptr(), depth.data_ptr(), None)
    assert binning.numel() == int(5000 * 1.25) + 4096  # the growth policy
    run(StandIn(), cache)
    assert cache.buf is binning  # large enough now: kept
    # without a cache the stage-2 buffer is allocated to size
    binning, _nr, _np = run(StandIn(codes=[N.RR_INCOMPLETE], need=640), None)
    assert binning.numel() == 640
    # a failed render drops the registration once and raises with the label
    for codes in ([1], [N.RR_INCOMPLETE, 3]):
        L = StandIn(codes=codes, need=9000)
        with pytest.raises(RuntimeError, match="^one call: "):
            run(L, cache)
        assert [n for n, _ in L.calls][len(codes):] == ["rr_set_forward_workspace"]
        assert L.calls[-1][1] == (None, 0)


@pytest.mark.parametrize("dist", [None, (0.5, 20.0)], ids=["aux", "dist"])
def test_counted_render(dist):
    frame, cam, gs, b = _frame_parts()
    color, depth, normal, moments = (torch.zeros(c, H, W) for c in (3, 1, 3, 2))
    L = StandIn()
    binning, num_rendered = driver.render_counted(L, frame, cam, gs, b["radii"], b["geom"], b["img"], None, color,
                                                  depth, normal, moments if dist else None, dist, None, "counted")
    render = "rr_forward_render_dist" if dist else "rr_forward_render_aux"
    assert [n for n, _ in L.calls] == ["rr_forward_geometry", "rr_binning_bytes", render]
    for name, args in L.entries():
        _check_count(name, args)
    assert L.calls[1][1] == (7, W, H)
    assert num_rendered == 11 and binning.numel() == QUERIES["rr_binning_bytes"]
    args = L.calls[2][1]
    assert (_value(args[6]), args[7], args[8]) == (binning.data_ptr(), binning.numel(), 7)
    assert [_value(a) for a in args[9:12]] == [color.data_ptr(), depth.data_ptr(), normal.data_ptr()]
    assert args[12:] == ((args[12], 0.5, 20.0, None) if dist else (None,))
    assert dist is None or args[12].value == moments.data_ptr()
    # no pairs: no size query, an empty buffer; a cache is grown through its policy
    L = StandIn(num_pairs=0)
    binning, _nr = driver.render_counted(L, frame, cam, gs, b["radii"], b["geom"], b["img"], driver.BinningCache(),
                                         color, depth, None, None, None, None, "counted")
    assert [n for n, _ in L.calls] == ["rr_forward_geometry", "rr_forward_render_aux"] and binning.numel() == 0
    assert L.calls[1][1][6] is None and L.calls[1][1][11] is None
    cache = driver.BinningCache()
    binning, _nr = driver.render_counted(StandIn(), frame, cam, gs, b["radii"], b["geom"], b["img"], cache, color,
                                         depth, None, None, None, None, "counted")
    assert binning is cache.buf and binning.numel() == int(QUERIES["rr_binning_bytes"] * 1.25) + 4096
    # a failed geometry stage drops the registration and stops
    L = StandIn(codes=[2])
    with pytest.raises(RuntimeError, match="^counted: "):
        driver.render_counted(L, frame, cam, gs, b["radii"], b["geom"], b["img"], None, color, depth, None, None,
                              None, None, "counted")
    assert [n for n, _ in L.calls] == ["rr_forward_geometry", "rr_set_forward_workspace"]


def test_workspace_registration_and_backward_frame():
    L = StandIn()
    assert driver.register_workspace(L, 0, torch.device("cpu")) is None and L.calls == []
    ws = driver.register_workspace(L, P, torch.device("cpu"))
    assert ws.numel() == QUERIES["rr_backward_workspace_bytes"] and ws.dtype == torch.uint8
    assert [n for n, _ in L.calls] == ["rr_backward_workspace_bytes", "rr_set_forward_workspace"]
    assert (L.calls[1][1][0].value, L.calls[1][1][1]) == (ws.data_ptr(), ws.numel())
    own = torch.zeros(64, dtype=torch.uint8)
    L = StandIn()
    assert driver.register_workspace(L, P, own.device, own) is own
    assert [(n, _value(a[0]), a[1]) for n, a in L.calls] == [("rr_set_forward_workspace", own.data_ptr(), 64)]
    # a backward's flags go on a copy; the forward's frame keeps its own
    frame = N.RRFrame(P, 0, 1, W, H, 0.5, 0.4, 1.0, 0.3, 0, 0, N.RR_FLAG_RAW_PARAMS)
    assert driver.backward_frame(frame, False) is frame
    for registered, flags in ((True, 0), (False, N.RR_FLAG_ABSGRAD), (True, N.RR_FLAG_ABSGRAD)):
        out = driver.backward_frame(frame, registered, flags)
        assert out is not frame and frame.flags == N.RR_FLAG_RAW_PARAMS
        assert out.flags == N.RR_FLAG_RAW_PARAMS | flags | (N.RR_FLAG_WORKSPACE_REGISTERED if registered else 0)
        assert (out.P, out.width, out.height, out.low_pass) == (frame.P, W, H, frame.low_pass)


@pytest.mark.parametrize("M", [1, 4])
def test_raw_gaussians(M):
    n = 5
    t = dict(xyz=torch.zeros(n, 3), f_dc=torch.zeros(n, 1, 3), opacity=torch.zeros(n, 1), scaling=torch.zeros(n, 3),
             rotation=torch.zeros(n, 4), f_rest=torch.zeros(n, M - 1, 3))
    fields = dict(means3D="xyz", shs="f_dc", opacities="opacity", scales="scaling", rotations="rotation",
                  shs_rest="f_rest")
    widths = dict(xyz=12, f_dc=12, opacity=4, scaling=12, rotation=16, f_rest=12 * (M - 1))
    for row in (0, 3):
        gs = driver.raw_gaussians(*t.values(), row) if row else driver.raw_gaussians(*t.values())
        assert gs.colors_precomp is None and gs.cov3D_precomp is None
        for field, name in fields.items():
            if name == "f_rest" and M == 1:
                assert gs.shs_rest is None
            else:
                assert getattr(gs, field) == t[name].data_ptr() + widths[name] * row, (field, row)


def test_camera_block():
    view = torch.arange(16.0).view(4, 4).t()  # not contiguous
    args = (torch.zeros(3), view, torch.eye(4), torch.ones(3))
    keep, cam = driver.camera_block(*args)
    assert all(k.is_contiguous() and torch.equal(k, a) for k, a in zip(keep, args))
    assert keep[0] is args[0] and keep[1] is not view
    assert (cam.background, cam.viewmatrix, cam.projmatrix, cam.campos) == tuple(k.data_ptr() for k in keep)


def test_ptr():
    assert driver.ptr(None) is None and driver.ptr(torch.zeros(0, 3)) is None
    t = torch.zeros(4, 3)
    assert driver.ptr(t).value == t.data_ptr() and driver.ptr(t, 24).value == t.data_ptr() + 24
    assert _C._ptr is fused._p is sharded._p is driver.ptr
    assert fused.BinningCache is driver.BinningCache
    assert fused._register_workspace is driver.register_workspace
