"""Fused L1+SSIM loss (rain_amd/csrc/loss.hip) per pixel against tests/loss_maps_ref.py: tile edges,
image sizes below the window, channel counts, degenerate inputs, lambda 0 / 1, grad_loss, and the
fixed-order reduction at more than 4096 block partials.

Every case goes through run_native(): the C ABI called as rain_amd/loss.py calls it, on buffers the
test owns.  dimg and the WHOLE workspace are NaN before each call, so a pixel or a partial the kernels
do not write shows as NaN (torch.empty would hand back the previous call's correct answer).  Both
entries run (rl_l1_ssim_forward + rl_l1_ssim_backward, and rl_l1_ssim_forward_backward) and must
agree bitwise.

Comparison rule, per pixel, for dimg and for each of the three workspace maps G1, G11, G12:
    max|got - g64| <= K * max(E32, 2^-23 max|g64|),   E32 = max|g32 - g64|
with g64 the float64 reference and g32 the same reference evaluated in float32 on the CPU (121-term
conv2d sums; the kernel sums 11 + 11 products).  The bound is the reference's own rounding, K the
margin for a different summation order; one K for the module.  Inputs whose true gradient is
rounding noise (identical images, both black) are bounded by K * the unit of the `random` case at
the same shape.  Measured ratios max|got - g64| / unit for every case on an MI355X are in
profiles/loss_edges_margins.txt (set RAIN_LOSS_MARGINS=<file> to write the table again).

The bars of tests/test_loss_gpu.py hold as well: loss and parts[2] within 2e-6 |ref| + 1e-7, and
aggregate relative L1 < 1e-4 wherever sum|g64| > 0.
"""
import os
from functools import lru_cache

import pytest
import torch

from rain_amd import _native as N
from rain_amd.loss import _window_host
from tests.loss_maps_ref import KINDS, loss_maps, make_inputs

pytestmark = pytest.mark.gpu

K = 4  # see profiles/loss_edges_margins.txt; may not exceed 16, the same for every case
FLOOR = 2.0 ** -23
QUANT = ("G1", "G11", "G12", "dimg")

# (H, W): every width of {1, 5, 6, 10, 11, 59, 63, 64, 65, 69, 70, 74, 75, 128, 129, 133} (one side of the
# 64-column tile; the 5-pixel halo exactly filling or spilling the second chunk of the 74-wide patch
# row) and every height of {1, 5, 6, 11, 27, 31, 32, 33, 37, 38, 42, 43, 64, 65} (the 32-row band +- the
# halo), sizes below the 11x11 window, odd 3 H W (float2 partials on a 4-byte boundary), and one
# shape of many bands.
SHAPES = [(1, 1), (1, 133), (1, 64), (5, 5), (6, 6), (5, 74), (11, 10), (11, 11), (6, 129), (27, 59), (31, 63),
          (32, 64), (32, 65), (33, 64), (33, 65), (37, 69), (37, 70), (37, 75), (38, 74), (38, 63), (42, 70),
          (42, 128), (43, 75), (64, 128), (65, 129), (65, 1), (64, 5), (43, 133), (33, 11), (330, 70)]
KIND_SHAPES = [(37, 70), (33, 65)]
# (C, H, W) by number of block partials nb = C ceil(W/64) ceil(H/32): 1024 (the tail loop alone),
# 1025, 4097 (the 4x-unrolled body entered by thread 0 alone), 7170 (the body twice for some threads)
REDUCTION_SHAPES = [(1, 1, 65473), (1, 1, 65537), (1, 1, 262145), (3, 1, 152900)]


def _record(case, what, ratio):
    line = f"{case:44s} {what:5s} {ratio:8.3f}"
    print(line)
    path = os.environ.get("RAIN_LOSS_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_native(gpu, img, gt, lam, scale=None, one_call=False):
    """One forward + backward through the C ABI on NaN-filled outputs.  img, gt: float32 [C,H,W]
    (CPU or device).  Returns CPU tensors: loss [], parts [3], maps [3,C,H,W], dimg [C,H,W]."""
    L = N.loss_lib()
    img = img.to(gpu).contiguous()
    gt = gt.to(gpu).contiguous()
    assert img.dtype == gt.dtype == torch.float32 and img.shape == gt.shape and img.dim() == 3
    C, H, W = img.shape
    n = C * H * W
    nbytes = L.rl_workspace_bytes(C, H, W)
    ws = torch.full(((nbytes + 3) // 4,), float("nan"), dtype=torch.float32, device=gpu)
    assert ws.numel() * 4 >= nbytes >= 12 * n
    dimg = torch.full((C, H, W), float("nan"), dtype=torch.float32, device=gpu)
    loss = torch.full((), float("nan"), dtype=torch.float32, device=gpu)
    parts = torch.full((3,), float("nan"), dtype=torch.float32, device=gpu)
    g = torch.tensor([1.0 if scale is None else scale], dtype=torch.float32, device=gpu)
    st = N.stream_of(img)
    win = _window_host()
    if one_call:
        rc = L.rl_l1_ssim_forward_backward(img.data_ptr(), gt.data_ptr(), C, H, W, float(lam), win, ws.data_ptr(),
                                           ws.numel() * 4, loss.data_ptr(), parts.data_ptr(), g.data_ptr(),
                                           dimg.data_ptr(), st)
        assert rc == 0, L.rl_last_error().decode()
    else:
        rc = L.rl_l1_ssim_forward(img.data_ptr(), gt.data_ptr(), C, H, W, float(lam), win, ws.data_ptr(),
                                  ws.numel() * 4, loss.data_ptr(), parts.data_ptr(), st)
        assert rc == 0, L.rl_last_error().decode()
        rc = L.rl_l1_ssim_backward(img.data_ptr(), gt.data_ptr(), C, H, W, float(lam), win, ws.data_ptr(),
                                   g.data_ptr(), dimg.data_ptr(), st)
        assert rc == 0, L.rl_last_error().decode()
    torch.cuda.synchronize()
    return dict(loss=loss.cpu(), parts=parts.cpu(), maps=ws[:3 * n].view(3, C, H, W).cpu(), dimg=dimg.cpu())


def run_both(gpu, img, gt, lam, scale=None):
    """Both entries; every pixel of the maps and of dimg written by each, and the one-call entry
    bitwise the two calls.  Returns the two-call result."""
    two = run_native(gpu, img, gt, lam, scale, one_call=False)
    one = run_native(gpu, img, gt, lam, scale, one_call=True)
    for name, r in (("two calls", two), ("one call", one)):
        assert not torch.isnan(r["maps"]).any(), f"{name}: workspace map pixels not written"
        assert not torch.isnan(r["dimg"]).any(), f"{name}: dimg pixels not written"
        assert not torch.isnan(r["loss"]).any() and not torch.isnan(r["parts"]).any(), f"{name}: loss is NaN"
    for key in ("loss", "parts", "maps", "dimg"):
        assert torch.equal(_bits(two[key]), _bits(one[key])), f"forward_backward differs from the two calls in {key}"
    return two


@lru_cache(maxsize=None)
def reference(kind, C, H, W, lam):
    """(img, gt, r64, r32, units): the float64 reference, the same in float32, and for each quantity
    the comparison unit max(E32, 2^-23 max|g64|).  Computed once per case, never modified."""
    img, gt = make_inputs(kind, C, H, W)
    r64 = loss_maps(img.double(), gt.double(), lam)
    r32 = loss_maps(img, gt, lam)
    units = {}
    for i, q in enumerate(QUANT):
        a64 = r64["dimg"] if q == "dimg" else r64["maps"][i]
        a32 = r32["dimg"] if q == "dimg" else r32["maps"][i]
        e32 = float((a32.double() - a64).abs().max())
        units[q] = max(e32, FLOOR * float(a64.abs().max()))
    return img, gt, r64, r32, units


def check_pixels(case, got, r64, units, dimg_unit=None):
    """The per-pixel rule for the three maps and for dimg (dimg_unit: the unit of another case, for
    inputs whose true gradient is rounding noise)."""
    fails = []
    for i, q in enumerate(QUANT):
        a64 = r64["dimg"] if q == "dimg" else r64["maps"][i]
        a = got["dimg"] if q == "dimg" else got["maps"][i]
        unit = units[q] if dimg_unit is None or q != "dimg" else dimg_unit
        err = float((a.double() - a64).abs().max())
        ratio = err / unit if unit > 0 else (0.0 if err == 0 else float("inf"))
        _record(case, q, ratio)
        if not ratio <= K:
            at = tuple(int(v) for v in torch.unravel_index((a.double() - a64).abs().argmax(), a.shape))
            fails.append(f"{q}: max|got - g64| = {err:.3e} at {at} is {ratio:.2f} units of {unit:.3e} (K = {K})")
    assert not fails, f"{case}: " + "; ".join(fails)


def check_bars(case, got, r64, aggregate=True):
    """The bars of tests/test_loss_gpu.py: loss, L1 and mean SSIM within 2e-6 |ref| + 1e-7 and the
    aggregate relative L1 of dimg < 1e-4 (where sum|g64| > 0).  Recorded as error / bar."""
    fails = []
    for q, g, ref in (("loss", got["loss"], r64["loss"]), ("loss", got["parts"][0], r64["loss"]),
                      ("l1", got["parts"][1], r64["l1"]), ("ssim", got["parts"][2], r64["ssim"])):
        err, bar = abs(float(g) - float(ref)), 2e-6 * abs(float(ref)) + 1e-7
        _record(case, q, err / bar)
        if not err <= bar:
            fails.append(f"{q}: got {float(g):.9g}, reference {float(ref):.9g}, error {err:.3e} > {bar:.3e}")
    tot = float(r64["dimg"].abs().sum())
    if aggregate and tot > 0:
        rel = float((got["dimg"].double() - r64["dimg"]).abs().sum() / tot)
        _record(case, "relL1", rel / 1e-4)
        if not rel < 1e-4:
            fails.append(f"aggregate relative L1 of dimg {rel:.3e} >= 1e-4")
    assert not fails, f"{case}: " + "; ".join(fails)


def check(case, got, r64, units):
    check_pixels(case, got, r64, units)
    check_bars(case, got, r64)


@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_per_pixel(gpu, H, W):
    img, gt, r64, _, units = reference("random", 3, H, W, 0.2)
    check(f"random 3x{H}x{W}", run_both(gpu, img, gt, 0.2), r64, units)


def test_shape_list_covers_the_tile_geometry():
    assert len(SHAPES) <= 40 and len(set(SHAPES)) == len(SHAPES)
    assert {1, 5, 6, 10, 11, 59, 63, 64, 65, 69, 70, 74, 75, 128, 129, 133} <= {w for _, w in SHAPES}
    assert {1, 5, 6, 11, 27, 31, 32, 33, 37, 38, 42, 43, 64, 65} <= {h for h, _ in SHAPES}
    assert {(1, 1), (33, 65), (37, 75), (330, 70)} <= set(SHAPES)
    assert sum((3 * h * w) % 2 for h, w in SHAPES) >= 3


@pytest.mark.parametrize("H,W", [(11, 11), (33, 65)])
@pytest.mark.parametrize("C", [1, 4])
def test_channel_counts(gpu, C, H, W):
    img, gt, r64, _, units = reference("random", C, H, W, 0.2)
    check(f"random {C}x{H}x{W}", run_both(gpu, img, gt, 0.2), r64, units)


def test_channels_are_independent(gpu):
    """C = 4: perturbing channel 0 leaves the other three channels' maps and dimg bitwise unchanged."""
    img, gt, _, _, _ = reference("random", 4, 33, 65, 0.2)
    a = run_both(gpu, img, gt, 0.2)
    img2 = img.clone()
    img2[0] = 1.0 - img2[0]
    b = run_both(gpu, img2, gt, 0.2)
    assert torch.equal(_bits(a["dimg"][1:]), _bits(b["dimg"][1:]))
    assert torch.equal(_bits(a["maps"][:, 1:]), _bits(b["maps"][:, 1:]))
    assert not torch.equal(a["dimg"][0], b["dimg"][0])


def _impulses(H, W):
    pts = [(0, 0), (H - 1, W - 1), (31, 63), (32, 64), (H // 2, W // 2)]
    return [f"impulse@{y},{x}" for y, x in dict.fromkeys(pts) if y < H and x < W]


GRADIENT_KINDS = [k for k in KINDS if k not in ("equal", "both_black")]
IMPULSES = [(H, W, kind) for H, W in KIND_SHAPES for kind in _impulses(H, W)]


@pytest.mark.parametrize("H,W", KIND_SHAPES)
@pytest.mark.parametrize("kind", GRADIENT_KINDS)
def test_input_kinds_per_pixel(gpu, kind, H, W):
    img, gt, r64, _, units = reference(kind, 3, H, W, 0.2)
    check_pixels(f"{kind} 3x{H}x{W}", run_both(gpu, img, gt, 0.2), r64, units)


@pytest.mark.parametrize("H,W", KIND_SHAPES)
@pytest.mark.parametrize("kind", GRADIENT_KINDS)
def test_input_kinds_loss_and_aggregate_bars(gpu, kind, H, W):
    """`const` and `smooth` are the cases that made the forward take its second moments about a
    per-lane origin: with E[x^2] - m^2 formed from O(1) sums, every interior pixel of such an image
    rounds the same way against C2 = 9e-4 and the mean SSIM was off by 2.6e-6 (const) and 8.5e-6
    (smooth, loss 1.7e-6 against a bar of 1.55e-7); the float32 conv2d reference is off by as much
    or more.  Now 0.05 - 0.14 of the bars (profiles/loss_edges_margins.txt)."""
    img, gt, r64, _, _ = reference(kind, 3, H, W, 0.2)
    check_bars(f"{kind} 3x{H}x{W}", run_both(gpu, img, gt, 0.2), r64)


@pytest.mark.parametrize("H,W,kind", IMPULSES)
def test_impulse_per_pixel(gpu, H, W, kind):
    """gt + 0.5 at one pixel: a 21x21 gradient footprint, placed at the corners, either side of the
    tile seam (31,63) / (32,64), and the centre."""
    img, gt, r64, _, units = reference(kind, 3, H, W, 0.2)
    check_pixels(f"{kind} 3x{H}x{W}", run_both(gpu, img, gt, 0.2), r64, units)


@pytest.mark.parametrize("H,W,kind", IMPULSES)
def test_impulse_loss_and_aggregate_bars(gpu, H, W, kind):
    """The images are identical except at one pixel, so outside the footprint the true gradient is
    zero and whatever the kernel leaves there is summed over every pixel and divided by the
    footprint's sum|g64| alone (a quarter footprint in a corner).  This is the case that made the
    backward blur G12 + 2 G11 instead of G12: blurring G12 and G11 apart left 1.1 - 1.34e-4 at the
    corners, now 0.29 - 0.38e-4 (profiles/loss_edges_margins.txt)."""
    img, gt, r64, _, _ = reference(kind, 3, H, W, 0.2)
    check_bars(f"{kind} 3x{H}x{W}", run_both(gpu, img, gt, 0.2), r64)


@pytest.mark.parametrize("H,W", KIND_SHAPES)
def test_equal_images_gradient_is_noise(gpu, H, W):
    """True gradient ~ 0 (and sign(0) = 0): what the kernel leaves is bounded by the rounding unit
    of an ordinary gradient at this shape."""
    rnd_units = reference("random", 3, H, W, 0.2)[4]
    img, gt, r64, _, units = reference("equal", 3, H, W, 0.2)
    got = run_both(gpu, img, gt, 0.2)
    check_pixels(f"equal 3x{H}x{W}", got, r64, units, dimg_unit=rnd_units["dimg"])
    check_bars(f"equal 3x{H}x{W}", got, r64, aggregate=False)
    assert abs(float(got["loss"])) <= 1e-6


@pytest.mark.parametrize("H,W", KIND_SHAPES)
def test_both_black(gpu, H, W):
    """m1 = m2 = 0: G1 is 0, and G11, G12 are multiplied by x = y = 0: dimg is exactly 0."""
    rnd_units = reference("random", 3, H, W, 0.2)[4]
    img, gt, r64, _, units = reference("both_black", 3, H, W, 0.2)
    got = run_both(gpu, img, gt, 0.2)
    check_pixels(f"both_black 3x{H}x{W}", got, r64, units, dimg_unit=rnd_units["dimg"])
    check_bars(f"both_black 3x{H}x{W}", got, r64, aggregate=False)
    assert torch.equal(got["dimg"], torch.zeros_like(got["dimg"]))
    assert abs(float(got["loss"])) <= 1e-6


@pytest.mark.parametrize("H,W", KIND_SHAPES)
def test_lambda_zero_is_pure_l1(gpu, H, W):
    """lambda = 0: dimg is sign(x - y) float32((1 - 0) float32(1/n)) and the three maps are zeros."""
    img, gt, r64, _, _ = reference("random", 3, H, W, 0.0)
    got = run_both(gpu, img, gt, 0.0)
    c = torch.tensor(1.0 / (3 * H * W), dtype=torch.float32)
    assert torch.equal(got["dimg"], torch.sign(img - gt) * c)
    assert torch.equal(got["maps"], torch.zeros_like(got["maps"]))
    ref_loss = float(r64["loss"])
    assert abs(float(got["loss"]) - ref_loss) <= 2e-6 * abs(ref_loss) + 1e-7


@pytest.mark.parametrize("H,W", KIND_SHAPES)
def test_lambda_one_per_pixel(gpu, H, W):
    img, gt, r64, _, units = reference("random", 3, H, W, 1.0)
    check(f"random lambda=1 3x{H}x{W}", run_both(gpu, img, gt, 1.0), r64, units)


@pytest.mark.parametrize("H,W", KIND_SHAPES)
def test_grad_loss_scale(gpu, H, W):
    """grad_loss = 2.5 gives the unscaled dimg times 2.5 within 1 ulp per pixel; maps and loss do
    not depend on it."""
    img, gt, _, _, _ = reference("random", 3, H, W, 0.2)
    a = run_both(gpu, img, gt, 0.2)
    b = run_both(gpu, img, gt, 0.2, scale=2.5)
    want = a["dimg"].double() * 2.5
    ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want)[1] - 24)
    assert bool(((b["dimg"].double() - want).abs() <= ulp).all())
    assert torch.equal(_bits(a["maps"]), _bits(b["maps"])) and torch.equal(_bits(a["loss"]), _bits(b["loss"]))


@pytest.mark.parametrize("C,H,W", REDUCTION_SHAPES)
def test_reduction_over_many_partials(gpu, C, H, W):
    """More than 1024 / 4096 block partials: loss and parts against float64 (one lost partial of
    4097 is 2.4e-4 relative, 100x the bar), dimg per pixel, and the one-wave finalize of
    rl_l1_ssim_forward_backward bitwise the 1024-thread kernel (run_both)."""
    nb = C * ((W + 63) // 64) * ((H + 31) // 32)
    assert nb in (1024, 1025, 4097, 7170)
    img, gt, r64, _, units = reference("random", C, H, W, 0.2)
    check(f"random {C}x{H}x{W} nb={nb}", run_both(gpu, img, gt, 0.2), r64, units)


def test_wrappers_refuse_another_device_and_match_the_abi(gpu):
    """rain_amd/loss.py: a gt or workspace on another device is refused by name, and a valid call
    gives bitwise what the C ABI gives on the test's own buffers."""
    from rain_amd.loss import fused_l1_ssim_loss, l1_ssim_backward, l1_ssim_forward, l1_ssim_forward_backward

    img, gt, _, _, _ = reference("random", 3, 33, 65, 0.2)
    x, y = img.to(gpu), gt.to(gpu)
    for call in (lambda a, b: l1_ssim_forward(a, b, 0.2), lambda a, b: l1_ssim_forward_backward(a, b, 0.2),
                 lambda a, b: fused_l1_ssim_loss(a, b, 0.2)):
        with pytest.raises(RuntimeError, match="gt must be on img's device"):
            call(x, gt)
        with pytest.raises(RuntimeError, match="img must be on a HIP device"):
            call(img, y)
    loss, parts, ws = l1_ssim_forward(x, y, 0.2)
    with pytest.raises(RuntimeError, match="l1_ssim_backward: gt must be on img's device"):
        l1_ssim_backward(x, gt, 0.2, ws)
    with pytest.raises(RuntimeError, match="l1_ssim_backward: ws must be on img's device"):
        l1_ssim_backward(x, y, 0.2, ws.cpu())
    with pytest.raises(RuntimeError, match="l1_ssim_backward: ws must be a contiguous workspace"):
        l1_ssim_backward(x, y, 0.2, ws[:-1])
    dimg = l1_ssim_backward(x, y, 0.2, ws)
    loss2, parts2, dimg2 = l1_ssim_forward_backward(x, y, 0.2)
    ref = run_native(gpu, img, gt, 0.2)
    for got in ((loss, parts, dimg), (loss2, parts2, dimg2)):
        for g, key in zip(got, ("loss", "parts", "dimg")):
            assert torch.equal(_bits(g.cpu()), _bits(ref[key])), key
