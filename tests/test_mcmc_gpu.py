"""GPU tests of the MCMC densification kernels (rain_amd/csrc/mcmc.hip: rt_mcmc_relocate, rt_mcmc_step) against
the float64 reference (tests/mcmc_ref.py) and against rt_adam_step, and of the MCMC training loop on HIP."""
import ctypes
import math

import numpy as np
import pytest
import torch

from rain_amd import _native as N
from rain_amd import cameras, fused
from rain_amd.renderer import PipelineParams
from rain_amd.train import TrainConfig, Trainer
from tests import mcmc_ref as R
from tests.test_mcmc_train_cpu import CAP, check_schedule, make_model, mcmc_opt, run_schedule

pytestmark = pytest.mark.gpu

P_RELOC = 4097  # one past a multiple of the 256-thread blocks; the last row is a destination
FLT_EPSILON = float(np.finfo(np.float32).eps)
WIDTHS = dict(xyz=(3,), f_dc=(1, 3), f_rest=(15, 3), opacity=(1,), scaling=(3,), rotation=(4,))  # M = 16
KINDS = dict(xyz=N.RT_GROUP_XYZ, scaling=N.RT_GROUP_SCALING, opacity=N.RT_GROUP_OPACITY)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- relocation ---------------------------------------------------------------------------------

def _reloc_state(seed=0):
    gen = torch.Generator().manual_seed(seed)
    P = P_RELOC
    prm = {k: torch.randn((P,) + w, generator=gen) for k, w in WIDTHS.items()}
    o = torch.rand(P, 1, generator=gen) * 0.9 + 0.05
    prm["opacity"] = torch.log(o / (1 - o))
    prm["opacity"][13, 0] = float(np.float32(math.log((1.0 - FLT_EPSILON) / FLT_EPSILON)))  # sigmoid: 1 - FLT_EPSILON
    prm["opacity"][17, 0] = -5.0  # sigmoid 0.0067: two copies of it fall below min_opacity (the clamp)
    prm["scaling"] = prm["scaling"] * 0.5 - 2.0
    mom = {k: (torch.rand((P,) + w, generator=gen) - 0.5, torch.rand((P,) + w, generator=gen) + 0.1)
           for k, w in WIDTHS.items()}
    return prm, mom


def _pairs():
    """Row 5 drawn 60 times (over the cap of 51 copies), row 9 once, row 13 (opacity 1 - FLT_EPSILON) three
    times, row 17 (the clamp) once, rows 21..59 step 2 two to four times; destinations: distinct rows from
    2000 on that are no source, ending with the last row."""
    src = [5] * 60 + [9] + [13] * 3 + [17]
    for i, s in enumerate(range(21, 60, 2)):
        src += [s] * (2 + i % 3)
    dst = [2000 + 3 * j for j in range(len(src) - 1)] + [P_RELOC - 1]
    perm = np.random.RandomState(1).permutation(len(src))  # a source's pairs are not adjacent
    return [src[i] for i in perm], [dst[i] for i in perm]


def _relocate(prm, mom, src, dst, min_opacity=0.005, ws_extra=0):
    """rt_mcmc_relocate on device copies; returns ({name: param}, {name: (m, v)} or None) as CPU tensors."""
    L = N.train_lib()
    dp = {k: v.clone().cuda().contiguous() for k, v in prm.items()}
    dm = {k: (m.clone().cuda(), v.clone().cuda()) for k, (m, v) in mom.items()} if mom is not None else None
    structs = []
    for k in dp:
        m, v = dm[k] if dm is not None else (None, None)
        structs.append(N.RTMcmcGroup(dp[k].data_ptr(), m.data_ptr() if m is not None else None,
                                     v.data_ptr() if v is not None else None, math.prod(WIDTHS[k]),
                                     KINDS.get(k, N.RT_GROUP_OTHER)))
    arr = (N.RTMcmcGroup * len(structs))(*structs)
    P = dp["xyz"].shape[0]
    s = torch.tensor(src, dtype=torch.int64, device="cuda")
    d = torch.tensor(dst, dtype=torch.int64, device="cuda")
    ws = torch.empty(L.rt_mcmc_workspace_bytes(P) + ws_extra, dtype=torch.uint8, device="cuda")
    rc = L.rt_mcmc_relocate(P, s.data_ptr() if len(src) else None, d.data_ptr() if len(dst) else None, len(src),
                            min_opacity, arr, len(structs), ws.data_ptr(), ws.numel(), _stream())
    assert rc == 0, L.rt_last_error()
    torch.cuda.synchronize()
    return ({k: v.cpu() for k, v in dp.items()},
            {k: (m.cpu(), v.cpu()) for k, (m, v) in dm.items()} if dm is not None else None)


def _ref_relocate(prm, mom, src, dst, min_opacity=0.005):
    groups = {k: (prm[k].numpy(), mom[k][0].numpy() if mom else None, mom[k][1].numpy() if mom else None)
              for k in prm}
    return R.relocate(groups, src, dst, min_opacity)


def _check_relocation(prm, mom, got_p, got_m, src, dst):
    ref, counts = _ref_relocate(prm, mom, src, dst)
    P = prm["xyz"].shape[0]
    pairs = [(s, d) for s, d in zip(src, dst) if 0 <= s < P and 0 <= d < P]
    srcs = sorted({s for s, _ in pairs})
    dsts = [d for _, d in pairs]
    touched = np.zeros(P, dtype=bool)
    touched[srcs] = True
    touched[dsts] = True
    # activated opacity and scale of every touched row: 1e-5 relative (double in the kernel, one rounding to
    # fp32, then the activation's few ulps)
    act_o = R.sigmoid(got_p["opacity"].numpy().astype(np.float64))[touched]
    ref_o = R.sigmoid(ref["opacity"][0])[touched]
    assert np.all(np.abs(act_o - ref_o) <= 1e-5 * ref_o), np.max(np.abs(act_o - ref_o) / ref_o)
    act_s = np.exp(got_p["scaling"].numpy().astype(np.float64))[touched]
    ref_s = np.exp(ref["scaling"][0])[touched]
    assert np.all(np.abs(act_s - ref_s) <= 1e-5 * ref_s), np.max(np.abs(act_s - ref_s) / ref_s)
    for k in prm:
        g = got_p[k]
        if k not in ("opacity", "scaling"):  # every other field of a destination: bitwise its source's old row
            for s, d in pairs:
                assert torch.equal(g[d], prm[k][s]), (k, s, d)
            assert torch.equal(g[srcs], prm[k][srcs]), k  # and a source keeps its own
        assert torch.equal(g[~touched], prm[k][~touched]), k  # rows that took no part: bitwise unchanged
        if got_m is not None:
            for a, b in zip(got_m[k], mom[k]):
                assert bool((a[touched] == 0).all()), k
                assert torch.equal(a[~touched], b[~touched]), k
    assert bool(all(torch.isfinite(v).all() for v in got_p.values()))
    return counts


def test_relocate_matches_reference(gpu):
    prm, mom = _reloc_state()
    src, dst = _pairs()
    got_p, got_m = _relocate(prm, mom, src, dst)
    counts = _check_relocation(prm, mom, got_p, got_m, src, dst)
    assert counts[5] == 60 and counts[9] == 1 and counts[13] == 3 and dst.count(P_RELOC - 1) == 1
    # 60 draws behave as 50: 51 copies
    on, _D, coeff = R.relocation(R.sigmoid(float(prm["opacity"][5, 0])), 51)
    assert abs(float(torch.sigmoid(got_p["opacity"][5, 0].double())) - on) <= 1e-5 * on
    assert np.allclose(np.exp(got_p["scaling"][5].double().numpy()), np.exp(prm["scaling"][5].double().numpy()) * coeff,
                       rtol=1e-5, atol=0)
    # the clamp: row 17 and its copy sit at min_opacity
    lo = float(np.float32(0.005))
    assert abs(float(torch.sigmoid(got_p["opacity"][17, 0].double())) - lo) <= 1e-5 * lo


def test_relocate_small_calls_and_no_moments(gpu):
    prm, mom = _reloc_state(seed=1)
    got_p, got_m = _relocate(prm, mom, [], [])  # n = 0: nothing launched, nothing changed
    for k in prm:
        assert torch.equal(got_p[k], prm[k]) and torch.equal(got_m[k][0], mom[k][0])
    got_p, got_m = _relocate(prm, mom, [9], [P_RELOC - 1])  # n = 1: two copies
    _check_relocation(prm, mom, got_p, got_m, [9], [P_RELOC - 1])
    src, dst = _pairs()
    got_p, got_m = _relocate(prm, None, src, dst, ws_extra=64)  # no optimizer state yet
    assert got_m is None
    _check_relocation(prm, None, got_p, None, src, dst)


def test_relocate_skips_out_of_range_pairs(gpu):
    prm, mom = _reloc_state(seed=2)
    src = [5, P_RELOC, 9, -1, 5, 30]
    dst = [100, 101, 102, 103, 104, P_RELOC + 7]  # pairs 1, 3 and 5 are skipped: rows 101, 103 stay
    got_p, got_m = _relocate(prm, mom, src, dst)
    counts = _check_relocation(prm, mom, got_p, got_m, src, dst)
    assert counts[5] == 2 and counts[9] == 1 and counts[30] == 0 and int(counts.sum()) == 3
    for k in prm:
        assert torch.equal(got_p[k][[101, 103, 30]], prm[k][[101, 103, 30]])


# ---- step ---------------------------------------------------------------------------------------

STEP_GROUPS = ("xyz", "opacity", "scaling", "rotation")
STEP_WIDTH = dict(xyz=3, opacity=1, scaling=3, rotation=4)
LRS = dict(xyz=1.6e-4 * 4.4, opacity=0.05, scaling=5e-3, rotation=1e-3)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15


def _step_state(P, seed=0, zero_moments=False, positive_grads=False):
    gen = torch.Generator().manual_seed(seed)
    prm = {k: torch.randn(P, w, generator=gen) for k, w in STEP_WIDTH.items()}
    # half the rows nearly transparent (the noise gate opens below ~0.05), the rest up to 0.999
    o = torch.rand(P, 1, generator=gen)
    o = torch.where(torch.arange(P)[:, None] % 2 == 0, 0.001 + 0.049 * o, 0.05 + 0.949 * o)
    prm["opacity"] = torch.log(o / (1 - o))
    prm["scaling"] = prm["scaling"] * 0.5 - 2.0
    grd = {k: torch.randn(P, w, generator=gen) for k, w in STEP_WIDTH.items()}
    if positive_grads:  # gradient + regulariser does not cancel: a relative bound holds per element
        grd = {k: v.abs() + 0.1 for k, v in grd.items()}
    if zero_moments:
        mom = {k: (torch.zeros(P, w), torch.zeros(P, w)) for k, w in STEP_WIDTH.items()}
    else:
        mom = {k: (torch.randn(P, w, generator=gen) * 0.1, torch.rand(P, w, generator=gen) * 0.01 + 1e-4)
               for k, w in STEP_WIDTH.items()}
    return prm, grd, mom


def _bias(step):
    return 1.0 - BETA1 ** step, math.sqrt(1.0 - BETA2 ** step)


def _mcmc_step(prm, grd, mom, step, do_adam=True, opacity_reg=0.0, scale_reg=0.0, noise=None, noise_scale=0.0):
    """rt_mcmc_step on device copies; returns (params, moments) as CPU tensors."""
    L = N.train_lib()
    dp = {k: v.clone().cuda() for k, v in prm.items()}
    dg = {k: v.clone().cuda() for k, v in grd.items()}
    dm = {k: (m.clone().cuda(), v.clone().cuda()) for k, (m, v) in mom.items()}
    a = N.RTMcmcStepArgs()
    a.P = dp["xyz"].shape[0]
    bc1, bc2s = _bias(step)
    for k in STEP_GROUPS:
        g = getattr(a, k)
        g.param, g.grad, g.exp_avg, g.exp_avg_sq = (dp[k].data_ptr(), dg[k].data_ptr(), dm[k][0].data_ptr(),
                                                    dm[k][1].data_ptr())
        g.lr, g.bias_correction1, g.bias_correction2_sqrt = LRS[k], bc1, bc2s
    a.beta1, a.beta2, a.eps = BETA1, BETA2, EPS
    a.do_adam, a.opacity_reg, a.scale_reg = int(do_adam), opacity_reg, scale_reg
    dn = noise.clone().cuda() if noise is not None else None
    a.noise = dn.data_ptr() if dn is not None else None
    a.noise_scale, a.gate_k, a.gate_x0 = noise_scale, 100.0, 0.005
    rc = L.rt_mcmc_step(ctypes.byref(a), _stream())
    assert rc == 0, L.rt_last_error()
    torch.cuda.synchronize()
    for k in STEP_GROUPS:
        assert torch.equal(dg[k].cpu(), grd[k]), k  # the gradient arrays are read only
    return {k: v.cpu() for k, v in dp.items()}, {k: (m.cpu(), v.cpu()) for k, (m, v) in dm.items()}


def _adam_step(prm, grd, mom, step):
    """rt_adam_step over the same four groups on device copies."""
    L = N.train_lib()
    dp = {k: v.clone().cuda() for k, v in prm.items()}
    dg = {k: v.clone().cuda() for k, v in grd.items()}
    dm = {k: (m.clone().cuda(), v.clone().cuda()) for k, (m, v) in mom.items()}
    bc1, bc2s = _bias(step)
    arr = (N.RTAdamGroup * 4)(*[N.RTAdamGroup(dp[k].data_ptr(), dg[k].data_ptr(), dm[k][0].data_ptr(),
                                              dm[k][1].data_ptr(), dp[k].numel(), LRS[k], bc1, bc2s)
                                for k in STEP_GROUPS])
    assert L.rt_adam_step(arr, 4, BETA1, BETA2, EPS, _stream()) == 0, L.rt_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dp.items()}, {k: (m.cpu(), v.cpu()) for k, (m, v) in dm.items()}


def _np(d):
    return {k: v.numpy() for k, v in d.items()}


SIZES = [4097, 3]  # four full tiles of 1024 rows and a one-row tail; less than one float4 per group


@pytest.mark.parametrize("P", SIZES)
def test_step_without_terms_is_rt_adam_step_bitwise(gpu, P):
    prm, grd, mom = _step_state(P, seed=3)
    got_p, got_m = _mcmc_step(prm, grd, mom, step=5)
    ref_p, ref_m = _adam_step(prm, grd, mom, step=5)
    for k in STEP_GROUPS:
        assert torch.equal(got_p[k], ref_p[k]), k
        assert torch.equal(got_m[k][0], ref_m[k][0]) and torch.equal(got_m[k][1], ref_m[k][1]), k
        assert not torch.equal(got_p[k], prm[k])


@pytest.mark.parametrize("P", SIZES)
def test_step_regulariser_gradients(gpu, P):
    """From zero moments one step leaves exp_avg = (1 - beta1) * (grad + reg): the total gradient read back
    from the moments against the reference within 1e-5 relative (weights of order P, so that the regulariser
    is of the gradient's order; gradients positive, so that the sum does not cancel)."""
    prm, grd, mom = _step_state(P, seed=4, zero_moments=True, positive_grads=True)
    lam_o, lam_s = 2.0 * P, 1.5 * P
    got_p, got_m = _mcmc_step(prm, grd, mom, step=1, opacity_reg=lam_o, scale_reg=lam_s)
    off_p, off_m = _mcmc_step(prm, grd, mom, step=1)
    go, gs = R.reg_gradients(prm["opacity"].numpy(), prm["scaling"].numpy(), lam_o, lam_s)
    w1 = float(np.float32(1.0 - BETA1))
    for k, reg in (("opacity", go), ("scaling", gs)):
        total = got_m[k][0].double().numpy() / w1
        ref = grd[k].double().numpy() + reg
        assert float(np.median(reg / ref)) > 0.01  # the term is far above the bound in most elements
        assert np.all(np.abs(total - ref) <= 1e-5 * np.abs(ref)), (k, np.max(np.abs(total - ref) / np.abs(ref)))
        assert not torch.equal(got_m[k][0], off_m[k][0])
    for k in ("xyz", "rotation"):  # no regulariser there: bitwise the unregularised step's
        assert torch.equal(got_p[k], off_p[k]) and torch.equal(got_m[k][0], off_m[k][0])
        assert torch.equal(got_m[k][1], off_m[k][1])


NOISE_SCALE = 4.0


def _noise(P, seed=9):
    return torch.randn(P, 3, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("P", SIZES)
def test_step_noise_alone(gpu, P):
    prm, grd, mom = _step_state(P, seed=5)
    prm["opacity"][P - 1, 0] = 40.0  # sigmoid rounds to 1: the gate's exponential overflows
    prm["opacity"][0, 0] = math.log(0.01 / 0.99)  # (at P = 3 the one row left with an open gate: 0.38)
    z = _noise(P)
    got_p, got_m = _mcmc_step(prm, grd, mom, step=5, do_adam=False, noise=z, noise_scale=NOISE_SCALE)
    p64 = _np(prm)
    ref_d = R.noise_delta(p64["opacity"], p64["scaling"], p64["rotation"], z.numpy(), NOISE_SCALE)
    gate = R.noise_gate(p64["opacity"]).reshape(-1)
    open_rows = gate > 0.01
    assert open_rows.any()
    # the displacement is large enough to be seen through the fp32 rounding of xyz + delta
    rel = np.linalg.norm(ref_d, axis=1)[open_rows] / np.linalg.norm(p64["xyz"].astype(np.float64), axis=1)[open_rows]
    assert float(np.median(rel)) >= 1e-3, float(np.median(rel))
    d = got_p["xyz"].double().numpy() - prm["xyz"].double().numpy()
    err = float(np.abs(d - ref_d).sum() / np.abs(ref_d).sum())
    assert err <= 1e-4, err
    opaque = R.sigmoid(p64["opacity"]).reshape(-1) >= 0.5
    assert opaque.any() and torch.equal(got_p["xyz"][opaque], prm["xyz"][opaque])
    for k in ("opacity", "scaling", "rotation"):
        assert torch.equal(got_p[k], prm[k]), k
    for k in STEP_GROUPS:
        assert torch.equal(got_m[k][0], mom[k][0]) and torch.equal(got_m[k][1], mom[k][1]), k
    assert bool(torch.isfinite(got_p["xyz"]).all())


@pytest.mark.parametrize("P", SIZES)
def test_step_all_terms(gpu, P):
    prm, grd, mom = _step_state(P, seed=6)
    z = _noise(P, seed=11)
    lam_o, lam_s = 2.0 * P, 1.5 * P
    got_p, got_m = _mcmc_step(prm, grd, mom, step=5, opacity_reg=lam_o, scale_reg=lam_s, noise=z,
                              noise_scale=NOISE_SCALE)
    steps = dict.fromkeys(STEP_GROUPS, 5)
    ref_p, ref_m = R.step(_np(prm), _np(grd), {k: (m.numpy(), v.numpy()) for k, (m, v) in mom.items()}, LRS, steps,
                          opacity_reg=lam_o, scale_reg=lam_s, noise=z.numpy(), noise_scale=NOISE_SCALE,
                          beta1=BETA1, beta2=BETA2, eps=EPS)
    adam_only, _m = R.step(_np(prm), _np(grd), {k: (m.numpy(), v.numpy()) for k, (m, v) in mom.items()}, LRS, steps,
                           opacity_reg=lam_o, scale_reg=lam_s, beta1=BETA1, beta2=BETA2, eps=EPS)
    for k in STEP_GROUPS:
        x, y = got_p[k].double().numpy(), ref_p[k]
        tol = 1e-6 * max(1.0, float(np.abs(y).max()))  # an Adam element (tests/test_fused_gpu.py)
        if k == "xyz":  # plus the noise's 1e-4 on the displacement
            tol = tol + 1e-4 * np.abs(y - adam_only[k])
        assert np.all(np.abs(x - y) <= tol), (k, float(np.max(np.abs(x - y))))
        # moments: fp32 roundings of operands below 8 (ulp 4.8e-7) weighted by 1 - beta1, resp. of v ~ 0.03
        assert np.allclose(got_m[k][0].double().numpy(), ref_m[k][0], rtol=1e-5, atol=1e-7), k
        assert np.allclose(got_m[k][1].double().numpy(), ref_m[k][1], rtol=1e-5, atol=1e-8), k


# ---- training -----------------------------------------------------------------------------------

def test_mcmc_training_on_hip(gpu):
    """The CPU test's schedule (tests/test_mcmc_train_cpu.py) through the fused forward / loss / backward and
    the native relocation and step kernels, with the same assertions on growth, cap, dead rows, finiteness and
    step counts.  (Run-to-run identity is the CPU test's: the rasterizer's backward sums gradients with float
    atomics, so two HIP runs agree only to rounding.)"""
    W = H = 64
    cams = [c.to("cuda") for c in cameras.fibonacci_cameras(3, W, H)]
    gts = [torch.rand(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(10 + i)) for i in range(3)]
    g = make_model(device="cuda")
    opt = mcmc_opt()
    g.training_setup(opt)
    tr = Trainer(g, cams, gts, opt, PipelineParams(), TrainConfig(c2f=False, seed=5), scene_extent=4.4)
    assert tr.fused and hasattr(g.optimizer, "fused_step")
    log = run_schedule(g, tr)
    check_schedule(g, log)
    with torch.no_grad():
        image, _radii, _depth, _st = fused.forward(g, cams[0], tr.background, 0.3, cache=fused.BinningCache())
    torch.cuda.synchronize()
    assert image.shape == (3, H, W) and bool(torch.isfinite(image).all()) and g.get_xyz.shape[0] == CAP
