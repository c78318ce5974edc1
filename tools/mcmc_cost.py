#!/usr/bin/env python3
"""Cost of the MCMC optimizer block (rain_amd/csrc/mcmc.hip rt_mcmc_step) at P Gaussians, HIP events, warm:

1. rt_mcmc_step with every term on (both regularisers, Adam, noise): 80 floats per row — param, grad,
   exp_avg, exp_avg_sq read and param, exp_avg, exp_avg_sq written for xyz / opacity / scaling / rotation
   (11 floats per row: 77) plus the 3 normals;
2. rt_adam_step over the same four groups (77 floats per row);
3. rt_stream_rmw (the bare read-modify-write stream) over the same bytes as 1.

The three are timed in alternation, `--rounds` windows of `--reps` calls each; the parameters are restored
before every window so that the values stay those of a training step.  Two modes: "back_to_back" (one event
pair around the window: the 320 MB of a 1M-row step partly stay in the 256 MB Infinity Cache from call to
call) and "swept" (a `--sweep-mb` buffer is filled before every call and each call has its own event pair:
the caches hold nothing of the arrays, as in a training step, where a whole frame runs between two calls).
`--variant NAME=PATH` adds rt_mcmc_step of another build of librain_train.so (tools/build_variant.py --lib
librain_train.so) to the alternation.

    python tools/mcmc_cost.py [--out profiles/mcmc_step_bench.json]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH = dict(xyz=3, opacity=1, scaling=3, rotation=4)
LRS = dict(xyz=1.6e-4 * 4.4, opacity=0.05, scaling=5e-3, rotation=1e-3)
STEP_FLOATS = 7 * sum(WIDTH.values()) + 3  # 80
ADAM_FLOATS = 7 * sum(WIDTH.values())      # 77


def main():
    import torch

    from rain_amd import _native as N

    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=6, help="timed windows per kernel")
    ap.add_argument("--sweep-mb", type=int, default=512, help="buffer filled before every call of the swept mode")
    ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of another librain_train.so")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("mcmc_cost.py: no HIP device", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    P = a.points
    L = N.train_lib()
    gen = torch.Generator(device=dev).manual_seed(0)
    prm = {k: torch.randn(P, w, device=dev, generator=gen) for k, w in WIDTH.items()}
    o = torch.rand(P, 1, device=dev, generator=gen) * 0.98 + 0.001
    prm["opacity"] = torch.log(o / (1 - o))
    prm["scaling"] = prm["scaling"] * 0.5 - 2.0
    grd = {k: torch.randn(P, w, device=dev, generator=gen) * 1e-3 for k, w in WIDTH.items()}
    mom = {k: (torch.randn(P, w, device=dev, generator=gen) * 1e-4, torch.rand(P, w, device=dev, generator=gen) * 1e-6)
           for k, w in WIDTH.items()}
    saved = {k: v.clone() for k, v in prm.items()}
    noise = torch.randn(P, 3, device=dev, generator=gen)
    stream = N.stream_of(noise)
    step = 100
    bc1, bc2s = 1.0 - 0.9 ** step, math.sqrt(1.0 - 0.999 ** step)

    args = N.RTMcmcStepArgs()
    args.P = P
    for k in WIDTH:
        g = getattr(args, k)
        g.param, g.grad, g.exp_avg, g.exp_avg_sq = (prm[k].data_ptr(), grd[k].data_ptr(), mom[k][0].data_ptr(),
                                                    mom[k][1].data_ptr())
        g.lr, g.bias_correction1, g.bias_correction2_sqrt = LRS[k], bc1, bc2s
    args.beta1, args.beta2, args.eps = 0.9, 0.999, 1e-15
    args.do_adam, args.opacity_reg, args.scale_reg = 1, 0.01, 0.01
    args.noise, args.noise_scale, args.gate_k, args.gate_x0 = noise.data_ptr(), 5e5 * LRS["xyz"], 100.0, 0.005
    groups = (N.RTAdamGroup * 4)(*[N.RTAdamGroup(prm[k].data_ptr(), grd[k].data_ptr(), mom[k][0].data_ptr(),
                                                 mom[k][1].data_ptr(), prm[k].numel(), LRS[k], bc1, bc2s)
                                   for k in WIDTH])
    # the bare stream: three arrays read and written back, 6 floats moved per element -> the step's bytes
    n_rmw = (STEP_FLOATS * P // 6 + 3) // 4 * 4
    rmw = [torch.zeros(n_rmw, device=dev) for _ in range(3)]

    def step_call(lib):
        def f():
            rc = lib.rt_mcmc_step(ctypes.byref(args), stream)
            if rc != 0:
                raise RuntimeError(lib.rt_last_error().decode(errors="replace"))
        return f

    def adam_call():
        N.check_rt(L.rt_adam_step(groups, 4, 0.9, 0.999, 1e-15, stream), "rt_adam_step")

    def rmw_call():
        N.check_rt(L.rt_stream_rmw(rmw[0].data_ptr(), rmw[1].data_ptr(), rmw[2].data_ptr(), n_rmw, stream),
                   "rt_stream_rmw")

    calls = {"rt_mcmc_step": step_call(L), "rt_adam_step": adam_call, "rt_stream_rmw": rmw_call}
    for spec in a.variant:
        name, _, path = spec.partition("=")
        V = ctypes.CDLL(os.path.abspath(path))
        V.rt_mcmc_step.restype = ctypes.c_int
        V.rt_mcmc_step.argtypes = [ctypes.POINTER(N.RTMcmcStepArgs), ctypes.c_void_p]
        V.rt_last_error.restype = ctypes.c_char_p
        calls["rt_mcmc_step@" + name] = step_call(V)

    def restore():
        for k in prm:
            prm[k].copy_(saved[k])

    for fn in calls.values():  # warm-up
        for _ in range(5):
            fn()
    us = {k: [] for k in calls}
    swept = {k: [] for k in calls}
    sweep = torch.empty(a.sweep_mb << 20, dtype=torch.uint8, device=dev)
    for _round in range(a.rounds):
        for name, fn in calls.items():
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(round(1000.0 * e0.elapsed_time(e1) / a.reps, 2))
        for name, fn in calls.items():
            restore()
            evs = []
            for i in range(a.reps):
                sweep.fill_(i & 0xff)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                evs.append((e0, e1))
            torch.cuda.synchronize()
            swept[name].append(round(1000.0 * sum(x.elapsed_time(y) for x, y in evs) / a.reps, 2))
    med = {k: statistics.median(v) for k, v in us.items()}
    med_swept = {k: statistics.median(v) for k, v in swept.items()}
    floats = {"rt_mcmc_step": STEP_FLOATS * P, "rt_adam_step": ADAM_FLOATS * P, "rt_stream_rmw": 6 * n_rmw}
    out = {
        "points": P, "reps": a.reps, "rounds": a.rounds, "us_per_call": us, "median_us": med,
        "swept": {"sweep_mb": a.sweep_mb, "us_per_call": swept, "median_us": med_swept,
                  "GBps": {k: round(4.0 * floats[k.split("@")[0]] / (med_swept[k] * 1e-6) / 1e9, 1)
                           for k in med_swept},
                  "ratio_mcmc_step_to_adam_step": round(med_swept["rt_mcmc_step"] / med_swept["rt_adam_step"], 3),
                  "ratio_mcmc_step_to_stream_rmw": round(med_swept["rt_mcmc_step"] / med_swept["rt_stream_rmw"], 3)},
        "floats_per_row": {"rt_mcmc_step": STEP_FLOATS, "rt_adam_step": ADAM_FLOATS},
        "GBps": {k: round(4.0 * floats[k.split("@")[0]] / (med[k] * 1e-6) / 1e9, 1) for k in med},
        "ratio_mcmc_step_to_adam_step": round(med["rt_mcmc_step"] / med["rt_adam_step"], 3),
        "ratio_mcmc_step_to_stream_rmw": round(med["rt_mcmc_step"] / med["rt_stream_rmw"], 3),
    }
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
