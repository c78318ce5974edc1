#!/usr/bin/env python3
"""Cost of the absolute-gradient densification statistics (RR_FLAG_ABSGRAD: AbsGS, gsplat's absgrad) on the
bench scene (1M Gaussians, 1920x1080, SH degree 3), flag off against flag on.

One model, the fused training step's own calls (rain_amd.fused): forward, fused L1+SSIM loss, backward with the
densification statistics, the fused Adam step and the next frame's preprocess inside the per-Gaussian backward.
Three figures per mode:

* blend_bwd       the blend backward (library HIP events, RR_STAGE_BLEND_BWD): k_blend_bwd<0> with the flag
                  off, k_blend_bwd<5> (plain + the absolute sums) with it on;
* gauss_bwd       the per-Gaussian backward with statistics, fused Adam and the next frame's preprocess
                  (RR_STAGE_GAUSS_BWD): k_gauss_bwd with the flag off; with it on, k_abs_stats (the absolute
                  sums' output and the statistics) and k_gauss_bwd launched without statistics;
* step            forward-from-geometry + loss + backward of one step, between two HIP events on the stream.

After a warm-up the two modes alternate step by step over the same view sequence (off, on, on, off, ...), each
step giving one sample of its mode; medians, minima and maxima are reported.  The stage figures are sampled
in a second pass with the library's profiler on (it adds events to the stream, so the step figure is taken
without it).  The flag changes no parameter, so both modes step the one model along the same trajectory.

The new blend variant's occupancy is a build-time choice (rr_blend.hip RR_BWD_ABS_OCC: 4 waves per SIMD with
spills, or 3 without).  --variants NAME=LIB,NAME=LIB runs this measurement once per library (builds of
tools/build_variant.py), each in a child process of its own, the variants alternating over --rounds rounds;
this process then opens no GPU itself.

    python tools/build_variant.py abs_occ4 -DRR_BWD_ABS_OCC=4
    python tools/build_variant.py abs_occ3 -DRR_BWD_ABS_OCC=3
    python tools/absgrad_bench.py --variants occ4=LIB4,occ3=LIB3 [--rounds 2] [--steps 60] [--bench FILE] \\
        [--out profiles/absgrad_bench.json]       (LIB4, LIB3: the paths the two builds printed)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(a):
    import torch

    from rain_amd import _native, fused, synthetic
    from rain_amd.cameras import fibonacci_cameras
    from rain_amd.diff_gaussian_rasterization import _C
    from rain_amd.gaussian_model import GaussianModel, OptimizationParams
    from rain_amd.loss import l1_ssim_forward_backward

    dev = torch.device("cuda:0")
    W, H, P = a.width, a.height, a.points
    cams = [c.to(dev) for c in fibonacci_cameras(200, W, H)]
    g = GaussianModel(3, device=dev)
    g.set_params(synthetic.random_gaussians(P, sh_degree=3, seed=0, bench=True, device=dev))
    g.active_sh_degree = 3
    g.spatial_lr_scale = 4.4
    g.training_setup(OptimizationParams())
    bg = torch.zeros(3, device=dev)
    gts = [torch.rand(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(i)) for i in range(4)]
    cache = fused.BinningCache()
    stats = (g.xyz_gradient_accum, g.denom, g.max_radii2D)

    def step(i, on, nxt):
        """One fused step of view i; returns the next frame's descriptor (preprocessed by this backward)."""
        with torch.no_grad():
            if nxt is None:
                color, _r, _d, st = fused.forward(g, cams[i % len(cams)], bg, 0.3, cache=cache)
            else:
                color, _r, _d, st = fused.forward_next(nxt, g, cache=cache)
            _loss, _parts, dimg = l1_ssim_forward_backward(color, gts[i % len(gts)], 0.2)
            new = fused.prepare_next(g, cams[(i + 1) % len(cams)], bg, 0.3)
            fused.backward(st, dimg, None, stats, adam=g.optimizer.fused_step(g), next_frame=new, absgrad=on)
        return new, st

    def mode_of(k):  # off, on, on, off, ...
        return bool(((k + 1) // 2) % 2)

    i = 0
    for k in range(a.warmup):  # both modes' kernels, the binning cache at its size
        for on in (False, True):
            nxt, _ = step(i, on, None)
            step(i + 1, on, nxt)
            i += 2
    torch.cuda.synchronize()

    # pass 1: the whole step (the trainer's steady state: the frame's geometry comes from the previous
    # step's backward).  Each sample is an untimed step of its mode, which prepares the next view on the
    # current parameters, then the timed step from that geometry.
    ms = {False: [], True: []}
    pairs = {False: [], True: []}
    for k in range(2 * a.steps):
        on = mode_of(k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        warm, _ = step(i, on, None)
        e0.record()
        _nxt, st = step(i + 1, on, warm)
        e1.record()
        e1.synchronize()
        ms[on].append(e0.elapsed_time(e1))
        pairs[on].append(_C.frame_stats(st.geom, st.img, P, W, H)["num_pairs"])
        i += 2

    # pass 2: the two stages, library events
    names = ("blend_bwd", "gauss_bwd")
    stage = {m: {n: [] for n in names} for m in (False, True)}
    for k in range(2 * a.steps):
        on = mode_of(k)
        _native.Profiler.collect()
        with _native.Profiler(list(names)):
            step(i, on, None)
            torch.cuda.synchronize()
        got = _native.Profiler.collect()
        for n in names:
            stage[on][n].append(got[n][0])
        i += 1

    def summary(v):
        return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                    samples=len(v))

    res = {}
    for on, label in ((False, "off"), (True, "on")):
        res[label] = dict(step=summary(ms[on]), blend_bwd=summary(stage[on]["blend_bwd"]),
                          gauss_bwd_stats_adam_next=summary(stage[on]["gauss_bwd"]),
                          num_pairs_median=int(statistics.median(pairs[on])))
    keys = ("step", "blend_bwd", "gauss_bwd_stats_adam_next")
    return {"absgrad": res,
            "on_over_off": {k: round(res["on"][k]["median_ms"] / res["off"][k]["median_ms"], 4) for k in keys},
            "on_minus_off_ms": {k: round(res["on"][k]["median_ms"] - res["off"][k]["median_ms"], 4) for k in keys}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60, help="measured steps per mode and pass")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--variants", default=None, help="NAME=LIB[,NAME=LIB...]: one child process per library and round")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--bench", default=None, help="JSON with the bench.py headline of this tree and of the parent")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"scene": dict(points=a.points, width=a.width, height=a.height, sh_degree=3, low_pass=0.3),
           "method": "alternating modes (off, on, on, off, ...) in one process after warm-up; medians"}
    if a.variants:
        # the occupancy builds of k_blend_bwd<5>: fresh child processes, alternating; the first failure ends the run
        variants = [v.split("=", 1) for v in a.variants.split(",")]
        runs = {name: [] for name, _ in variants}
        for _r in range(a.rounds):
            for name, lib in variants:
                env = dict(os.environ, RAIN_RASTER_LIB=os.path.abspath(lib))
                cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup),
                       "--points", str(a.points), "--width", str(a.width), "--height", str(a.height)]
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.timeout)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-4000:])
                    raise SystemExit(f"variant {name} failed with exit status {r.returncode}")
                runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
        out["method"] += "; one child process per variant and round, the variants alternating"
        out["variants"] = {name: dict(library=lib, rounds=[r for r in runs[name]]) for name, lib in variants}
    else:
        out.update(measure(a))
        out["library"] = os.path.basename(os.environ.get("RAIN_RASTER_LIB") or "librain_raster.so")
    if a.bench:
        with open(a.bench) as f:
            out["bench_py_flag_off"] = json.load(f)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
