#!/usr/bin/env python3
"""Cost of anti-aliased rendering (RR_FLAG_ANTIALIAS: the opacity compensation of the 2D dilation) on the
bench scene (1M Gaussians, 1920x1080, SH degree 3), flag off against flag on.

One process, one model, the fused training step's own calls (rain_amd.fused): forward, fused L1+SSIM loss,
backward with the fused Adam step and the next frame's preprocess inside the per-Gaussian backward.  Three
figures per mode:

* preprocess      the forward preprocess kernel of a frame that runs its own (library HIP events,
                  RR_STAGE_PREPROCESS);
* gauss_bwd       the per-Gaussian backward with fused Adam and the next frame's preprocess
                  (RR_STAGE_GAUSS_BWD): k_gauss_bwd<3> with the flag off, k_gauss_bwd_aa<3, 0> with it on;
* step            forward-from-geometry + loss + backward of one step, between two HIP events on the stream.

After a warm-up the two modes alternate step by step over the same view sequence (off, on, on, off, ...), each
step giving one sample of its mode; medians, minima and maxima are reported.  The stage figures are sampled
in a second pass with the library's profiler on (it adds events to the stream, so the step figure is taken
without it).  The flag changes the rendered image, hence the gradients and the parameters: both modes step
the one model, which only matters to the figures through the pair count, reported per mode.

    python tools/antialias_bench.py [--steps 60] [--out profiles/antialias_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from rain_amd import _native, fused, synthetic
    from rain_amd.cameras import fibonacci_cameras
    from rain_amd.diff_gaussian_rasterization import _C
    from rain_amd.gaussian_model import GaussianModel, OptimizationParams
    from rain_amd.loss import l1_ssim_forward_backward

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60, help="measured steps per mode and pass")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bench", default=None, help="JSON with the bench.py headline of this tree and of the parent")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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

    def step(i, aa, nxt):
        """One fused step of view i; returns the next frame's descriptor (preprocessed by this backward)."""
        with torch.no_grad():
            if nxt is None:
                color, _r, _d, st = fused.forward(g, cams[i % len(cams)], bg, 0.3, cache=cache, antialiasing=aa)
            else:
                color, _r, _d, st = fused.forward_next(nxt, g, cache=cache)
            _loss, _parts, dimg = l1_ssim_forward_backward(color, gts[i % len(gts)], 0.2)
            new = fused.prepare_next(g, cams[(i + 1) % len(cams)], bg, 0.3, antialiasing=aa)
            fused.backward(st, dimg, None, None, adam=g.optimizer.fused_step(g), next_frame=new)
        return new, st

    def mode_of(k):  # off, on, on, off, ...
        return bool(((k + 1) // 2) % 2)

    i = 0
    for k in range(a.warmup):  # both modes' kernels, the binning cache at its size
        for aa in (False, True):
            nxt, _ = step(i, aa, None)
            step(i + 1, aa, nxt)
            i += 2
    torch.cuda.synchronize()

    # pass 1: the whole step (the trainer's steady state: the frame's geometry comes from the previous
    # step's backward).  Each sample is an untimed step of its mode, which prepares the next view on the
    # current parameters, then the timed step from that geometry.
    ms = {False: [], True: []}
    pairs = {False: [], True: []}
    for k in range(2 * a.steps):
        aa = mode_of(k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        warm, _ = step(i, aa, None)
        e0.record()
        _nxt, st = step(i + 1, aa, warm)
        e1.record()
        e1.synchronize()
        ms[aa].append(e0.elapsed_time(e1))
        pairs[aa].append(_C.frame_stats(st.geom, st.img, P, W, H)["num_pairs"])
        i += 2

    # pass 2: the two stages, library events
    stage = {False: {"preprocess": [], "gauss_bwd": []}, True: {"preprocess": [], "gauss_bwd": []}}
    for k in range(2 * a.steps):
        aa = mode_of(k)
        _native.Profiler.collect()
        with _native.Profiler(["preprocess", "gauss_bwd"]):
            step(i, aa, None)  # a forward with its own preprocess, and a backward with Adam + next frame
            torch.cuda.synchronize()
        got = _native.Profiler.collect()
        for name in ("preprocess", "gauss_bwd"):
            stage[aa][name].append(got[name][0])
        i += 1

    def summary(v):
        return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                    samples=len(v))

    res = {}
    for aa, label in ((False, "off"), (True, "on")):
        res[label] = dict(step=summary(ms[aa]), preprocess=summary(stage[aa]["preprocess"]),
                          gauss_bwd_adam_next=summary(stage[aa]["gauss_bwd"]),
                          num_pairs_median=int(statistics.median(pairs[aa])))
    ratio = {k: round(res["on"][k]["median_ms"] / res["off"][k]["median_ms"], 4)
             for k in ("step", "preprocess", "gauss_bwd_adam_next")}
    out = {"scene": dict(points=P, width=W, height=H, sh_degree=3, low_pass=0.3),
           "method": "alternating modes (off, on, on, off, ...) in one process after warm-up; medians",
           "antialiasing": res, "on_over_off": ratio}
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
