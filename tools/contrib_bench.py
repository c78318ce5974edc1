#!/usr/bin/env python3
"""Cost of the per-Gaussian blend-contribution statistics (rr_contributions) on the bench scene (1M
Gaussians, 1920x1080, SH degree 3), beside the forward blend of the same frames: the existing kernel
that does the same walk, and the yardstick.

One process.  Per view: a forward whose blend stage (RR_STAGE_BLEND_FWD, both phases) the library times
with its own HIP events (rr_profile_*), then rr_contributions on that frame between two HIP events,
without and with a pixel-weight map, accumulating into one buffer (the N-view use: the walk alone) and,
as a third figure, with accumulate = 0 (plus the clear of the records).  After a warm-up over every view,
each view gives one sample per mode, the order of the modes alternating from view to view; medians are
reported, with the ratio to the forward blend and the kernel's resource line from the compiler
(tools/kernel_resources.py's figures, for rr_contrib.hip alone).

    python tools/contrib_bench.py [--views 24] [--out profiles/contrib_bench.json]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resource_line():
    """VGPRs / AGPRs / SGPRs / scratch / LDS / waves per SIMD / spills of k_contrib, as compiled."""
    from rain_amd import _build as B
    from tools.kernel_resources import LABELS

    src = "rr_contrib.hip"
    cmd = [B.HIPCC, "-O3", "-fPIC", "-std=c++17", f"--offload-arch={B.ARCH}", "-I", os.path.join(ROOT, "include"),
           "-I", B.CSRC, *B.EXTRA.get(src, []), "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(B.CSRC, src), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return None
    fig, on = {}, False
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s*(.*?)(?: \[-Rpass-analysis=kernel-resource-usage\])?$", line)
        t = m.group(1).strip() if m else ""
        if t.startswith("Function Name:"):
            on = "k_contribENS" in t
        for label in LABELS:
            if on and t.startswith(label + ":"):
                fig[label] = t.split(":")[1].strip()
    return "k_contrib: " + ", ".join(f"{k} {fig.get(k, '?')}" for k in LABELS) if fig else None


def main():
    import torch

    from rain_amd import _native, fused, synthetic
    from rain_amd.cameras import fibonacci_cameras
    from rain_amd.diff_gaussian_rasterization import _C
    from rain_amd.gaussian_model import GaussianModel

    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--resources", default=None, help="the kernel's resource line (default: compile and read it)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H, P = a.width, a.height, a.points
    cams = [c.to(dev) for c in fibonacci_cameras(200, W, H)][:a.views]
    g = GaussianModel(3, device=dev)
    g.set_params(synthetic.random_gaussians(P, sh_degree=3, seed=0, bench=True, device=dev))
    g.active_sh_degree = 3
    bg = torch.zeros(3, device=dev)
    gmap = torch.randn(H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    buf = torch.zeros((P, 4), dtype=torch.float32, device=dev)
    modes = {"no_map": dict(pixel_weight=None, out=buf), "map": dict(pixel_weight=gmap, out=buf),
             "no_map_with_clear": dict(pixel_weight=None, out=None)}

    def forward(c, profile):
        if profile:
            _native.Profiler.collect()
            with _native.Profiler(["blend_fwd"]), torch.no_grad():
                st = fused.forward(g, c, bg, 0.3)[3]
            torch.cuda.synchronize()
            ms, _n = _native.Profiler.collect()["blend_fwd"]
            return st, ms  # the stage's total of the frame: phase A + phase B
        with torch.no_grad():
            st = fused.forward(g, c, bg, 0.3)[3]
        return st, None

    def contrib(st, kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _C.gaussian_contributions(st.radii, st.geom, st.binning, st.img, st.num_rendered, P, W, H, **kw)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for c in cams:  # warm-up of every mode on every view
        st, _ = forward(c, False)
        for kw in modes.values():
            contrib(st, kw)
    ms = {m: [] for m in modes}
    blend, pairs = [], []
    for i, c in enumerate(cams):
        st, b = forward(c, True)
        blend.append(b)
        pairs.append(_C.frame_stats(st.geom, st.img, P, W, H)["l_eff"])
        order = list(modes) if i % 2 == 0 else list(modes)[::-1]
        for m in order:
            ms[m].append(contrib(st, modes[m]))
    med = {m: statistics.median(v) for m, v in ms.items()}
    bmed = statistics.median(blend)
    visible = int((buf.view(torch.int32)[:, 3] != 0).sum())
    out = {"scene": dict(points=P, width=W, height=H, sh_degree=3, views=len(cams)),
           "samples_per_mode": len(cams),
           "walked_pairs_median": int(statistics.median(pairs)),
           "gaussians_hit_in_any_view": visible,
           "blend_fwd_median_ms": round(bmed, 4),
           "contributions_median_ms": {m: round(v, 4) for m, v in med.items()},
           "contributions_min_ms": {m: round(min(v), 4) for m, v in ms.items()},
           "contributions_max_ms": {m: round(max(v), 4) for m, v in ms.items()},
           "ratio_to_blend_fwd": {m: round(v / bmed, 3) for m, v in med.items()},
           "kernel_resources": a.resources or resource_line()}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
