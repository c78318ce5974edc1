#!/usr/bin/env python3
"""Per-kernel resource usage of every HIP source of the package, as the compiler reports it
(-Rpass-analysis=kernel-resource-usage) with the project's build flags.  Needs no GPU.

    python tools/kernel_resources.py [--against OTHER_ROOT] [--out FILE]

One row per kernel of the project: VGPRs / AGPRs / SGPRs / scratch B per lane / LDS B per block /
waves per SIMD / spilled VGPRs / spilled SGPRs.  The kernels a source instantiates from rocPRIM are
summed up per source as their count and a digest of their (symbol, figures) rows.  --against
compiles another checkout's rain_amd/csrc and include with the same flags and prints its figures
beside this tree's ("=" where they are equal, "-" where a kernel exists in one tree only).
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LABELS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]", "VGPRs Spill", "SGPRs Spill"]


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return r.stdout.splitlines() if r.returncode == 0 else names


def figures(root):
    """{(source, kernel): "v/a/s/scratch/lds/occ/spillv/spills"} of the checkout at `root`."""
    from rain_amd import _build as B

    csrc, include = os.path.join(root, "rain_amd", "csrc"), os.path.join(root, "include")

    def one(src):
        flags = ["-O3", "-fPIC", "-std=c++17", f"--offload-arch={B.ARCH}", "-I", include, "-I", csrc]
        cmd = [B.HIPCC, *flags, *B.EXTRA.get(src, []), "--offload-device-only", "-Rpass-analysis=kernel-resource-usage",
               "-c", os.path.join(csrc, src), "-o", os.devnull]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
        rows, cur = [], None
        for line in r.stderr.splitlines():
            m = re.search(r"remark:\s*(.*?)(?: \[-Rpass-analysis=kernel-resource-usage\])?$", line)
            t = m.group(1).strip() if m else ""
            f = re.match(r"Function Name: (\S+)", t)
            if f:
                cur = {"name": f.group(1)}
                rows.append(cur)
            for label in LABELS:
                if cur is not None and t.startswith(label + ":"):
                    cur[label] = t.split(":")[1].strip()
        return src, rows

    srcs = sorted(s for lib in B.LIBS.values() for s in lib if os.path.exists(os.path.join(csrc, s)))
    out = {}
    with ThreadPoolExecutor(max_workers=8) as ex:
        for src, rows in ex.map(one, srcs):
            lib = []
            for r, n in zip(rows, demangle([r["name"] for r in rows])):
                fig = "/".join(r.get(k, "?") for k in LABELS)
                n = n.replace("(anonymous namespace)::", "")
                if "rocprim::" in n.split("(")[0].split("<")[0]:
                    lib.append(f"{r['name']} {fig}")
                    continue
                n = re.sub(r"^void ", "", re.sub(r"\(.*$", "", n))  # the kernel and its template arguments
                if len(n) > 64:  # long template argument lists: cut, kept unique by a digest of the symbol
                    n = n[:56] + "~" + hashlib.sha1(r["name"].encode()).hexdigest()[:6]
                out[(src, n)] = fig
            if lib:
                out[(src, f"({len(lib)} rocPRIM kernels)")] = "sha1:" + hashlib.sha1("\n".join(sorted(lib)).encode()).hexdigest()[:12]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", default=None, help="root of another checkout to print beside this tree")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mine = figures(ROOT)
    other = figures(os.path.abspath(a.against)) if a.against else None
    lines = []
    for key in sorted(set(mine) | set(other or {})):
        row = f"{key[0]:<19} {key[1]:<64} {mine.get(key, '-'):<28}"
        if other is not None:
            o = other.get(key, "-")
            row += " " + ("=" if o == mine.get(key) else o)
        lines.append(row.rstrip())
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
