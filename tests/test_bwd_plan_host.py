"""The backward's variant choice (rain_amd/csrc/rr_bwd_plan.hpp) checked on the CPU: tests/host/
bwd_plan_check.hip is built with the product's compiler, include paths and target plus the host
sanitizers, and run as a stand-alone program (no GPU, nothing preloaded)."""
import os
import subprocess

from rain_amd import _build as B

HERE = os.path.dirname(os.path.abspath(__file__))


def test_backward_plan_host_checker(tmp_path):
    exe = str(tmp_path / "bwd_plan_check")
    cmd = [B.HIPCC, *B.CXXFLAGS, "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined",
           os.path.join(HERE, "host", "bwd_plan_check.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout
