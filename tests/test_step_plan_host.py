"""plan_step (csrc/fd_plan.h: which kernel variant every stage of a denoiser step launches, and the fusions that are on) walked on the
host over its whole input space (no GPU): tools/step_plan_check.cpp, a program of its own that calls the very function the library
calls, built with the host sanitizers and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_plan_keeps_what_the_stage_drivers_rely_on(tmp_path):
    from fastdiff_amd import build as fdbuild
    hipcc = fdbuild.HIPCC if os.path.exists(fdbuild.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "step_plan_check")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + fdbuild.CSRC,
           os.path.join(ROOT, "tools", "step_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count(": ok") == 2 and "FAIL" not in r.stdout, r.stdout
