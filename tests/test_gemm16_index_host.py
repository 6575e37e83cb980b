"""The index arithmetic of k_kp_gemm_w<16> walked on the host (no GPU): tools/gemm16_index_check.cpp, a program of its own that calls
the lane maps the kernel calls (fd_kernels.h: gw16_*), built with the host sanitizers and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_lane_and_register_of_the_16_row_item_on_the_host(tmp_path):
    from fastdiff_amd import build as fdbuild
    hipcc = fdbuild.HIPCC if os.path.exists(fdbuild.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "gemm16_index_check")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + fdbuild.CSRC,
           os.path.join(ROOT, "tools", "gemm16_index_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count(": ok") == 8 and "FAIL" not in r.stdout, r.stdout
