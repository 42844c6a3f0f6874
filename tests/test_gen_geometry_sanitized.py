"""The generic path's geometry and LDS layouts under AddressSanitizer + UndefinedBehaviorSanitizer:
radio-mapper_amd/csrc/gen_geometry.hpp is a HIP-free header that the kernels (region pointers) and rmx_hip.hip (launch
bytes) both read; tests/host/test_gen_geometry.cpp holds it to the formulas the launch code carried before, over the
whole domain the selection code can reach, built here with g++ -fsanitize=address,undefined (a stand-alone CPU program,
as tests/test_host_plan_sanitized.py)."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_gen_geometry_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_gen_geometry")
    src = os.path.join(ROOT, "tests", "host", "test_gen_geometry.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-pthread", "-Wall", "-Wextra", "-Werror", "-o", exe, src]
    subprocess.run(cmd, check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "all checks passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
