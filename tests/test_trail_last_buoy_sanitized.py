"""The fused N = 4096 kernel does not store the last buoy's spectrum, so no entry of its pair table may request it
(host::encode_pair_trail, host::trail_kernel_ok in radio-mapper_amd/csrc/host_plan.hpp): tests/host/test_trail_last_buoy.cpp
under AddressSanitizer + UndefinedBehaviorSanitizer, for B = 2 ... 32 and 40 (a CPU build; nothing here touches the GPU)."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_trail_never_requests_last_buoy_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_trail_last_buoy")
    src = os.path.join(ROOT, "tests", "host", "test_trail_last_buoy.cpp")
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
