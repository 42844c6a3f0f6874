"""host::check_caf_request and host::plan_caf as rmx_caf_batch_bands calls them (radio-mapper_amd/csrc/host_request.hpp,
host_plan.hpp), under AddressSanitizer + UndefinedBehaviorSanitizer: tests/host/test_caf_bands_request.cpp is a stand-alone
program over arrays of exactly the stated sizes, built here with g++ -fsanitize=address,undefined and run directly."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_caf_bands_request_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_caf_bands_request")
    src = os.path.join(ROOT, "tests", "host", "test_caf_bands_request.cpp")
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
