"""Every device and pinned buffer of a ctx is one growable type that owns its block, its capacity, its share of
rmx_scratch_bytes and, where its content is cached, the key of what it holds (radio-mapper_amd/csrc/dev_buf.hpp, a HIP-free
header that rmx_hip.hip instantiates with the HIP calls).  tests/host/test_dev_buf.cpp instantiates it with a counting
malloc that fails on demand, built here with g++ under AddressSanitizer (leak detection on) + UndefinedBehaviorSanitizer:
live blocks and ledger after any interleaving of reserve / assign / move / destruction, what a reserve costs in
allocations and waits, the state after the n-th allocation fails for every n of a scripted sequence -- the pair plan
whose second allocation fails and the pair list whose refill fails among them --, and the halve-and-retry loop of
generic_ensure.  A CPU build; nothing here touches the GPU."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_dev_buf_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_dev_buf")
    src = os.path.join(ROOT, "tests", "host", "test_dev_buf.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-pthread", "-Wall", "-Wextra", "-Werror", "-o", exe, src]
    subprocess.run(cmd, check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "all checks passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "ERROR: LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr
