"""CPU only: the Python time of one device-pointer call of the binding (radio-mapper_amd/xcorr.py), over a fake library whose
entries return RMX_OK at once -- what a call costs before and after the C entry, which is what shows in bench.py's
single-window latency (a kernel of the order of 13 us).  Three cases, each the minimum of 7 repetitions of 20 000 calls:

  correlate_device        default arguments, 8 buoys
  caf_device              a 21-point grid, otherwise default arguments
  correlate_bands_device  two shared bands

usage: python tools/bench_binding_overhead.py [--reps 7] [--calls 20000]
       prints one JSON line, microseconds per call.  To compare two trees, alternate runs of this script between them in
       one session and hold the difference against the run-to-run spread of either (profiles/r16_binding_overhead.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rmx_xcorr_batch" + s for s in ("", "_bounded", "_weighted", "_bands", "_integrated", "_refined", "_quality",
                                           "_bands_quality", "_bands_integrated")] + \
          ["rmx_caf_batch" + s for s in ("", "_request", "_quality", "_integrated")]


def _ok(*args):
    return 0


class FakeLib:
    pass


for _name in ENTRIES:
    setattr(FakeLib, _name, staticmethod(_ok))


def engine(n_buoys):
    sys.path.insert(0, ROOT)
    from radio_mapper_amd import xcorr

    class Engine(xcorr.XcorrEngine):
        def __init__(self):
            self.n_buoys, self.n_samples, self.max_windows, self.device = n_buoys, 4096, 64, 0
            self._lib, self._ctx = FakeLib(), None

        def __del__(self):
            pass
    return Engine()


def per_call_us(fn, reps, calls):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        best = min(best, time.perf_counter() - t0)
    return best / calls * 1e6


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20000)
    a = ap.parse_args()
    eng = engine(8)
    grid = np.linspace(-1e-4, 1e-4, 21)
    bands = np.array([[-0.25, 0.0], [0.0, 0.25]])
    cases = {
        "correlate_device": lambda: eng.correlate_device(4096, 1, 8192, 12288, 16384),
        "caf_device": lambda: eng.caf_device(4096, 1, grid, 20480, 8192, 12288, 16384),
        "correlate_bands_device": lambda: eng.correlate_bands_device(4096, 1, bands, 8192, 12288, 16384),
    }
    for fn in cases.values():   # warm up
        for _ in range(1000):
            fn()
    print(json.dumps({k: round(per_call_us(fn, a.reps, a.calls), 3) for k, fn in cases.items()}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
