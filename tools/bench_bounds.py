"""Bounded against unbounded cross-correlation (rmx_xcorr_batch_bounded vs rmx_xcorr_batch) on the same seeded inputs,
in one process, alternating the two calls, HIP-event times of the whole call with inputs and outputs resident on the
device, behind a warm-up that covers the clock ramp.  Not part of bench.py.

    python tools/bench_bounds.py [--steps 20] [--warmup-s 2.0] [--shapes cfg3,n8192,n16384,four]

One JSON line per shape: median ms of each, their ratio (bounded / unbounded), and the intervals used (+-1668 lags at
N = 4096, the BASELINE bound of 50 km at 10 MS/s; the same physical bound elsewhere, clipped to the window)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {   # name: (buoys, windows, N)
    "cfg3": (8, 4096, 4096),
    "n8192": (8, 512, 8192),
    "n16384": (8, 256, 16384),
    "four": (3, 64, 1 << 20),
}
BOUND = 1668   # lags: 50 km / c at 10 MS/s


def run_shape(xcorr, torch, name, steps, warmup_s):
    B, W, N = SHAPES[name]
    P = B * (B - 1) // 2
    rng = np.random.default_rng(1)
    iq = (rng.standard_normal((W, B, N)) + 1j * rng.standard_normal((W, B, N))).astype(np.complex64) * 30
    b = min(BOUND, N - 1)
    lb = np.tile(np.array([[-b, b]], np.int32), (P, 1))
    d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
    del iq
    outs = [(torch.empty((W, P), dtype=torch.int32, device="cuda"), torch.empty((W, P), dtype=torch.float32, device="cuda"),
             torch.empty((W, P), dtype=torch.float32, device="cuda")) for _ in range(2)]
    with xcorr.XcorrEngine(B, N, W) as eng:
        stream = torch.cuda.current_stream()
        eng.set_stream(stream.cuda_stream)

        def call(bounded):
            li, lf, pk = outs[1 if bounded else 0]
            eng.correlate_device(d_iq.data_ptr(), W, li.data_ptr(), lf.data_ptr(), pk.data_ptr(),
                                 lag_bounds=lb if bounded else None)

        t_end = time.time() + warmup_s                     # clock ramp: keep the chip busy before timing
        while time.time() < t_end:
            call(False)
            call(True)
            torch.cuda.synchronize()
        times = {False: [], True: []}
        for s in range(steps):
            for bounded in ((False, True) if s % 2 == 0 else (True, False)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call(bounded)
                e1.record(stream)
                e1.synchronize()
                times[bounded].append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        same = bool(torch.equal(outs[0][0], outs[1][0]))   # with no physical decoy in random data: usually the same lags
    u, bb = float(np.median(times[False])), float(np.median(times[True]))
    return {"shape": name, "buoys": B, "windows": W, "n_samples": N, "bound_lags": [-b, b], "steps": steps,
            "unbounded_ms": round(u, 4), "bounded_ms": round(bb, 4), "ratio": round(bb / u, 4),
            "unbounded_min_ms": round(float(np.min(times[False])), 4), "bounded_min_ms": round(float(np.min(times[True])), 4),
            "same_lag_int": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup-s", type=float, default=2.0)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    for name in a.shapes.split(","):
        print(json.dumps(run_shape(xcorr, torch, name, a.steps, a.warmup_s)), flush=True)


if __name__ == "__main__":
    main()
