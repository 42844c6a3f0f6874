"""The quality figures against the call they qualify (rmx_xcorr_batch_quality vs rmx_xcorr_batch_weighted) on the same
seeded inputs, in one process, the calls alternating, HIP-event times of the whole call with inputs and outputs resident on
the device, behind a warm-up that covers the clock ramp.  Not part of bench.py.

    python tools/bench_quality.py [--steps 20] [--warmup-s 2.0] [--shapes seam,full]

One JSON line per shape: median ms per call of correlate(whiten=True) and of the same call with the quality output, the
ratio, and the k_quality family's own time per call (HIP events around its launches, option "timing", taken in a separate
pass so that the events do not sit inside the timed calls).  Shapes: tools/bench_weighted.py's seam and full batches."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEAM = [(b, 1, n) for n in (256, 4096, 8192, 16384) for b in (3, 8)]   # (buoys, windows, N)
FULL = [(8, 4096, 4096), (3, 1024, 8192), (8, 256, 16384)]


def run_shape(xcorr, torch, B, W, N, steps, warmup_s):
    P = B * (B - 1) // 2
    rng = np.random.default_rng(1)
    iq = (rng.standard_normal((W, B, N)) + 1j * rng.standard_normal((W, B, N))).astype(np.complex64) * 30
    d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
    del iq
    modes = (False, True)
    outs = {m: (torch.empty((W, P), dtype=torch.int32, device="cuda"), torch.empty((W, P), dtype=torch.float32, device="cuda"),
                torch.empty((W, P), dtype=torch.float32, device="cuda")) for m in modes}
    d_q = torch.empty((W, P, 4), dtype=torch.float32, device="cuda")
    with xcorr.XcorrEngine(B, N, W) as eng:
        stream = torch.cuda.current_stream()
        eng.set_stream(stream.cuda_stream)

        def call(m):
            li, lf, pk = outs[m]
            eng.correlate_device(d_iq.data_ptr(), W, li.data_ptr(), lf.data_ptr(), pk.data_ptr(), whiten=True,
                                 quality_ptr=d_q.data_ptr() if m else 0)

        t_end = time.time() + warmup_s
        while time.time() < t_end:
            for m in modes:
                call(m)
            torch.cuda.synchronize()
        times = {m: [] for m in modes}
        for s in range(steps):
            for m in (modes if s % 2 == 0 else modes[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call(m)
                e1.record(stream)
                e1.synchronize()
                times[m].append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        eng.set_option("timing", 1)
        own = []
        for s in range(steps):
            call(True)
            own.append(eng.last_timing_by_kernel()["k_quality"]["ms"])
    med = {m: float(np.median(times[m])) for m in modes}
    return {"buoys": B, "windows": W, "n_samples": N, "steps": steps, "phat_ms": round(med[False], 4),
            "quality_ms": round(med[True], 4), "quality_ratio": round(med[True] / med[False], 3),
            "k_quality_ms": round(float(np.median(own)), 4),
            "spectrum_gb_read": round(2.0 * 2 * N * 8 * W * P / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup-s", type=float, default=2.0)
    ap.add_argument("--shapes", default="seam,full")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    groups = {"seam": SEAM, "full": FULL}
    for grp in a.shapes.split(","):
        for B, W, N in groups[grp]:
            print(json.dumps(dict(group=grp, **run_shape(xcorr, torch, B, W, N, a.steps, a.warmup_s))), flush=True)


if __name__ == "__main__":
    main()
