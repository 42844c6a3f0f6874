"""The fine lag search against the call it refines (rmx_xcorr_batch_refined vs rmx_xcorr_batch_weighted) on the same
seeded inputs, in one process, the calls alternating, HIP-event times of the whole call with inputs and outputs resident on
the device, behind a warm-up that covers the clock ramp.  Not part of bench.py.

    python tools/bench_refined.py [--steps 20] [--warmup-s 2.0] [--shapes seam,full,integrated]

One JSON line per shape: median ms per call of correlate(whiten=True) and of correlate(whiten=True, refine=U) for
U = 4, 8, 16, the ratios, and the k_refine family's own time per call (HIP events around its launches, option "timing",
taken in a separate pass so that the events do not sit inside the timed calls).  Shapes: tools/bench_weighted.py's seam and
full batches, plus the integrated seam shape (3 buoys, 8 windows of 1024 samples, integrate = 8: one group per call)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEAM = [(b, 1, n, 1) for n in (256, 4096, 8192, 16384) for b in (3, 8)]   # (buoys, windows, N, integrate)
FULL = [(8, 4096, 4096, 1), (3, 1024, 8192, 1), (8, 256, 16384, 1)]
INTEGRATED = [(3, 8, 1024, 8)]
REFINE = (4, 8, 16)


def run_shape(xcorr, torch, B, W, N, K, steps, warmup_s):
    P = B * (B - 1) // 2
    G = W // K
    rng = np.random.default_rng(1)
    iq = (rng.standard_normal((W, B, N)) + 1j * rng.standard_normal((W, B, N))).astype(np.complex64) * 30
    d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
    del iq
    modes = [0] + list(REFINE)
    outs = {m: (torch.empty((G, P), dtype=torch.int32, device="cuda"), torch.empty((G, P), dtype=torch.float32, device="cuda"),
                torch.empty((G, P), dtype=torch.float32, device="cuda")) for m in modes}
    with xcorr.XcorrEngine(B, N, W) as eng:
        stream = torch.cuda.current_stream()
        eng.set_stream(stream.cuda_stream)

        def call(m):
            li, lf, pk = outs[m]
            eng.correlate_device(d_iq.data_ptr(), W, li.data_ptr(), lf.data_ptr(), pk.data_ptr(), whiten=True, integrate=K, refine=m)

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
        own = {m: [] for m in REFINE}
        for s in range(steps):
            for m in REFINE:
                call(m)
                own[m].append(eng.last_timing_by_kernel()["k_refine"]["ms"])
    med = {m: float(np.median(times[m])) for m in modes}
    out = {"buoys": B, "windows": W, "n_samples": N, "integrate": K, "steps": steps, "phat_ms": round(med[0], 4)}
    for m in REFINE:
        out["refine%d_ms" % m] = round(med[m], 4)
        out["refine%d_ratio" % m] = round(med[m] / med[0], 3)
        out["k_refine%d_ms" % m] = round(float(np.median(own[m])), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup-s", type=float, default=2.0)
    ap.add_argument("--shapes", default="seam,full,integrated")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    groups = {"seam": SEAM, "full": FULL, "integrated": INTEGRATED}
    for grp in a.shapes.split(","):
        for B, W, N, K in groups[grp]:
            print(json.dumps(dict(group=grp, **run_shape(xcorr, torch, B, W, N, K, a.steps, a.warmup_s))), flush=True)


if __name__ == "__main__":
    main()
