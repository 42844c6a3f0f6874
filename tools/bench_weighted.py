"""Weighted against plain cross-correlation (rmx_xcorr_batch_weighted vs rmx_xcorr_batch) on the same seeded inputs, in
one process, the three calls alternating, HIP-event times of the whole call with inputs and outputs resident on the
device, behind a warm-up that covers the clock ramp.  Not part of bench.py.

    python tools/bench_weighted.py [--steps 20] [--warmup-s 2.0] [--shapes seam,full]

One JSON line per shape: median ms per call of NONE (the plain call), band ([-0.25, 0.25] cycles per sample) and band +
PHAT, and the two ratios to NONE.  Seam shapes: one window of 3 and of 8 buoys at N = 256, 4096, 8192, 16384 (the
reference's one frequency group per call); full batches: cfg3 (8 x 4096 x 4096), 3 x 1024 x 8192, 8 x 256 x 16384."""
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
BAND = (-0.25, 0.25)


def run_shape(xcorr, torch, B, W, N, steps, warmup_s):
    P = B * (B - 1) // 2
    rng = np.random.default_rng(1)
    iq = (rng.standard_normal((W, B, N)) + 1j * rng.standard_normal((W, B, N))).astype(np.complex64) * 30
    d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
    del iq
    modes = {"none": (None, False), "band": (BAND, False), "band_phat": (BAND, True)}
    outs = {m: (torch.empty((W, P), dtype=torch.int32, device="cuda"), torch.empty((W, P), dtype=torch.float32, device="cuda"),
                torch.empty((W, P), dtype=torch.float32, device="cuda")) for m in modes}
    with xcorr.XcorrEngine(B, N, W) as eng:
        stream = torch.cuda.current_stream()
        eng.set_stream(stream.cuda_stream)

        def call(m):
            li, lf, pk = outs[m]
            band, phat = modes[m]
            eng.correlate_device(d_iq.data_ptr(), W, li.data_ptr(), lf.data_ptr(), pk.data_ptr(), band=band, whiten=phat)

        t_end = time.time() + warmup_s
        while time.time() < t_end:
            for m in modes:
                call(m)
            torch.cuda.synchronize()
        times = {m: [] for m in modes}
        order = list(modes)
        for s in range(steps):
            for m in (order if s % 2 == 0 else order[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call(m)
                e1.record(stream)
                e1.synchronize()
                times[m].append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
    med = {m: float(np.median(times[m])) for m in modes}
    return {"buoys": B, "windows": W, "n_samples": N, "steps": steps, "band_cps": list(BAND),
            "none_ms": round(med["none"], 4), "band_ms": round(med["band"], 4), "band_phat_ms": round(med["band_phat"], 4),
            "band_ratio": round(med["band"] / med["none"], 3), "band_phat_ratio": round(med["band_phat"] / med["none"], 3)}


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
