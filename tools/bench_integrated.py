"""Integrated against per-window cross-correlation (rmx_xcorr_batch_integrated vs rmx_xcorr_batch_weighted) on the same
seeded windows, in one process, the calls alternating, HIP-event times of the whole call with inputs and outputs resident
on the device, behind a warm-up that covers the clock ramp.  Not part of bench.py.

    python tools/bench_integrated.py [--steps 20] [--warmup-s 2.0] [--shapes full,capture,seam]

One JSON line per shape: median ms per call of `correlate(whiten=True)` (the baseline: a weighted call always takes the
per-transform kernels, so both sides run the same forward kernels and differ only in the pair / peak kernels; those
kernels are instruction-identical to the parent commit's, tools/isa_diff.py), of `correlate(whiten=True, integrate=K)` for
K = 4, 16, 64 with the ratio to the baseline, and of the plain call for orientation (it may take the whole-window kernels).
Shapes: 8 buoys x 4096 windows x N = 4096; 3 and 8 buoys x 4096 windows x N = 1024; the reference's capture lengths at
bench.py's shapes (N = 8192: 3 x 1024 and 8 x 512 windows; N = 16384: 3 x 512 and 8 x 256); the seam shape (3 buoys, one
group of 16 x 1024, K = 16 only)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL = [(8, 4096, 4096), (3, 4096, 1024), (8, 4096, 1024)]   # (buoys, windows, N)
CAPTURE = [(3, 1024, 8192), (8, 512, 8192), (3, 512, 16384), (8, 256, 16384)]
SEAM = [(3, 16, 1024)]
KS = (4, 16, 64)


def run_shape(xcorr, torch, B, W, N, ks, steps, warmup_s):
    P = B * (B - 1) // 2
    rng = np.random.default_rng(1)
    iq = (rng.standard_normal((W, B, N)) + 1j * rng.standard_normal((W, B, N))).astype(np.complex64) * 30
    d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
    del iq
    modes = {"plain": (False, 1), "phat": (True, 1)}
    modes.update({"phat_k%d" % k: (True, k) for k in ks})
    outs = {m: tuple(torch.empty((W // k, P), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.float32))
            for m, (_, k) in modes.items()}
    with xcorr.XcorrEngine(B, N, W) as eng:
        stream = torch.cuda.current_stream()
        eng.set_stream(stream.cuda_stream)

        def call(m):
            li, lf, pk = outs[m]
            phat, k = modes[m]
            eng.correlate_device(d_iq.data_ptr(), W, li.data_ptr(), lf.data_ptr(), pk.data_ptr(), whiten=phat, integrate=k)

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
    out = {"buoys": B, "windows": W, "n_samples": N, "steps": steps, "plain_ms": round(med["plain"], 4),
           "phat_ms": round(med["phat"], 4)}
    for k in ks:
        out["phat_k%d_ms" % k] = round(med["phat_k%d" % k], 4)
        out["k%d_ratio" % k] = round(med["phat_k%d" % k] / med["phat"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup-s", type=float, default=2.0)
    ap.add_argument("--shapes", default="full,capture,seam")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    groups = {"full": FULL, "capture": CAPTURE, "seam": SEAM}
    for grp in a.shapes.split(","):
        for B, W, N in groups[grp]:
            ks = (16,) if grp == "seam" else KS
            print(json.dumps(dict(group=grp, **run_shape(xcorr, torch, B, W, N, ks, a.steps, a.warmup_s))), flush=True)


if __name__ == "__main__":
    main()
