"""GPU box: integrated, refined and qualified lags of M bands per window through ONE call
(rmx_xcorr_batch_bands_integrated with refine = 8 and quality: B + M P transforms per window) against the only way a
caller had before, M calls of the single-band correlate(..., band=, integrate=K, refine=8, quality=True) over the same
windows (M (B + P) transforms per window).  Device-resident input and output, a warm-up per shape, a synchronised host
clock over at least 0.2 s of calls per figure, the two sides alternating in one process, three figures a side: the median
and the spread (max - min) / median.  One more figure with host arrays in and out, where the single upload counts.
usage: python tools/exp_multiband_integrated.py [--quick] [--fill] [--buoys B] [--out FILE]
  --fill        the rows with 128 groups of K = 8 instead (1024 windows a call: batches that fill the chip, where the
                transform count and not the per-call floor decides)
  --buoys B     the rows of B buoys only (a driver script runs one B per process, each under its own time limit)
  --out FILE    also append every line to FILE"""
import argparse
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true")
ap.add_argument("--fill", action="store_true")
ap.add_argument("--buoys", type=int, default=0)
ap.add_argument("--out", default="")
args = ap.parse_args()
sys.path.insert(0, ".")
import numpy as np   # noqa: E402
import torch         # noqa: E402
from radio_mapper_amd import xcorr   # noqa: E402

MIN_S = 0.2
U = 8


def say(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fn, sync):
    """seconds per call over at least MIN_S of calls"""
    n, t = 1, 0.0
    while True:
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        t = time.perf_counter() - t0
        if t >= MIN_S:
            return t / n
        n = max(n + 1, int(n * 1.2 * MIN_S / max(t, 1e-6)))


def bands_for(M):
    """M disjoint bands over [-0.4, 0.4], shared by every window"""
    c = -0.4 + (np.arange(M) + 0.5) * 0.8 / M
    return np.stack([c - 0.35 / M, c + 0.35 / M], -1)


def measure(sides, sync):
    for _, fn in sides:                     # warm-up: buffers, staging, clocks
        for _ in range(3):
            fn()
    sync()
    got = {k: [] for k, _ in sides}
    for _ in range(3):                      # alternate the sides
        for k, fn in sides:
            got[k].append(timed(fn, sync) * 1e6)
    med = {k: statistics.median(v) for k, v in got.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in got.items()}
    return med, spread


def row(B, N, K, G, M, host=False):
    P, W = B * (B - 1) // 2, G * K
    g = torch.Generator(device="cuda").manual_seed(N + W + B)
    d_iq = torch.randn((W, B, N, 2), generator=g, device="cuda", dtype=torch.float32) * 20.0
    bands = bands_for(M)
    outs = [torch.zeros((G, M, P), dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.float32)]
    d_q = torch.zeros((G, M, P, 4), dtype=torch.float32, device="cuda")
    ptrs = [o.data_ptr() for o in outs]
    head = f"B={B} N={N:5d} K={K:2d} G={G:3d} M={M}" + (" host arrays" if host else "")
    with xcorr.XcorrEngine(B, N, W) as eng:
        if host:
            iq = d_iq.cpu().numpy().view(np.complex64).reshape(W, B, N)
            one = lambda: eng.correlate_bands(iq, bands, refine=U, quality=True, integrate=K)   # noqa: E731

            def rep():
                for m in range(M):
                    eng.correlate(iq, band=bands[m], integrate=K, refine=U, quality=True)
        else:
            one = lambda: eng.correlate_bands_device(d_iq.data_ptr(), W, bands, *ptrs, refine=U, quality_ptr=d_q.data_ptr(),   # noqa: E731
                                                     integrate=K)

            def rep():
                for m in range(M):
                    eng.correlate_device(d_iq.data_ptr(), W, *ptrs, band=bands[m], integrate=K, refine=U, quality_ptr=d_q.data_ptr())
        med, spread = measure([("one", one), ("rep", rep)], eng.synchronize)
    model = (B + M * P) / (M * (B + P))
    say(f"{head}  one call {med['one']:9.1f} us ({100 * spread['one']:4.1f} %)  M calls {med['rep']:9.1f} us "
        f"({100 * spread['rep']:4.1f} %)  one/M calls {med['one'] / med['rep']:5.2f}  transforms "
        f"(B + M P) / (M (B + P)) = {model:4.2f}")


say(xcorr.build_info()["text"])
for B in ((args.buoys,) if args.buoys else (3, 8)):
    for N in ((4096,) if args.quick else (1024, 4096, 8192)):
        for K, G in (((8, 128),) if args.fill else ((8, 8),) if args.quick else ((8, 8), (64, 2))):
            for M in (2, 4, 8):
                row(B, N, K, G, M)
    row(B, 4096, 8, 128 if args.fill else 8, 4, host=True)
