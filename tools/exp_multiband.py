"""GPU box: M bands per window through ONE banded call (rmx_xcorr_batch_bands: B + M P transforms, one copy of the samples)
against the repeated-window call that was the only way before (correlate(np.repeat(iq, M, 0), band=per-window):
M (B + P) transforms, M times the input).  Device-resident input and output, a warm-up per shape, a synchronised host
clock over at least 0.2 s of calls per figure, the two sides alternating in one process, three figures a side: the median
and the spread (max - min) / median.  One host-pointer row, where the copy of the samples counts.
usage: python tools/exp_multiband.py [--quick] [--baseline-only] [--tree DIR]
  --baseline-only   the repeated-window call alone (its kernels are not the banded call's: the figure of a build of the
                    parent commit, via --tree, shows whether it moved)
  --tree DIR        import the package (and its library) from the checkout at DIR instead of this one"""
import argparse
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true")
ap.add_argument("--baseline-only", action="store_true")
ap.add_argument("--tree", default=".")
args = ap.parse_args()
sys.path.insert(0, args.tree)
import numpy as np   # noqa: E402
import torch         # noqa: E402
from radio_mapper_amd import xcorr   # noqa: E402

MIN_S = 0.2


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


def bands_for(M, W, rng):
    """M disjoint bands of equal width over [-0.4, 0.4], the same for every window"""
    edges = np.linspace(-0.4, 0.4, M + 1)
    return np.tile(np.stack([edges[:-1], edges[1:] - 1e-3], -1), (W, 1, 1))


def row(B, N, W, M, phat, host=False):
    P = B * (B - 1) // 2
    g = torch.Generator(device="cuda").manual_seed(N + W + B)
    d_iq = torch.randn((W, B, N, 2), generator=g, device="cuda", dtype=torch.float32) * 20.0
    d_rep = d_iq.repeat_interleave(M, dim=0).contiguous()          # window-major, as np.repeat(iq, M, 0)
    bands = bands_for(M, W, None)
    rep_band = bands.reshape(W * M, 2)
    outs = [torch.zeros((W * M, P), dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.float32)]
    ptrs = [o.data_ptr() for o in outs]
    torch.cuda.synchronize()
    with xcorr.XcorrEngine(B, N, W * M) as eng:
        if host:
            h_iq = d_iq.cpu().numpy().view(np.complex64).reshape(W, B, N)
            h_rep = np.repeat(h_iq, M, axis=0)
            one = lambda: eng.correlate_bands(h_iq, bands, whiten=phat)                        # noqa: E731
            rep = lambda: eng.correlate(h_rep, band=rep_band, whiten=phat)                     # noqa: E731
        else:
            one = lambda: eng.correlate_bands_device(d_iq.data_ptr(), W, bands, *ptrs, whiten=phat)             # noqa: E731
            rep = lambda: eng.correlate_device(d_rep.data_ptr(), W * M, *ptrs, band=rep_band, whiten=phat)     # noqa: E731
        sides = [("rep", rep)] if args.baseline_only else [("one", one), ("rep", rep)]
        for _, fn in sides:                     # warm-up: buffers, staging, clocks
            for _ in range(3):
                fn()
        eng.synchronize()
        got = {k: [] for k, _ in sides}
        for _ in range(3):                      # alternate the sides
            for k, fn in sides:
                got[k].append(timed(fn, eng.synchronize) * 1e6)
    med = {k: statistics.median(v) for k, v in got.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in got.items()}
    model = (B + M * P) / (M * (B + P))
    head = f"B={B} N={N:5d} W={W:4d} M={M} {'PHAT' if phat else 'NONE'} {'host  ' if host else 'device'}"
    if args.baseline_only:
        print(f"{head}  repeated {med['rep']:9.1f} us (spread {100 * spread['rep']:4.1f} %)", flush=True)
    else:
        print(f"{head}  banded {med['one']:9.1f} us ({100 * spread['one']:4.1f} %)  repeated {med['rep']:9.1f} us "
              f"({100 * spread['rep']:4.1f} %)  banded/repeated {med['one'] / med['rep']:5.2f}  transforms "
              f"(B + M P) / (M (B + P)) = {model:4.2f}", flush=True)


print(xcorr.build_info()["text"], flush=True)
shapes = [(4096, 64), (4096, 1024), (8192, 256), (16384, 128)]
if args.quick:
    shapes = [(4096, 64), (8192, 32)]
for B in (3, 8):
    for N, W in shapes:
        for M in (2, 4, 8):
            for phat in (False, True):
                row(B, N, W, M, phat)
if not args.baseline_only:
    for M in (2, 8):
        row(3, 4096, 64, M, False, host=True)
    row(8, 8192, 64, 4, False, host=True)
