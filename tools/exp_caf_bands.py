"""GPU box: the Doppler search under M bands through ONE banded call (rmx_caf_batch_bands: (1 + D) B forward transforms and
M D P inverse ones, one copy of the samples) against the M single-band searches that were the only way before (M calls of
rmx_caf_batch_request, one per band, over the same windows: M ((1 + D) B + D P) transforms).  Device-resident input and
output, a warm-up per shape, a synchronised host clock over at least 0.2 s of calls per figure, the two sides alternating
in one process, three figures a side: the median and the spread (max - min) / median.  One host-array row, where the single
upload counts.
usage: python tools/exp_caf_bands.py [--quick] [--baseline-only] [--tree DIR]
  --baseline-only   the M single-band calls alone (rmx_caf_batch_request, whose kernels the banded entry does not share on
                    the pair side: the figure of a build of the parent commit, via --tree, shows whether they moved)
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
D = 21


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
    """M disjoint bands of equal width over [-0.4, 0.4], shared by every window"""
    edges = np.linspace(-0.4, 0.4, M + 1)
    return np.stack([edges[:-1], edges[1:] - 1e-3], -1)


def row(B, N, W, M, phat=False, host=False, chunk=0):
    P = B * (B - 1) // 2
    g = torch.Generator(device="cuda").manual_seed(N + W + B)
    d_iq = torch.randn((W, B, N, 2), generator=g, device="cuda", dtype=torch.float32) * 20.0
    bands = bands_for(M)
    grid = (np.arange(D) - D // 2) * (0.5 / N)
    outs = [torch.zeros((W, M, P), dtype=t, device="cuda") for t in (torch.int32, torch.int32, torch.float32, torch.float32)]
    ptrs = [o.data_ptr() for o in outs]
    per_band = [[torch.zeros((W, P), dtype=t, device="cuda") for t in (torch.int32, torch.int32, torch.float32, torch.float32)]
                for _ in range(M)]
    band_ptrs = [[o.data_ptr() for o in q] for q in per_band]
    torch.cuda.synchronize()
    with xcorr.XcorrEngine(B, N, W) as eng:
        if chunk:                               # N = 4096: the per-hypothesis sweep over chunks instead of one launch
            eng.set_option("chunk_windows", chunk)
        if host:
            h_iq = d_iq.cpu().numpy().view(np.complex64).reshape(W, B, N)
            one = lambda: eng.caf_bands(h_iq, grid, bands, whiten=phat)                                   # noqa: E731

            def sep():
                for m in range(M):
                    eng.caf(h_iq, grid, band=bands[m], whiten=phat)
        else:
            one = lambda: eng.caf_bands_device(d_iq.data_ptr(), W, grid, bands, *ptrs, whiten=phat)       # noqa: E731

            def sep():
                for m in range(M):
                    eng.caf_device(d_iq.data_ptr(), W, grid, *band_ptrs[m], band=bands[m], whiten=phat)
        sides = [("sep", sep)] if args.baseline_only else [("one", one), ("sep", sep)]
        for _, fn in sides:                     # warm-up: buffers, staging, the phasor table, clocks
            for _ in range(3):
                fn()
        eng.synchronize()
        if not host and not args.baseline_only:   # the two sides answer alike (bit for bit off the four-step anchor route)
            one()
            sep()
            eng.synchronize()
            same = all(torch.equal(outs[k][:, m], per_band[m][k]) for m in range(M) for k in range(4))
        else:
            same = None
        got = {k: [] for k, _ in sides}
        for _ in range(3):                      # alternate the sides
            for k, fn in sides:
                got[k].append(timed(fn, eng.synchronize) * 1e6)
    med = {k: statistics.median(v) for k, v in got.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in got.items()}
    model = ((1 + D) * B + M * D * P) / (M * ((1 + D) * B + D * P))
    head = f"B={B} N={N:5d} W={W:3d}{'/%-2d' % chunk if chunk else '   '} D={D} M={M} {'PHAT' if phat else 'NONE'} {'host  ' if host else 'device'}"
    if args.baseline_only:
        print(f"{head}  M calls {med['sep']:9.1f} us (spread {100 * spread['sep']:4.1f} %)", flush=True)
    else:
        print(f"{head}  banded {med['one']:9.1f} us ({100 * spread['one']:4.1f} %)  M calls {med['sep']:9.1f} us "
              f"({100 * spread['sep']:4.1f} %)  banded/M calls {med['one'] / med['sep']:5.2f}  transforms {model:4.2f}"
              + ("" if same is None else "  same bits" if same else "  bits differ"), flush=True)


print(xcorr.build_info()["text"], flush=True)
print("transforms = ((1 + D) B + M D P) / (M ((1 + D) B + D P))", flush=True)
# N = 4096 in one launch (1 and 8 windows), N = 4096 in chunks (64 windows, W/16: option chunk_windows = 16), N = 8192 (8 windows)
shapes = [(4096, 1, 0), (4096, 8, 0), (4096, 64, 16), (8192, 8, 0)]
if args.quick:
    shapes = [(4096, 1, 0), (8192, 8, 0)]
for B in (3, 8):
    for N, W, chunk in shapes:
        for M in (2, 4, 8):
            row(B, N, W, M, chunk=chunk)
row(3, 4096, 8, 4, phat=True)
row(3, 8192, 8, 4, phat=True)
for M in (2, 8):
    row(3, 4096, 8, M, host=True)
row(8, 8192, 8, 4, host=True)
