"""GPU box: refined and qualified lags of M bands per window through ONE banded call (rmx_xcorr_batch_bands_quality with
refine = 8 and quality: B + M P transforms, M P refine and quality slots that read their band only) against the only way a
caller had before, M repeated windows through correlate(..., band=, refine=8, quality=True) (M (B + P) transforms, M P
slots that each read two full spectra).  Device-resident input and output, a warm-up per shape, a synchronised host clock
over at least 0.2 s of calls per figure, the two sides alternating in one process, three figures a side: the median and the
spread (max - min) / median, and the per-family kernel times of one call of either side.
usage: python tools/exp_multiband_quality.py [--quick] [--buoys B] [--plain] [--tree DIR]
  --buoys B     the rows of B buoys only (a driver script runs one B per process, each under its own time limit)
  --plain       the banded call WITHOUT refine or quality alone (rmx_xcorr_batch_bands): the figure of a build of the
                parent commit, via --tree, shows whether it moved
  --tree DIR    import the package (and its library) from the checkout at DIR instead of this one"""
import argparse
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true")
ap.add_argument("--buoys", type=int, default=0)
ap.add_argument("--plain", action="store_true")
ap.add_argument("--tree", default=".")
args = ap.parse_args()
sys.path.insert(0, args.tree)
import numpy as np   # noqa: E402
import torch         # noqa: E402
from radio_mapper_amd import xcorr   # noqa: E402

MIN_S = 0.2
U = 8


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


def bands_for(M, W, width):
    """M disjoint bands of `width` cycles per sample each, centred on equal steps over [-0.4, 0.4]; width 0.4: M overlapping
    bands whose lower edges step over [-0.4, 0.0]"""
    if width * M <= 0.8:
        c = -0.4 + (np.arange(M) + 0.5) * 0.8 / M
        b = np.stack([c - width / 2, c + width / 2], -1)
    else:
        lo = np.linspace(-0.4, 0.4 - width, M)
        b = np.stack([lo, lo + width], -1)
    return np.tile(b, (W, 1, 1))


def families(eng, fn):
    eng.set_option("timing", 1)
    fn()
    eng.synchronize()
    tk = eng.last_timing_by_kernel()
    eng.set_option("timing", 0)
    return " ".join("%s %.0f" % (k, 1e3 * v["ms"]) for k, v in sorted(tk.items()))


def row(B, N, W, M, width):
    P = B * (B - 1) // 2
    g = torch.Generator(device="cuda").manual_seed(N + W + B)
    d_iq = torch.randn((W, B, N, 2), generator=g, device="cuda", dtype=torch.float32) * 20.0
    bands = bands_for(M, W, width)
    rep_band = bands.reshape(W * M, 2)
    outs = [torch.zeros((W * M, P), dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.float32)]
    d_q = torch.zeros((W * M, P, 4), dtype=torch.float32, device="cuda")
    ptrs = [o.data_ptr() for o in outs]
    head = f"B={B} N={N:5d} W={W:4d} M={M} width {width:4.2f}"
    with xcorr.XcorrEngine(B, N, W * M) as eng:
        if args.plain:
            plain = lambda: eng.correlate_bands_device(d_iq.data_ptr(), W, bands, *ptrs)   # noqa: E731
            for _ in range(3):
                plain()
            got = [timed(plain, eng.synchronize) * 1e6 for _ in range(3)]
            med = statistics.median(got)
            print(f"{head}  banded, nothing requested {med:9.1f} us ({100 * (max(got) - min(got)) / med:4.1f} %)", flush=True)
            return
        d_rep = d_iq.repeat_interleave(M, dim=0).contiguous()          # window-major, as np.repeat(iq, M, 0)
        torch.cuda.synchronize()
        one = lambda: eng.correlate_bands_device(d_iq.data_ptr(), W, bands, *ptrs, refine=U, quality_ptr=d_q.data_ptr())   # noqa: E731
        rep = lambda: eng.correlate_device(d_rep.data_ptr(), W * M, *ptrs, band=rep_band, refine=U,                       # noqa: E731
                                           quality_ptr=d_q.data_ptr())
        sides = [("one", one), ("rep", rep)]
        for _, fn in sides:                     # warm-up: buffers, staging, clocks
            for _ in range(3):
                fn()
        eng.synchronize()
        got = {k: [] for k, _ in sides}
        for _ in range(3):                      # alternate the sides
            for k, fn in sides:
                got[k].append(timed(fn, eng.synchronize) * 1e6)
        fam = {k: families(eng, fn) for k, fn in sides}
    med = {k: statistics.median(v) for k, v in got.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in got.items()}
    model = (B + M * P) / (M * (B + P))
    print(f"{head}  banded {med['one']:9.1f} us ({100 * spread['one']:4.1f} %)  repeated {med['rep']:9.1f} us "
          f"({100 * spread['rep']:4.1f} %)  banded/repeated {med['one'] / med['rep']:5.2f}  transforms "
          f"(B + M P) / (M (B + P)) = {model:4.2f}", flush=True)
    print(f"    us per family, one call: banded [{fam['one']}]  repeated [{fam['rep']}]", flush=True)


print(xcorr.build_info()["text"], flush=True)
shapes = [(4096, 64), (4096, 1024), (8192, 256), (16384, 128)]
if args.quick:
    shapes = [(4096, 64), (8192, 32)]
for B in ((args.buoys,) if args.buoys else (3, 8)):
    for N, W in shapes:
        for M in (2, 4, 8):
            for width in (0.05, 0.4):
                row(B, N, W, M, width)
