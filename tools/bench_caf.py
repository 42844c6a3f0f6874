#!/usr/bin/env python3
"""GPU box: the Doppler search (rmx_caf_batch / rmx_caf_batch_request / rmx_caf_batch_quality / rmx_caf_batch_integrated) at
one shape, device arrays in and out.
usage: bench_caf.py B N W D [--whiten] [--band LO HI] [--bounds HALF] [--fine] [--refine U] [--quality] [--integrate K]
                    [--host] [--reps R] [--rounds K] [--option KEY VALUE]... [--timing]

  --whiten       PHAT                                      --band LO HI   keep [LO, HI] cycles per sample
  --bounds HALF  per-window lag intervals of +-HALF samples around the true lags
  --fine         with the sub-grid Doppler estimate (dop_frac)
  --refine U     the fine lag search on each slot's winning hypothesis       --quality   with the four quality figures
  --integrate K  one peak search per group of K consecutive windows (the windows of a group share their delays); the
                 outputs and --bounds are then per group
  --option K V   an engine option (chunk_windows 16: the per-hypothesis route in chunks)
  --timing       one more call under the timing option: the per-family times of its launches
  --host         host arrays in and out (XcorrEngine.caf: the copies and the synchronisation are part of every call)

Each round times R back-to-back calls between two stream synchronisations and reports the time per call; the line gives
the rounds' median and their spread (min .. max), so two builds can be compared by running them in turn.  The package is
imported from RMX_BENCH_ROOT when that is set (another checkout with its own build), else from this tree."""
import argparse
import os
import sys
import time

ROOT = os.environ.get("RMX_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import radio_mapper_amd as rm  # noqa: E402
from radio_mapper_amd import xcorr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("shape", type=int, nargs=4, metavar=("B", "N", "W", "D"))
ap.add_argument("--whiten", action="store_true")
ap.add_argument("--band", type=float, nargs=2, metavar=("LO", "HI"))
ap.add_argument("--bounds", type=int, metavar="HALF")
ap.add_argument("--fine", action="store_true")
ap.add_argument("--refine", type=int, default=0)
ap.add_argument("--quality", action="store_true")
ap.add_argument("--integrate", type=int, default=1)
ap.add_argument("--option", nargs=2, action="append", default=[], metavar=("KEY", "VALUE"))
ap.add_argument("--timing", action="store_true")
ap.add_argument("--host", action="store_true")
ap.add_argument("--reps", type=int, default=0, help="calls per round (default: enough for about 0.3 s)")
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()
xcorr.apply_env_options(report=sys.stderr)   # (a refused knob raises) RMX_<KEY>=<int> of the calling shell -> default options
B, N, W, D = args.shape
fs = 20e6
step = 50.0 / fs
grid = (np.arange(D) - D // 2) * step
rng = np.random.default_rng(5)
offs = rng.integers(-(D // 2) + 1, D // 2, size=B) * step * 0.5
iq, delays = rm.synth.make_windows(W, B, N, fs, seed=1005, doppler_cps=offs)
K = args.integrate
if K > 1:   # (the windows of a group hear the emitter at the delays of the group's first window)
    iq, delays = rm.synth.make_windows(W, B, N, fs, seed=1005, doppler_cps=offs, delays=np.repeat(delays[::K], K, axis=0))
    delays = delays[::K]
G = W // K
pl = xcorr.pair_list(B)
P = len(pl)
true = delays[:, pl[:, 1]] - delays[:, pl[:, 0]]
kw = {}
if args.whiten:
    kw["whiten"] = True
if args.band:
    kw["band"] = np.array(args.band)
if args.bounds is not None:
    r = np.rint(true).astype(np.int64)
    kw["lag_bounds"] = np.stack([np.clip(r - args.bounds, -(N - 1), N - 1), np.clip(r + args.bounds, -(N - 1), N - 1)], -1).astype(np.int32)
dev = torch.device("cuda", 0)
x = torch.from_numpy(np.ascontiguousarray(iq).view(np.float32).reshape(W, B, N, 2)).to(dev)
out = [torch.zeros((G, P), dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.float32, torch.float32, torch.float32)]
if args.fine:
    kw["fine" if args.host else "dop_frac_ptr"] = True if args.host else out[4].data_ptr()
if args.refine:
    kw["refine"] = args.refine
qual = torch.zeros((G, P, 4), dtype=torch.float32, device=dev)
if args.quality:
    kw["quality" if args.host else "quality_ptr"] = True if args.host else qual.data_ptr()
if K > 1:
    kw["integrate"] = K
eng = xcorr.XcorrEngine(B, N, W)
for key, value in args.option:
    eng.set_option(key, int(value))
eng.set_stream(torch.cuda.current_stream().cuda_stream)


def call():
    if args.host:
        res = eng.caf(iq, grid, **kw)
        res = res[:-1] if args.quality else res
        out[1], out[2] = torch.from_numpy(res[-3]), torch.from_numpy(res[-2])
        return
    eng.caf_device(x.data_ptr(), W, grid, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), **kw)


call()
eng.synchronize()
t0 = time.perf_counter()
call()
eng.synchronize()
one = time.perf_counter() - t0
reps = args.reps or max(1, min(2000, int(0.3 / max(one, 1e-6))))
per_call = []
for _ in range(args.rounds):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    eng.synchronize()
    per_call.append((time.perf_counter() - t0) / reps)
li, lf = out[1].cpu().numpy(), out[2].cpu().numpy()
ok = np.mean(np.abs(li + lf - true) < 1.0)
med, lo, hi = np.median(per_call), min(per_call), max(per_call)
what = " ".join([k for k in ("whiten", "band", "lag_bounds", "dop_frac_ptr", "fine", "quality_ptr", "quality") if k in kw]
                + ["refine=%d" % args.refine] * bool(args.refine) + ["integrate=%d" % K] * (K > 1)
                + ["%s=%s" % (k, v) for k, v in args.option] + ["host"] * args.host) or "plain"
print(f"caf B={B} N={N} W={W} D={D} [{what}] {xcorr.build_info().get('source_digest')}: {med * 1e6:.1f} us per call "
      f"(median of {args.rounds} rounds of {reps}, {lo * 1e6:.1f} .. {hi * 1e6:.1f}) = {W * P * D * N / med / 1e9:.2f} Gsample-bins/s; "
      f"lags within 1 sample of the truth: {ok * 100:.1f}%  scratch {eng.scratch_bytes() / 2**30:.2f} GiB", flush=True)
if args.timing:
    eng.set_option("timing", 1)
    call()
    eng.synchronize()
    fam = eng.last_timing_by_kernel()
    print("  per family: " + ", ".join("%s %d launches %.1f us" % (k, v["launches"], 1e3 * v["ms"]) for k, v in fam.items()), flush=True)
