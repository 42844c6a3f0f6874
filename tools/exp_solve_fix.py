#!/usr/bin/env python3
"""GPU box: what rmx_solve_batch_fix costs beside rmx_solve_batch AS BUILT FROM THE PARENT COMMIT (device arrays in and
out, the scenario of tests/perf_solve.py: 8 buoys x 40 960 windows), and the same on the five-station sea-level scene of
tests/solve_fix_ref.py, where the plane mode walks a third of the iterations.

usage: python tools/exp_solve_fix.py --parent-lib PATH [--out FILE] [--calls N]
  --parent-lib  librmx_hip.so compiled from the parent commit's tree (a checkout of it, built with its own
                __graft_entry__.build(), gives radio-mapper_amd/csrc/librmx_hip.so)
The parent's call is timed twice in the same run (first and last in every round of calls): the difference of the two is
the run-to-run spread that the other figures are read against.  Every figure is the median of N >= 5 timed calls after
three warm-up calls, by HIP events around the call on the ctx stream; the versions alternate call by call."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import solve_fix_ref as fr  # noqa: E402
from radio_mapper_amd import xcorr  # noqa: E402
from radio_mapper_amd.tdoa_processor import GeodeticCalculator as G  # noqa: E402
from test_solve import scenario  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=25)
args = ap.parse_args()
assert args.calls >= 5

vp, ci, cu = C.c_void_p, C.c_int, C.c_uint
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
new = xcorr.load_library()
old = C.CDLL(os.path.abspath(args.parent_lib))
old.rmx_create.argtypes = [C.POINTER(vp), ci, ci, ci, ci, cu]
old.rmx_destroy.argtypes = [vp]
old.rmx_destroy.restype = None
old.rmx_set_stream.argtypes = [vp, vp]
old.rmx_solve_batch.argtypes = new.rmx_solve_batch.argtypes
old.rmx_build_info.restype = C.c_char_p
assert not hasattr(old, "rmx_solve_batch_fix"), "--parent-lib already has the new entry: it is not the parent's build"
lines = ["parent library: %s" % old.rmx_build_info().decode(), "this library:   %s" % new.rmx_build_info().decode()]


def ctx_of(lib, B):
    ctx = vp()
    assert lib.rmx_create(C.byref(ctx), 0, B, 4096, 1, 0) == 0
    assert lib.rmx_set_stream(ctx, vp(stream)) == 0
    return ctx


def timed_ms(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(title, buoys, li, lf, wgt, fs, plane):
    B, (W, P) = len(buoys), li.shape
    bx = np.ascontiguousarray(buoys, np.float64)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    dli, dlf, dwg = d(li), d(lf), None if wgt is None else d(wgt)
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)     # noqa: E731
    tp = lambda t: None if t is None else vp(t.data_ptr())                    # noqa: E731
    o_old = [z(W, 3), z(W), z(W, dt=torch.int32)]
    c_old, c_new = ctx_of(old, B), ctx_of(new, B)

    def parent():
        assert old.rmx_solve_batch(c_old, bx.ctypes.data_as(vp), B, None, P, tp(dli), tp(dlf), tp(dwg), float(fs), W, 60,
                                   *map(tp, o_old), 3) == 0

    def fix(pl, resid):
        n = 6 if pl is None else 3
        o = [z(W, 3), z(W), z(W, dt=torch.int32), z(W, n), z(W, n), z(W, P) if resid else None]
        plp = None if pl is None else pl.ctypes.data_as(vp)

        def call():
            assert new.rmx_solve_batch_fix(c_new, bx.ctypes.data_as(vp), B, None, P, tp(dli), tp(dlf), tp(dwg), float(fs), plp,
                                           W, 60, *map(tp, o), 3) == 0
        return call, o

    variants = [(name, pl, resid) + fix(pl, resid) for name, pl, resid in (
        ("three unknowns", None, False), ("three unknowns + resid", None, True), ("plane", plane, False),
        ("plane + resid", plane, True))]
    # every round times the parent's call, each variant, and the parent's call again: the versions alternate, and the two
    # parent columns differ by nothing but their place in the round
    order = [parent] + [v[3] for v in variants] + [parent]
    for _ in range(3):
        for call in order:
            call()
    torch.cuda.synchronize()
    ms = np.array([[timed_ms(call) for call in order] for _ in range(args.calls)])
    med = np.median(ms, axis=0)
    t_a, t_b = med[0], med[-1]
    rows = []
    for (name, pl, resid, call, o), t in zip(variants, med[1:-1]):
        rows.append((name, t, o[2].float().mean().item(), torch.isinf(o[4][:, 0]).float().mean().item()))
        if pl is None:
            assert all(torch.equal(a, b) for a, b in zip(o[:3], o_old)), "three unknowns: not the parent's bits"
    it_old = o_old[2].float().mean().item()
    lines.append("")
    lines.append("%s: B = %d, P = %d, W = %d, weights %s" % (title, B, P, W, "given" if wgt is not None else "none"))
    lines.append("  parent rmx_solve_batch          %8.3f ms first, %8.3f ms last (spread %+.1f %%), mean iterations %.1f" % (
        t_a, t_b, 100.0 * (t_b - t_a) / t_a, it_old))
    base = 0.5 * (t_a + t_b)
    for name, t, its, sing in rows:
        lines.append("  rmx_solve_batch_fix %-22s %8.3f ms = %.3f of the parent's call, mean iterations %.1f, singular %.4f" % (
            name, t, t / base, its, sing))
    lines.append("  three unknowns add one Jacobian pass to a walk of %.1f iterations of two passes each: the bar is "
                 "1 + 2 / iterations = %.3f" % (it_old, 1.0 + 2.0 / it_old))
    old.rmx_destroy(c_old)
    new.rmx_destroy(c_new)


buoys, tx, pairs, li, lf, fs = scenario(8, 40960, seed=5, noise_m=5.0)
lat, lng, _ = G.xyz_to_lat_lng(*buoys.mean(axis=0))
run("tests/perf_solve.py scenario", buoys, li, lf, None, fs, fr.as_plane(*G.tangent_plane(lat, lng, 150.0)))
buoys, emitter, plane = fr.scene("sea5")
pairs, li, lf, wgt = fr.noisy_lags(buoys, emitter, 40960, seed=1)
run("five sea-level stations", buoys, li, lf, wgt, fr.FS_SCENE, plane)
text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
