"""The reference side of the Doppler-search tests (rmx_caf_batch): oracle/xcorr_ref.py's caf_pair taken apart so that a
test sees every hypothesis, not only the winner.  bin_peaks runs the oracle's per-hypothesis correlation, first_max is
caf_pair's selection rule (d-major first maximum: strict >, ties keep the lowest d), hypothesis_margin is the condition
under which "dop_idx exact" is a fair demand, winner_margins the ones for the lag of the winning row.  libm_phasor is the
phasor table as rmx_caf_batch builds it, rot_mul the product as the kernels round it, scene the seeded windows with
on-grid frequency offsets.  A helper of tests/test_caf_ref_cpu.py and tests/test_gpu_caf.py, not part of the oracle."""
import math

import numpy as np

import radio_mapper_amd as rm
from oracle import xcorr_ref as orc

MARGIN_BAR = 1e-3   # test_caf_golden's bar on the gap between the best and the second-best hypothesis


def _pairs(pairs, n_buoys):
    return orc.pair_list(n_buoys) if pairs is None else np.asarray(pairs, np.int32).reshape(-1, 2)


def rotated(x, nu, n_samples):
    """x_j de-rotated by hypothesis nu exactly as caf_pair does it"""
    return (np.ascontiguousarray(x, np.complex64) * orc.doppler_phasor(nu, n_samples)).astype(np.complex64)


def bin_peaks(iq, grid, pairs=None):
    """(peak float32, lag_int int32, lag_frac float64), each [W][P][D]: xcorr_pair of every hypothesis of every pair-window"""
    iq = np.asarray(iq)
    W, B, N = iq.shape
    pl = _pairs(pairs, B)
    grid = np.asarray(grid, np.float64).reshape(-1)
    pk = np.zeros((W, len(pl), len(grid)), np.float32)
    li = np.zeros((W, len(pl), len(grid)), np.int32)
    lf = np.zeros((W, len(pl), len(grid)), np.float64)
    for w in range(W):
        for d, nu in enumerate(grid):
            ph = orc.doppler_phasor(nu, N)
            y = {}
            for q, (i, j) in enumerate(pl.tolist()):
                if j not in y:
                    y[j] = (np.ascontiguousarray(iq[w, j], np.complex64) * ph).astype(np.complex64)
                li[w, q, d], lf[w, q, d], pk[w, q, d] = orc.xcorr_pair(iq[w, i], y[j])
    return pk, li, lf


def first_max(peaks):
    """index of the d-major first maximum along the last axis: d wins only with peak[d] > the best so far (caf_pair)"""
    peaks = np.asarray(peaks)
    best = np.zeros(peaks.shape[:-1], np.int32)
    top = peaks[..., 0].copy()
    for d in range(1, peaks.shape[-1]):
        better = peaks[..., d] > top
        best[better] = d
        top = np.where(better, peaks[..., d], top)
    return best


def take(a, idx):
    """a[w, q, idx[w, q]]"""
    return np.take_along_axis(np.asarray(a), np.asarray(idx)[..., None].astype(np.int64), axis=-1)[..., 0]


def hypothesis_margin(peaks):
    """(best - second best) / best over the hypotheses of each pair-window, float64 [W][P]; inf for a single hypothesis,
    0 where the best is 0"""
    p = np.sort(np.asarray(peaks, np.float64), axis=-1)
    if p.shape[-1] < 2:
        return np.full(p.shape[:-1], np.inf)
    top = p[..., -1]
    return np.where(top > 0, (top - p[..., -2]) / np.where(top > 0, top, 1.0), 0.0)


def winner_margins(iq, grid, dop, pairs=None):
    """For the winning row of each pair-window: (margin between the oracle's two largest magnitudes, lag of the second
    largest, oracle.parabola_ulp_bound), each [W][P] -- what the project's parity rule excuses a lag by"""
    iq = np.asarray(iq)
    W, B, N = iq.shape
    pl = _pairs(pairs, B)
    mg = np.zeros((W, len(pl)))
    second = np.zeros((W, len(pl)), np.int64)
    flat = np.zeros((W, len(pl)))
    for w in range(W):
        for q, (i, j) in enumerate(pl.tolist()):
            y = rotated(iq[w, j], grid[int(dop[w, q])], N)
            mg[w, q], _, second[w, q] = orc.peak_top2(iq[w, i], y)
            flat[w, q] = orc.parabola_ulp_bound(iq[w, i], y)
    return mg, second, flat


def reference(iq, grid, pairs=None):
    """Everything a GPU test compares with, computed once: dict of dop / lag_int / lag_frac / peak [W][P] (first_max over
    bin_peaks, which IS orc.caf_batch), bin_peak [W][P][D], hyp_margin, lag_margin, lag_second, flat_bound [W][P]"""
    pk, li, lf = bin_peaks(iq, grid, pairs)
    dop = first_max(pk)
    mg, second, flat = winner_margins(iq, grid, dop, pairs)
    return dict(dop=dop, lag_int=take(li, dop), lag_frac=take(lf, dop), peak=take(pk, dop), bin_peak=pk,
                hyp_margin=hypothesis_margin(pk), lag_margin=mg, lag_second=second, flat_bound=flat)


def libm_phasor(nu, n_samples):
    """The phasor table of one hypothesis exactly as rmx_caf_batch builds it: cos / sin of -6.283185307179586 * nu * n in
    double (the C library's, which Python's math module calls), each rounded once to float32"""
    out = np.empty(n_samples, np.complex64)
    nu = float(nu)
    for n in range(n_samples):
        a = -6.283185307179586 * nu * float(n)
        out[n] = np.float32(math.cos(a)) + 1j * np.float32(math.sin(a))
    return out


def rot_mul(x, r):
    """x * r as gen::rot_mul rounds it: four float32 products, one float32 difference and one float32 sum, nothing fused.
    (numpy's own complex64 product is NOT that on every machine: its SIMD loop fuses one product into the sum where the
    CPU has FMA.)"""
    x = np.asarray(x, np.complex64)
    r = np.asarray(r, np.complex64)
    xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    rr, ri = np.ascontiguousarray(r.real), np.ascontiguousarray(r.imag)
    out = np.empty(np.broadcast(x, r).shape, np.complex64)
    out.real = xr * rr - xi * ri
    out.imag = xr * ri + xi * rr
    return out


def scene(W, B, N, D, seed, fs=2.4e6, snr_db=10.0, spread=None):
    """Seeded windows for a Doppler search over D hypotheses: grid = (arange(D) - D // 2) * step, step = 0.5 / N cycles per
    sample; buoy b of window w carries the offset k[w][b] * step with whole k drawn from 0 ... spread (default D // 2), so
    that every pair's difference, in either order, is a grid point; consecutive windows never draw the same row of k.
    -> (iq complex64 [W][B][N], raw uint8 [W][B][2N] that decodes to iq, grid float64 [D], k int [W][B])"""
    step = 0.5 / N
    grid = (np.arange(D) - D // 2) * step
    spread = D // 2 if spread is None else int(spread)
    rng = np.random.default_rng(seed)
    k = np.zeros((W, B), np.int64)
    for w in range(W):
        k[w] = rng.integers(0, spread + 1, size=B)
        while spread > 0 and w > 0 and np.array_equal(k[w], k[w - 1]):
            k[w] = rng.integers(0, spread + 1, size=B)
    iq, _, raw = rm.synth.make_windows(W, B, N, fs, seed=seed, snr_db=snr_db, return_u8=True, doppler_cps=k * step)
    return iq, raw, grid, k


def custom_pairs(n_buoys):
    """a pair list with a reversed pair (B-1, 0) and a repeated one (0, 1)"""
    return np.array([(n_buoys - 1, 0), (0, 1), (1, n_buoys - 1), (0, 1)], np.int32)


CROSS_PAIRS = np.array([(0, 2), (0, 3), (1, 2), (1, 3)], np.int32)   # {0, 1} x {2, 3}: no buoy is both an i and a j

# Every seeded scene of tests/test_gpu_caf.py: name -> (W, B, N, D, seed).  tests/test_caf_ref_cpu.py checks the
# hypothesis margin of each (default and custom pair list) on the reference alone.
SCENES = {
    # small windows (g_fwd_small / g_pair_small)
    "n16": (5, 3, 16, 5, 19), "n256": (5, 4, 256, 7, 256), "n2048": (3, 4, 2048, 5, 2048), "g4096": (3, 3, 4096, 5, 4097),
    # four-step
    "n8192": (3, 3, 8192, 5, 8192), "n16384": (2, 5, 16384, 5, 16384), "n65536": (2, 3, 65536, 3, 65536),
    "n8192b6": (2, 6, 8192, 5, 8198),
    # N = 4096: all hypotheses in one launch (D W a multiple of 8 / not), per hypothesis over chunks of 8, 8 and 4
    "one8": (8, 4, 4096, 5, 40), "one3": (3, 3, 4096, 7, 21), "chunked": (20, 4, 4096, 5, 100),
    # chunk seams of the generic paths
    "seam256": (5, 3, 256, 5, 2560), "seam8192": (5, 3, 8192, 5, 81920),
}


def scene_of(name):
    W, B, N, D, seed = SCENES[name]
    return scene(W, B, N, D, seed)


def limit_scene():
    """n_dopplers at its limit: N = 256, 2 buoys, 1 window, 4096 evenly spaced hypotheses over the whole unambiguous
    range [-0.5, 0.5), the true offset on one of them.  Neighbouring hypotheses differ by 1/16 of a cycle over the window:
    delays of a few samples and 30 dB keep the best one 7e-3 above its neighbours.
    -> (iq, raw, grid, index of the true hypothesis)"""
    N, D, at = 256, 4096, 2048 + 517
    grid = (np.arange(D) - D // 2) / float(D)
    offs = np.array([[0.0, grid[at]]])
    iq, _, raw = rm.synth.make_windows(1, 2, N, 2.4e6, seed=4097, snr_db=30.0, return_u8=True, doppler_cps=offs,
                                       max_delay=8.0)
    return iq, raw, grid, at
