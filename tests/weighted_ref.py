"""The float32 reference of rmx_xcorr_batch_weighted (include/rmx.h): complex64 FFT_2N of each zero-padded window, the
band mask and PHAT applied in float32, the complex64 inverse with numpy's 1/L, the 'full' reorder, then the sliced peak
rule of tests/lag_bounds_ref.py.  A helper of tests/test_weighted_cpu.py and tests/test_gpu_weighted.py, not part of the
oracle."""
import math

import numpy as np
from scipy import fft as sp_fft

from lag_bounds_ref import peak_in_slice


def kept_bins(lo, hi, n_samples):
    """(s_lo, s_hi): the signed bins s in [-N, N-1] of the L = 2N point transform with lo <= s / L <= hi (s_lo > s_hi:
    none)"""
    L = 2 * n_samples
    return max(math.ceil(lo * L), -n_samples), min(math.floor(hi * L), n_samples - 1)


def mask(lo, hi, n_samples):
    """bool [L] over the natural bins k (signed s = k, or k - L for k >= N)"""
    L = 2 * n_samples
    s = np.fft.fftfreq(L, 1.0 / L).astype(np.int64)        # 0, 1, ..., N-1, -N, ..., -1
    s_lo, s_hi = kept_bins(lo, hi, n_samples)
    return (s >= s_lo) & (s <= s_hi)


def weighted_spectrum(x, band=None, phat=False):
    """Y = M X (NONE) or M X / |X| (PHAT, 0 where X == 0), complex64 [2N]"""
    N = x.shape[-1]
    X = sp_fft.fft(np.asarray(x, np.complex64), 2 * N)
    if phat:
        a = np.abs(X)
        X = np.where(a > 0, X / np.where(a > 0, a, np.float32(1)), np.complex64(0)).astype(np.complex64)
    if band is not None:
        X = np.where(mask(band[0], band[1], N), X, np.complex64(0)).astype(np.complex64)
    return X


def weighted_full(x_i, x_j, band=None, phat=False):
    """|r| in 'full' order (2N-1 lags, float32), r = IFFT_L(Y_j conj(Y_i))"""
    N = x_i.shape[-1]
    L = 2 * N
    r = sp_fft.ifft(weighted_spectrum(x_j, band, phat) * np.conj(weighted_spectrum(x_i, band, phat)))
    r = np.asarray(r, np.complex64)
    return np.abs(np.concatenate([r[L - (N - 1):], r[:N]])).astype(np.float32)


def flat_bound(m, n_samples, lag_int, lo, hi):
    """what one float32 ulp on each of the three taps of the peak moves the interpolated lag, relative to max(|lag|, 1)
    (oracle.xcorr_ref.parabola_ulp_bound on the weighted vector): the flat-peak part of the parity rule"""
    k = lag_int + n_samples - 1
    if lag_int <= lo or lag_int >= hi:
        return 0.0
    a, b, c = (float(v) for v in m[k - 1:k + 2])
    den = a - 2.0 * b + c
    if den == 0.0:
        return 0.0
    ulp = float(np.spacing(np.float32(b)))
    pa = 0.5 * (1.0 / den - (a - c) / den ** 2)
    pb = (a - c) / den ** 2
    pc = 0.5 * (-1.0 / den - (a - c) / den ** 2)
    lag = lag_int + 0.5 * (a - c) / den
    return (abs(pa) + abs(pb) + abs(pc)) * ulp / max(abs(lag), 1.0)


def weighted_batch(iq, band=None, phat=False, lag_bounds=None, pairs=None, with_bound=False):
    """iq complex64 [W][B][N]; band None / [2] / [W][2]; lag_bounds None / [P][2] / [W][P][2] ->
    (lag_int, lag_frac, peak, margin, full_max), each [W][P]; with_bound: and flat_bound [W][P] as a sixth"""
    W, B, N = iq.shape
    if pairs is None:
        pairs = [(i, j) for i in range(B) for j in range(i + 1, B)]
    pairs = np.asarray(pairs).reshape(-1, 2)
    P = pairs.shape[0]
    bd = None if band is None else np.broadcast_to(np.asarray(band, np.float64), (W, 2))
    lb = np.array([[-(N - 1), N - 1]] * P) if lag_bounds is None else np.asarray(lag_bounds)
    if lb.ndim == 2:
        lb = np.broadcast_to(lb, (W,) + lb.shape)
    li = np.zeros((W, P), np.int64)
    lf = np.zeros((W, P), np.float64)
    pk = np.zeros((W, P), np.float64)
    mg = np.zeros((W, P), np.float64)
    fm = np.zeros((W, P), np.float64)
    fb = np.zeros((W, P), np.float64)
    for w in range(W):
        spec = [weighted_spectrum(iq[w, b], None if bd is None else bd[w], phat) for b in range(B)]
        for q, (i, j) in enumerate(pairs):
            r = np.asarray(sp_fft.ifft(spec[j] * np.conj(spec[i])), np.complex64)
            m = np.abs(np.concatenate([r[2 * N - (N - 1):], r[:N]])).astype(np.float32)
            li[w, q], lf[w, q], pk[w, q], mg[w, q] = peak_in_slice(m, N, int(lb[w, q, 0]), int(lb[w, q, 1]))
            fm[w, q] = float(m.max())
            if with_bound:
                fb[w, q] = flat_bound(m, N, int(li[w, q]), int(lb[w, q, 0]), int(lb[w, q, 1]))
    return (li, lf, pk, mg, fm, fb) if with_bound else (li, lf, pk, mg, fm)


# -- the two scenarios the weighting exists for (fixed seeds; tests pin the helper and the GPU on them) -----------------
def _delayed(s, d, N, base):
    return s[base - d:base - d + N]


def dc_offset_scene(N=4096, delays=(0, 1100, 2300), seed=1, dc_over_rms=2.0):
    """one white emitter delayed per buoy, plus the SAME DC offset in every buoy (rtl_sdr DC offset / LO leakage at the
    centre frequency: no geometric delay), dc_over_rms times the signal RMS; light noise.  The DC triangle N|c|^2 (1 - |lag| / N)
    outweighs the true peak (N - |lag|) (|c|^2 + sigma^2) once |lag| > N sigma^2 / (|c|^2 + sigma^2) = N / 5 at twice the RMS: the
    delays are chosen so that every pair is past that.  -> (iq [1][B][N], delays)"""
    rng = np.random.default_rng(seed)
    s = ((rng.standard_normal(4 * N) + 1j * rng.standard_normal(4 * N)) / math.sqrt(2)).astype(np.complex64) * 20
    rms = 20.0
    dc = np.complex64(dc_over_rms * rms * np.exp(0.7j))
    out = np.zeros((len(delays), N), np.complex64)
    for b, d in enumerate(delays):
        out[b] = _delayed(s, d, N, 2 * N) + dc
        out[b] += (0.1 * rms * (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / math.sqrt(2)).astype(np.complex64)
    return out[None], np.asarray(delays)


def band_signal(rng, n, f0, f1):
    """complex white noise limited to [f0, f1] cycles per sample (unit RMS), n samples"""
    X = np.fft.fft(rng.standard_normal(n) + 1j * rng.standard_normal(n))
    f = np.fft.fftfreq(n)
    X[(f < f0) | (f > f1)] = 0
    x = np.fft.ifft(X)
    return (x / np.sqrt(np.mean(np.abs(x) ** 2))).astype(np.complex64)


# sub-bands of the two emitters (cycles per sample) and the bands that keep each
STRONG_BAND = (0.05, 0.15)
WEAK_BAND = (-0.30, -0.20)


def two_emitter_scene(N=4096, d_strong=(0, 35, 90, 12), d_weak=(50, 0, 17, 120), seed=2, strong_db=20.0):
    """two band-limited emitters in disjoint sub-bands with their own delays, the strong one strong_db above the weak one;
    light noise.  -> (iq [1][B][N], strong delays, weak delays)"""
    rng = np.random.default_rng(seed)
    a = band_signal(rng, 4 * N, *STRONG_BAND) * np.float32(10 ** (strong_db / 20) * 5)
    b = band_signal(rng, 4 * N, *WEAK_BAND) * np.float32(5)
    out = np.zeros((len(d_strong), N), np.complex64)
    for k, (ds, dw) in enumerate(zip(d_strong, d_weak)):
        out[k] = _delayed(a, ds, N, 2 * N) + _delayed(b, dw, N, 2 * N)
        out[k] += (0.05 * 5 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))).astype(np.complex64)
    return out[None], np.asarray(d_strong), np.asarray(d_weak)


def true_lags(delays):
    B = len(delays)
    return np.array([delays[j] - delays[i] for i in range(B) for j in range(i + 1, B)])
