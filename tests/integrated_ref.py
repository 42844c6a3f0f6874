"""The float32 reference of rmx_xcorr_batch_integrated (include/rmx.h): per window the complex64 correlation of
tests/weighted_ref.py (band mask and PHAT where given), |c_w|^2 in float32, the lag-by-lag sum over a group's K windows in
window order in float32, m = sqrt(s), then the sliced peak rule of tests/lag_bounds_ref.py on m.  K = 1 is the weighted
helper itself.  A helper of tests/test_integrated_cpu.py and tests/test_gpu_integrated.py, not part of the oracle."""
import numpy as np
from scipy import fft as sp_fft

import weighted_ref as wr
from lag_bounds_ref import peak_in_slice


def window_power(spec_i, spec_j, n_samples):
    """|c_w|^2 in 'full' order (2N-1 lags, float32) of one window's weighted spectra"""
    N = n_samples
    r = np.asarray(sp_fft.ifft(spec_j * np.conj(spec_i)), np.complex64)
    r = np.concatenate([r[2 * N - (N - 1):], r[:N]])
    re, im = r.real.astype(np.float32), r.imag.astype(np.float32)
    return (re * re + im * im).astype(np.float32)


def integrated_full(iq_group, i, j, band=None, phat=False):
    """m = sqrt(sum_w |c_w|^2) of one group [K][B][N] and one pair, float32 [2N-1]; band None / [2] / [K][2]"""
    K, _, N = iq_group.shape
    bd = None if band is None else np.broadcast_to(np.asarray(band, np.float64), (K, 2))
    s = np.zeros(2 * N - 1, np.float32)
    for w in range(K):
        b = None if bd is None else bd[w]
        s = (s + window_power(wr.weighted_spectrum(iq_group[w, i], b, phat), wr.weighted_spectrum(iq_group[w, j], b, phat),
                              N)).astype(np.float32)
    return np.sqrt(s).astype(np.float32)


def integrated_batch(iq, integrate, band=None, phat=False, lag_bounds=None, pairs=None, with_bound=False):
    """iq complex64 [W][B][N], W a multiple of K = integrate; band None / [2] / [W][2] (per WINDOW); lag_bounds None /
    [P][2] / [G][P][2] (per GROUP, G = W // K) -> (lag_int, lag_frac, peak, margin, full_max), each [G][P], all computed
    on m; with_bound: and flat_bound [G][P] as a sixth (what _assert_parity of tests/test_gpu_weighted.py consumes)"""
    K = int(integrate)
    W, B, N = iq.shape
    if K < 1 or W % K:
        raise ValueError(f"{W} windows are not a multiple of integrate = {K}")
    if K == 1:
        return wr.weighted_batch(iq, band, phat, lag_bounds, pairs, with_bound)
    G = W // K
    if pairs is None:
        pairs = [(i, j) for i in range(B) for j in range(i + 1, B)]
    pairs = np.asarray(pairs).reshape(-1, 2)
    P = pairs.shape[0]
    bd = None if band is None else np.broadcast_to(np.asarray(band, np.float64), (W, 2))
    lb = np.array([[-(N - 1), N - 1]] * P) if lag_bounds is None else np.asarray(lag_bounds)
    if lb.ndim == 2:
        lb = np.broadcast_to(lb, (G,) + lb.shape)
    li = np.zeros((G, P), np.int64)
    lf = np.zeros((G, P), np.float64)
    pk = np.zeros((G, P), np.float64)
    mg = np.zeros((G, P), np.float64)
    fm = np.zeros((G, P), np.float64)
    fb = np.zeros((G, P), np.float64)
    for g in range(G):
        s = np.zeros((P, 2 * N - 1), np.float32)
        for w in range(g * K, (g + 1) * K):
            spec = [wr.weighted_spectrum(iq[w, b], None if bd is None else bd[w], phat) for b in range(B)]
            for q, (i, j) in enumerate(pairs):
                s[q] = s[q] + window_power(spec[i], spec[j], N)
        for q in range(P):
            m = np.sqrt(s[q]).astype(np.float32)
            li[g, q], lf[g, q], pk[g, q], mg[g, q] = peak_in_slice(m, N, int(lb[g, q, 0]), int(lb[g, q, 1]))
            fm[g, q] = float(m.max())
            if with_bound:
                fb[g, q] = wr.flat_bound(m, N, int(li[g, q]), int(lb[g, q, 0]), int(lb[g, q, 1]))
    return (li, lf, pk, mg, fm, fb) if with_bound else (li, lf, pk, mg, fm)


# -- the scenario integration exists for (the generator of the issue's table; tests pin the helper and the GPU on it) -----
def offset_scene(n, seed, snr_db, delays=(0, 9, -14), cycles=(0, 3, 8)):
    """3 buoys, one white emitter delayed per buoy, a frequency offset per receiver of cycles[b] cycles over the n-sample
    capture, unit noise, the emitter snr_db below / above it.  -> complex64 [3][n]; true lag of pair (i, j) = d[j] - d[i]"""
    rng = np.random.default_rng(seed)
    pad = 64
    t = np.arange(n)
    d, cyc = delays, cycles

    def cn(m):
        return (rng.standard_normal(m) + 1j * rng.standard_normal(m)) / np.sqrt(2)
    s = cn(n + 2 * pad)
    return np.stack([(10 ** (snr_db / 20) * s[pad - d[b]: pad - d[b] + n] * np.exp(2j * np.pi * cyc[b] / n * t) + cn(n))
                     for b in range(3)]).astype(np.complex64)


def segments(x, k):
    """[B][n] -> [k][B][n // k]: the capture as k consecutive windows"""
    B, n = x.shape
    return np.ascontiguousarray(x.reshape(B, k, n // k).transpose(1, 0, 2))


TRUE_LAGS = np.array([9, -14, -23])   # delays (0, 9, -14): pairs (0,1), (0,2), (1,2)
