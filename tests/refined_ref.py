"""The restatement of rmx_xcorr_batch_refined (include/rmx.h): the coarse integer lag lag0 of tests/weighted_ref.py /
tests/integrated_ref.py (the float32 references of the existing entries, sliced by tests/lag_bounds_ref.py), then the
band-limited interpolant r(t) = (1/L) sum_s P[s] exp(2 pi i s t / L) of the same weighted spectra at the 2U + 1 lags
lag0 + u / U, the argmax over the admitted u, the parabola on the fine taps and the carry into lag_int.  The products and
sums run in complex128 (the float64 restatement the GPU is compared against) or in complex64 (`single=True`); the phases
are exact rationals either way.  A helper of tests/test_refined_cpu.py and tests/test_gpu_refined.py, not part of the
oracle."""
import numpy as np

import integrated_ref as ir
import weighted_ref as wr
from lag_bounds_ref import peak_in_slice
from oracle import xcorr_ref as orc


def signed_bins(n_samples):
    """s of natural bin k of the L = 2N point transform: 0 .. N-1, -N .. -1"""
    L = 2 * n_samples
    return np.fft.fftfreq(L, 1.0 / L).astype(np.int64)


def fine_r(spec_i, spec_j, n_samples, lag0, U, single=False):
    """r(lag0 + u / U), u = -U .. U, complex [2U + 1], of one window's weighted spectra"""
    L = 2 * n_samples
    s = signed_bins(n_samples)
    u = np.arange(-U, U + 1, dtype=np.int64)
    # turns, reduced in integers: ((s lag0) mod L) / L + ((s u) mod (U L)) / (U L)
    turns = ((s * int(lag0)) % L)[None, :] / float(L) + ((s[None, :] * u[:, None]) % (U * L)) / float(U * L)
    e = np.exp(2j * np.pi * turns)
    if single:
        p = (np.asarray(spec_j, np.complex64) * np.conj(np.asarray(spec_i, np.complex64))).astype(np.complex64)
        return ((e.astype(np.complex64) * p[None, :]).sum(axis=1, dtype=np.complex64) / np.float32(L)).astype(np.complex64)
    p = np.asarray(spec_j, np.complex128) * np.conj(np.asarray(spec_i, np.complex128))
    return (e * p[None, :]).sum(axis=1) / L


def resolve(f, lag0, lo, hi, U):
    """the fine rule on the float32 taps f[2U + 1] -> (lag_int, lag_frac, peak, u*, d, umin, umax)"""
    f = np.asarray(f, np.float32)
    umin = -U if lag0 > lo else 0
    umax = U if lag0 < hi else 0
    best = 0
    for d in range(1, U + 1):                       # equal values: the smallest |u|, then the negative one
        if -d >= umin and f[U - d] > f[U + best]:
            best = -d
        if d <= umax and f[U + d] > f[U + best]:
            best = d
    dd = 0.0
    if best - 1 >= umin and best + 1 <= umax:
        dd = orc.parabolic_offset(f[U + best - 1], f[U + best], f[U + best + 1])
    delta = (best + dd) / U
    n = 1 if delta > 0.5 else (-1 if delta < -0.5 else 0)
    return lag0 + n, float(np.float32(delta - n)), float(f[U + best]), best, dd, umin, umax


def fine_bound(f, U, best, dd, umin, umax):
    """weighted_ref.flat_bound on the fine taps (their index is u + U), divided by U"""
    return wr.flat_bound(np.asarray(f, np.float32), U + 1, best, umin, umax) / U


def refined_batch(iq, refine, integrate=1, band=None, phat=False, lag_bounds=None, pairs=None, single=False, detail=False):
    """iq complex64 [W][B][N]; refine = U in (2, 4, 8, 16); integrate = K; band None / [2] / [W][2] (per window);
    lag_bounds None / [P][2] / [G][P][2] (G = W // K) ->
    (lag_int, lag_frac, peak, margin, full_max, bound), each [G][P]: margin and full_max are the coarse reference's (the
    parity rule's condition and scale), bound the flat-peak bound of the fine taps / U.
    detail: and a dict with lag0 [G][P], the coarse (lag_frac, peak) and the fine taps [G][P][2U + 1]"""
    U, K = int(refine), int(integrate)
    W, B, N = iq.shape
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
    det = dict(lag0=np.zeros((G, P), np.int64), coarse_frac=np.zeros((G, P)), coarse_peak=np.zeros((G, P)),
               taps=np.zeros((G, P, 2 * U + 1), np.float32))
    for g in range(G):
        ws = range(g * K, (g + 1) * K)
        spec = [[wr.weighted_spectrum(iq[w, b], None if bd is None else bd[w], phat) for b in range(B)] for w in ws]
        for q, (i, j) in enumerate(pairs):
            s = np.zeros(2 * N - 1, np.float32)
            for x in spec:
                s = (s + ir.window_power(x[i], x[j], N)).astype(np.float32)
            if K == 1:   # the weighted helper's own vector: |r| of the complex64 inverse
                r = np.asarray(wr.sp_fft.ifft(spec[0][j] * np.conj(spec[0][i])), np.complex64)
                m = np.abs(np.concatenate([r[2 * N - (N - 1):], r[:N]])).astype(np.float32)
            else:
                m = np.sqrt(s).astype(np.float32)
            lo, hi = int(lb[g, q, 0]), int(lb[g, q, 1])
            lag0, cfrac, cpk, mg[g, q] = peak_in_slice(m, N, lo, hi)
            fm[g, q] = float(m.max())
            acc = np.zeros(2 * U + 1, np.float32 if single else np.float64)
            for x in spec:                              # in window order
                r = fine_r(x[i], x[j], N, lag0, U, single)
                p2 = (r.real * r.real + r.imag * r.imag)
                acc = (acc + p2).astype(acc.dtype)
            f = np.sqrt(acc).astype(np.float32)
            li[g, q], lf[g, q], pk[g, q], best, dd, umin, umax = resolve(f, lag0, lo, hi, U)
            fb[g, q] = fine_bound(f, U, best, dd, umin, umax)
            det["lag0"][g, q], det["coarse_frac"][g, q], det["coarse_peak"][g, q], det["taps"][g, q] = lag0, cfrac, cpk, f
    out = (li, lf, pk, mg, fm, fb)
    return out + (det,) if detail else out
