"""The sliced reference of rmx_xcorr_batch_bounded (include/rmx.h): S4-S6 of the oracle applied to the slice
m[lo+N-1 .. hi+N-1] of the 'full' magnitude vector.  A helper of tests/test_lag_bounds_cpu.py and
tests/test_gpu_lag_bounds.py, not part of the oracle."""
import numpy as np

from oracle import xcorr_ref as orc


def full_magnitude(x_i, x_j):
    """|correlate(x_j, x_i, 'full', 'fft')| in float32, 2N-1 lags (the oracle's primitive)"""
    return np.abs(orc.xcorr_full_scipy(x_i, x_j)).astype(np.float32)


def peak_in_slice(m, n_samples, lo, hi):
    """(lag_int, lag_frac, peak, margin) of the 'full' magnitude vector m restricted to lags lo..hi: argmax over the
    slice (ties -> lowest), the parabola only strictly inside the slice (0 at its edges), and the relative margin of
    the slice's two largest values (the parity rule's condition)."""
    s = m[lo + n_samples - 1:hi + n_samples]
    k, frac, pk = orc.peak_from_magnitude(s, 1)        # lag relative to the slice start
    if s.shape[0] > 1:
        top = np.partition(s, -2)[-2:]
        margin = float((top[1] - top[0]) / max(top[1], 1e-30))
    else:
        margin = np.inf
    return k + lo, frac, pk, margin


def bounded_batch(iq, lag_bounds, pairs=None):
    """iq complex64 [W][B][N]; lag_bounds [P][2] or [W][P][2] -> (lag_int, lag_frac, peak, margin, full_max), each
    [W][P]; full_max = the largest |c| of the whole 'full' vector (the scale of a float32 FFT's rounding error)"""
    W, B, N = iq.shape
    if pairs is None:
        pairs = [(i, j) for i in range(B) for j in range(i + 1, B)]
    pairs = np.asarray(pairs).reshape(-1, 2)
    lb = np.asarray(lag_bounds)
    if lb.ndim == 2:
        lb = np.broadcast_to(lb, (W,) + lb.shape)
    P = pairs.shape[0]
    li = np.zeros((W, P), np.int64)
    lf = np.zeros((W, P), np.float64)
    pk = np.zeros((W, P), np.float64)
    mg = np.zeros((W, P), np.float64)
    fm = np.zeros((W, P), np.float64)
    for w in range(W):
        for q, (i, j) in enumerate(pairs):
            m = full_magnitude(iq[w, i], iq[w, j])
            li[w, q], lf[w, q], pk[w, q], mg[w, q] = peak_in_slice(m, N, int(lb[w, q, 0]), int(lb[w, q, 1]))
            fm[w, q] = float(m.max())
    return li, lf, pk, mg, fm
