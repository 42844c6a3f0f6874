"""float32 reference of rmx_xcorr_batch_bands (include/rmx.h): slot (w, m, q) is, by definition, slot (w, q) of the weighted
call with band[w][m], so the reference stacks weighted_ref.weighted_batch per band.  numpy / scipy only."""
import numpy as np

import weighted_ref as wr


def per_window(bands, n_windows):
    """bands [M][2] (shared) or [W][M][2] -> float64 [W][M][2]"""
    b = np.asarray(bands, np.float64)
    if b.ndim == 2:
        b = np.broadcast_to(b, (n_windows,) + b.shape)
    assert b.shape[0] == n_windows and b.shape[2] == 2, b.shape
    return b


def bands_batch(iq, bands, phat=False, lag_bounds=None, pairs=None, with_bound=False):
    """iq complex64 [W][B][N]; bands [M][2] / [W][M][2]; lag_bounds None / [P][2] / [W][P][2] (per (window, pair), shared by
    the window's bands) -> weighted_batch's tuple (lag_int, lag_frac, peak, margin, full_max[, flat_bound]), each [W][M][P]"""
    b = per_window(bands, iq.shape[0])
    per_band = [wr.weighted_batch(iq, b[:, m], phat, lag_bounds, pairs, with_bound=with_bound) for m in range(b.shape[1])]
    return tuple(np.stack([o[k] for o in per_band], axis=1) for k in range(len(per_band[0])))
