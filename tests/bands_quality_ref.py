"""Reference of rmx_xcorr_batch_bands_quality (include/rmx.h): slot (w, m, q) is, by definition, slot (w, q) of
rmx_xcorr_batch_quality called with integrate = 1 and band[w][m], so the reference stacks refined_ref.refined_batch (the
coarse weighted_ref.weighted_batch when refine = 0) and quality_ref.quality_batch per band, as bands_ref.py stacks
weighted_ref.py.  It carries the reference's own coarse top-two margin per slot: the condition of the refined entry's
parity rule.  numpy / scipy only."""
import numpy as np

import quality_ref as qr
import refined_ref as rr
import weighted_ref as wr
from bands_ref import per_window


def bands_quality_batch(iq, bands, refine=0, phat=False, lag_bounds=None, pairs=None, quality=True):
    """iq complex64 [W][B][N]; bands [M][2] / [W][M][2]; refine = U in (0, 2, 4, 8, 16); lag_bounds None / [P][2] /
    [W][P][2] (per (window, pair), shared by the window's bands) ->
    (lag_int, lag_frac, peak, margin, full_max, bound), each [W][M][P] -- refined_batch's tuple: margin and full_max are the
    COARSE reference's, bound the flat-peak bound (of the fine taps / U when refined) --, and quality float64 [W][M][P][4]
    (None with quality=False)"""
    b = per_window(bands, iq.shape[0])
    U = int(refine)
    per_band, qual = [], []
    for m in range(b.shape[1]):
        if U:
            per_band.append(rr.refined_batch(iq, U, 1, b[:, m], phat, lag_bounds, pairs))
        else:
            per_band.append(wr.weighted_batch(iq, b[:, m], phat, lag_bounds, pairs, with_bound=True))
        if quality:
            qual.append(qr.quality_batch(iq, 1, b[:, m], phat, lag_bounds, pairs))
    lags = tuple(np.stack([o[k] for o in per_band], axis=1) for k in range(6))
    return lags + ((np.stack(qual, axis=1) if quality else None),)
