"""Reference of rmx_xcorr_batch_bands_integrated (include/rmx.h): slot (g, m, q) is, by definition, slot (g, q) of
rmx_xcorr_batch_quality called with the same integrate, band_per_window = 1 and band[w] = band_cps[w][m], so the reference
stacks refined_ref.refined_batch (the coarse integrated_ref.integrated_batch when refine = 0) and
quality_ref.quality_batch per band, as bands_quality_ref.py does for integrate = 1.  It adds no arithmetic of its own.
numpy / scipy only."""
import numpy as np

import integrated_ref as ir
import quality_ref as qr
import refined_ref as rr
from bands_ref import per_window


def bands_integrated_batch(iq, bands, integrate, refine=0, phat=False, lag_bounds=None, pairs=None, quality=True):
    """iq complex64 [W][B][N]; bands [M][2] / [W][M][2] (per WINDOW: the windows of a group may differ); integrate = K
    dividing W; refine = U in (0, 2, 4, 8, 16); lag_bounds None / [P][2] / [W // K][P][2] (per (group, pair), shared by
    the group's bands) ->
    (lag_int, lag_frac, peak, margin, full_max, bound), each [W // K][M][P] -- refined_batch's tuple: margin and full_max
    are the COARSE integrated reference's, bound the flat-peak bound --, and quality float64 [W // K][M][P][4] (None with
    quality=False)"""
    b = per_window(bands, iq.shape[0])
    K, U = int(integrate), int(refine)
    per_band, qual = [], []
    for m in range(b.shape[1]):
        if U:
            per_band.append(rr.refined_batch(iq, U, K, b[:, m], phat, lag_bounds, pairs))
        else:
            per_band.append(ir.integrated_batch(iq, K, b[:, m], phat, lag_bounds, pairs, with_bound=True))
        if quality:
            qual.append(qr.quality_batch(iq, K, b[:, m], phat, lag_bounds, pairs))
    lags = tuple(np.stack([o[k] for o in per_band], axis=1) for k in range(6))
    return lags + ((np.stack(qual, axis=1) if quality else None),)
