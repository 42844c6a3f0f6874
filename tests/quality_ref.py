"""The restatement of rmx_xcorr_batch_quality (include/rmx.h): the complex64 weighted spectra of tests/weighted_ref.py, the
five sums A, B, C, D, F of every window formed in float64, EE / Et / sum D / sum F / sum C added over a group's windows, and
the coarse peak p0 taken from tests/weighted_ref.py (K = 1) or tests/integrated_ref.py (K > 1), the float32 references of
the existing entries.  A helper of tests/test_quality_cpu.py and tests/test_gpu_quality.py, not part of the oracle."""
import numpy as np

import integrated_ref as ir
import weighted_ref as wr
from refined_ref import signed_bins

COHERENCE, PSR, RMS_BW, NEFF = 0, 1, 2, 3


def window_sums(spec_i, spec_j, n_samples):
    """(A, B, C, D, F) of one window's weighted spectra, float64"""
    L = 2 * n_samples
    ai = np.abs(np.asarray(spec_i, np.complex128))
    aj = np.abs(np.asarray(spec_j, np.complex128))
    t = signed_bins(n_samples) / float(L)
    d = ai * aj
    return float((ai * ai).sum()), float((aj * aj).sum()), float((d * d).sum()), float(d.sum()), float((t * t * d).sum())


def figures(ee, et, sum_c, sum_d, sum_f, p0, n_samples):
    """the four values of one slot from its sums and its coarse peak (the table of include/rmx.h)"""
    L = 2 * n_samples
    p2 = float(p0) ** 2
    coh = min(float(p0) / np.sqrt(ee), 1.0) if ee > 0 else 0.0
    if p0 == 0:
        psr = 0.0
    elif et - p2 <= 0:
        psr = np.inf
    else:
        psr = p2 * (L - 1) / (et - p2)
    bw = np.sqrt(sum_f / sum_d) if sum_d > 0 else 0.0
    neff = sum_d * sum_d / sum_c if sum_c > 0 else 0.0
    return coh, psr, bw, neff


def quality_batch(iq, integrate=1, band=None, phat=False, lag_bounds=None, pairs=None, detail=False):
    """iq complex64 [W][B][N]; integrate = K; band None / [2] / [W][2] (per window); lag_bounds None / [P][2] / [G][P][2]
    (G = W // K) -> quality float64 [G][P][4].  detail: and a dict with p0, EE, Et, each [G][P], and the coarse
    reference's (lag_int, lag_frac)."""
    K = int(integrate)
    W, B, N = iq.shape
    G = W // K
    L = 2 * N
    if pairs is None:
        pairs = [(i, j) for i in range(B) for j in range(i + 1, B)]
    pairs = np.asarray(pairs).reshape(-1, 2)
    P = pairs.shape[0]
    bd = None if band is None else np.broadcast_to(np.asarray(band, np.float64), (W, 2))
    coarse = ir.integrated_batch(iq, K, band, phat, lag_bounds, pairs)
    p0 = coarse[2]
    out = np.zeros((G, P, 4), np.float64)
    det = dict(p0=p0, EE=np.zeros((G, P)), Et=np.zeros((G, P)), lag_int=coarse[0], lag_frac=coarse[1])
    for g in range(G):
        spec = [[wr.weighted_spectrum(iq[w, b], None if bd is None else bd[w], phat) for b in range(B)]
                for w in range(g * K, (g + 1) * K)]
        for q, (i, j) in enumerate(pairs):
            ee = sc = sd = sf = 0.0
            for x in spec:                              # in window order
                a, b, c, d, f = window_sums(x[i], x[j], N)
                ee += (a / L) * (b / L)
                sc += c
                sd += d
                sf += f
            det["EE"][g, q], det["Et"][g, q] = ee, sc / L
            out[g, q] = figures(ee, sc / L, sc, sd, sf, p0[g, q], N)
    return (out, det) if detail else out


def et_over_p2(quality, n_samples):
    """Et / p0^2 = (L - 1) / psr + 1 of quality [...][4]: what psr is compared through (Et - p0^2 cancels on a clean
    signal); inf where psr = 0"""
    psr = np.asarray(quality, np.float64)[..., PSR]
    with np.errstate(divide="ignore"):
        return (2 * n_samples - 1) / psr + 1.0
