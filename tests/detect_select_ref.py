"""What d_peaks (radio-mapper_amd/csrc/detect_path.hpp) must report for a given float32 dB spectrum: the peak
selection of rmx_detect_batch restated in plain numpy, with the rules include/rmx.h states where scipy's own are
unspecified (exact ties) or differ in arithmetic (float32 comparisons).  A helper of tests/test_detect_exact.py, not
part of the oracle.

    candidates  local maxima as scipy's _local_maxima_1d: a plateau counts once, at its lower middle bin; nothing at
                bin 0 or N-1
    height      a candidate is kept when its float32 dB >= float32(threshold_db)
    distance    ceil(distance); greedy highest-first removal of every candidate closer than distance bins to a kept
                one; an exact tie in dB ranks the HIGHER bin first; any distance >= N behaves like N
    floor       (lo + hi) * 0.5f of the two middle values of the spectrum (float32)
    snr, conf   snr = p - floor (float32); conf = clamp(snr / 20f, 0, 1) (float32)
    exclusions  a peak is dropped when |signed bin| < dc_exclude_bins or conf < float32(min_confidence)
"""
import bisect
import math

import numpy as np

F32 = np.float32


def local_maxima(p):
    """candidate bins (ascending) of the spectrum p, as scipy.signal._peak_finding_utils._local_maxima_1d"""
    p = np.asarray(p)
    n = p.shape[0]
    if n < 3:
        return np.zeros(0, np.int64)
    # runs of equal values: [s, e] inclusive
    brk = np.flatnonzero(p[1:] != p[:-1]) + 1
    s = np.concatenate(([0], brk))
    e = np.concatenate((brk - 1, [n - 1]))
    ok = (s >= 1) & (e <= n - 2)
    s, e = s[ok], e[ok]
    ok = (p[s - 1] < p[s]) & (p[e + 1] < p[s])
    return ((s[ok] + e[ok]) // 2).astype(np.int64)


def keep_by_distance(bins, heights, distance, n):
    """mask over the candidates (bins ascending) that survive the highest-first distance filter"""
    bins = np.asarray(bins, np.int64)
    heights = np.asarray(heights, np.float32)
    keep = np.ones(bins.shape[0], bool)
    d = math.ceil(distance) if distance < n else n
    if d <= 1 or bins.shape[0] < 2:
        return keep
    order = np.lexsort((bins, heights))[::-1]      # dB descending, on exact ties the higher bin first
    bl = bins.tolist()
    kp = bytearray(b"\x01") * len(bl)
    for i in order.tolist():
        if not kp[i]:
            continue
        lo = bisect.bisect_left(bl, bl[i] - d + 1)
        hi = bisect.bisect_right(bl, bl[i] + d - 1)
        kp[lo:i] = bytes(i - lo)
        kp[i + 1:hi] = bytes(hi - i - 1)
    keep[:] = np.frombuffer(bytes(kp), np.uint8).astype(bool)
    return keep


def noise_floor(p):
    """median of the float32 spectrum as d_peaks forms it: (lo + hi) * 0.5f of the two middle values"""
    q = np.sort(np.asarray(p, np.float32))
    n = q.shape[0]
    lo, hi = q[(n - 1) // 2], q[n // 2]
    return F32(F32(lo + hi) * F32(0.5))


def select_candidates(n, bins, db, floor, threshold_db=-70.0, distance=10, dc_exclude_bins=0.0, min_confidence=0.3):
    """the peaks of a window of n bins whose local maxima are `bins` (ascending) with float32 dB values `db` and whose
    noise floor is `floor`: (bins int64, power_db, snr_db, confidence float32)"""
    bins = np.asarray(bins, np.int64)
    db = np.asarray(db, np.float32)
    floor = F32(floor)
    h = db >= F32(threshold_db)
    bins, db = bins[h], db[h]
    k = keep_by_distance(bins, db, distance, n)
    bins, db = bins[k], db[k]
    sb = np.where(bins < n // 2, bins, bins - n)
    snr = (db - floor).astype(np.float32)
    conf = np.clip(snr / F32(20.0), F32(0.0), F32(1.0)).astype(np.float32)
    ok = ~(np.abs(sb).astype(np.float64) < float(dc_exclude_bins)) & ~(conf < F32(min_confidence))
    return bins[ok], db[ok], snr[ok], conf[ok]


def select(p, threshold_db=-70.0, distance=10, dc_exclude_bins=0.0, min_confidence=0.3):
    """the whole selection on one float32 dB spectrum p: (bins, power_db, snr_db, confidence, noise_floor_db)"""
    p = np.asarray(p, np.float32)
    c = local_maxima(p)
    fl = noise_floor(p)
    return select_candidates(p.shape[0], c, p[c], fl, threshold_db, distance, dc_exclude_bins, min_confidence) + (fl,)
