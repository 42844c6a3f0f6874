"""The reference side of the tests of rmx_caf_batch_quality (include/rmx.h): the Doppler search of tests/caf_request_ref.py
(the winner and the coarse outputs), then tests/quality_ref.py and tests/refined_ref.py on the WINNER's pair of windows
(x_i, rot_mul(x_j, libm_phasor(grid[d*]))) with integrate = 1 and the call's band, weighting, lag bounds and refine.  The
winner is never revisited; the quality figures use the coarse peak.  A helper of tests/test_caf_quality_cpu.py and
tests/test_gpu_caf_quality.py, not part of the oracle."""
import math

import numpy as np

import caf_ref as cr
import caf_request_ref as rq
import quality_ref as qr
import radio_mapper_amd as rm
import refined_ref as rr



def rotated_pairs(iq, grid, dop, pairs=None):
    """The host-rotated pair of every slot: complex64 [W][P][2][N] = (x_i, x_j * rot_d*), the table and the product those
    of the kernels (caf_ref.libm_phasor, caf_ref.rot_mul)"""
    iq = np.asarray(iq, np.complex64)
    W, B, N = iq.shape
    pl = rq.pair_array(pairs, B)
    out = np.zeros((W, len(pl), 2, N), np.complex64)
    tables = {}
    for w in range(W):
        for q, (i, j) in enumerate(pl.tolist()):
            d = int(dop[w, q])
            if d not in tables:
                tables[d] = cr.libm_phasor(grid[d], N)
            out[w, q, 0] = iq[w, i]
            out[w, q, 1] = cr.rot_mul(iq[w, j], tables[d])
    return out


def slot_request(w, q, n_windows, band, lag_bounds):
    """the band [2] and the lag interval [1][2] (or None) that slot (w, q) is correlated under"""
    bd = None if band is None else np.broadcast_to(np.asarray(band, np.float64), (n_windows, 2))[w]
    if lag_bounds is None:
        return bd, None
    lb = np.asarray(lag_bounds)
    return bd, (lb[q:q + 1] if lb.ndim == 2 else lb[w, q:q + 1])


def reference(iq, grid, pairs=None, band=None, phat=False, lag_bounds=None, refine=0):
    """caf_request_ref.reference's dict (its lag_int / lag_frac / peak are the COARSE outputs: those of refine = 0) and
    quality float64 [W][P][4], q_p0 / q_Et [W][P] (what psr is compared through); with refine = U also fine_int,
    fine_frac, fine_peak, fine_bound (the flat-peak bound of the fine taps / U) and full_max, each [W][P]."""
    iq = np.asarray(iq, np.complex64)
    W, B, N = iq.shape
    base = dict(rq.reference(iq, grid, pairs, band, phat, lag_bounds))
    pl = rq.pair_array(pairs, B)
    P = len(pl)
    x = rotated_pairs(iq, grid, base["dop"], pairs)
    qual = np.zeros((W, P, 4))
    p0, et = np.zeros((W, P)), np.zeros((W, P))
    fine = {k: np.zeros((W, P)) for k in ("fine_frac", "fine_peak", "fine_bound", "full_max")}
    fine["fine_int"] = np.zeros((W, P), np.int64)
    for w in range(W):
        for q in range(P):
            bd, lb = slot_request(w, q, W, band, lag_bounds)
            v, det = qr.quality_batch(x[w, q][None], 1, bd, phat, lb, pairs=[(0, 1)], detail=True)
            qual[w, q], p0[w, q], et[w, q] = v[0, 0], det["p0"][0, 0], det["Et"][0, 0]
            if refine:
                li, lf, pk, _, fm, fb = rr.refined_batch(x[w, q][None], refine, 1, bd, phat, lb, pairs=[(0, 1)])
                fine["fine_int"][w, q], fine["fine_frac"][w, q], fine["fine_peak"][w, q] = li[0, 0], lf[0, 0], pk[0, 0]
                fine["fine_bound"][w, q], fine["full_max"][w, q] = fb[0, 0], fm[0, 0]
    base.update(quality=qual, q_p0=p0, q_Et=et)
    if refine:
        base.update(fine)
    return base


# ---- the use case: the DC-offset scene of DESIGN.md section 5.5 with a noise-only buoy -----------------------------------
def dc_noise_scene(N, seed=7):
    """caf_request_ref.dc_scene (three buoys hear one emitter with frequency offsets and share a DC offset) plus a fourth buoy
    that hears noise of the emitter's power and the same DC offset: pairs (0,1), (0,2), (1,2) hold the emitter, pairs
    (0,3), (1,3), (2,3) are noise-only.  -> (iq [1][4][N], grid, emitter pair rows, noise pair rows of the default list)"""
    iq, grid, _, _ = rq.dc_scene(N, seed)
    rng = np.random.default_rng(seed + 1000)
    rms = 20.0
    dc = 2.0 * rms * np.exp(0.7j)
    x = rms * (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / math.sqrt(2) + dc
    iq4 = np.concatenate([iq, x.astype(np.complex64)[None, None]], axis=1)
    pl = rq.pair_array(None, 4).tolist()
    emit = [k for k, (i, j) in enumerate(pl) if j != 3]
    noise = [k for k, (i, j) in enumerate(pl) if j == 3]
    return iq4, grid, emit, noise


# ---- the cases of tests/test_gpu_caf_quality.py -----------------------------------------------------------------------------
# name -> (W, B, N, D, seed) of caf_ref.scene: the smallest shape of each route of tests/test_gpu_caf_request.py's ROUTES.
# tests/test_caf_quality_cpu.py checks the conditions on the inputs of each on the reference alone.
SCENES = {
    "n16": (5, 3, 16, 5, 19), "n256": (3, 4, 256, 5, 256),                       # small windows
    "n8192b4": (2, 4, 8192, 3, 8204), "n8192b6": (2, 6, 8192, 3, 8198),          # four-step: g_rows_inv / g_rows_anchor
    "one3": (3, 3, 4096, 5, 21),                                                 # N = 4096, every hypothesis in one launch
    "chunked12": (12, 3, 4096, 3, 112),                                          # N = 4096 per hypothesis, chunks of 8 + 4
    "seam256": (5, 3, 256, 5, 2560), "seam8192": (5, 3, 8192, 3, 81920),         # chunk seams of the generic paths (gen_chunk = 2)
}
REFINE = 8
_LOADED, _REFERENCES = {}, {}


def scene_of(name):
    """-> (iq, raw uint8, grid, true delays [W][B]), seeded and read-only"""
    if name not in _LOADED:
        W, B, N, D, seed = SCENES[name]
        iq, raw, grid, k = cr.scene(W, B, N, D, seed)
        iq2, delays = rm.synth.make_windows(W, B, N, 2.4e6, seed=seed, snr_db=10.0, doppler_cps=k * (0.5 / N))[:2]
        assert np.array_equal(iq, iq2)
        _LOADED[name] = (iq, raw, grid, np.asarray(delays))
        for a in _LOADED[name]:
            a.setflags(write=False)
    return _LOADED[name]


def case(name, custom):
    """-> (iq, raw, grid, pairs or None, caf() keywords): the default pair list under per-window bounds + per-window bands +
    PHAT, the custom list (a reversed and a repeated pair) under PHAT alone"""
    iq, raw, grid, delays = scene_of(name)
    W, B, N = iq.shape
    pairs = cr.custom_pairs(B) if custom else None
    kw = dict(rq.requests(W, N, rq.true_lags(delays, rq.pair_array(pairs, B))))["phat" if custom else "all"]
    return iq, raw, grid, pairs, kw


def case_reference(name, custom, refine=REFINE):
    """reference() of a case, computed once per process and left unchanged"""
    key = (name, custom, refine)
    if key not in _REFERENCES:
        iq, _, grid, pairs, kw = case(name, custom)
        ref = reference(iq, grid, pairs, refine=refine, **rq.ref_kwargs(kw))
        for a in ref.values():
            a.setflags(write=False)
        _REFERENCES[key] = ref
    return _REFERENCES[key]
