"""The reference side of the tests of rmx_caf_batch_integrated (include/rmx.h): the Doppler search integrated noncoherently
over groups of K consecutive windows.  A float restatement that stacks the helpers of the entries it combines: per
hypothesis tests/integrated_ref.py's integrated_batch on the group's window sequence (x_i, rot_mul(x_j, libm_phasor(nu)))
-- the table of tests/caf_request_ref.py, indexed n = 0 .. N-1 in every window --, caf_ref.first_max and
caf_request_ref.dop_parabola over the hypotheses' INTEGRATED peaks, then tests/quality_ref.py and tests/refined_ref.py
with the same integrate on the winner's rotated sequence.  The margins the GPU bars need -- the winner's top-two lag margin
inside its slice and the hypothesis margin -- are taken on the integrated vectors.  K = 1 is caf_quality_ref.reference.
A helper of tests/test_caf_integrated_cpu.py and tests/test_gpu_caf_integrated.py, not part of the oracle."""
import numpy as np

import caf_quality_ref as cq
import caf_ref as cr
import caf_request_ref as rq
import integrated_ref as ir
import quality_ref as qr
import radio_mapper_amd as rm
import refined_ref as rr


def group_request(g, q, K, n_windows, band, lag_bounds):
    """the bands [K][2] (or None) and the lag interval [1][2] (or None) that slot (g, q) is integrated under"""
    bd = None if band is None else np.broadcast_to(np.asarray(band, np.float64), (n_windows, 2))[g * K:(g + 1) * K]
    if lag_bounds is None:
        return bd, None
    lb = np.asarray(lag_bounds)
    return bd, (lb[q:q + 1] if lb.ndim == 2 else lb[g, q:q + 1])


def rotated_group(iq, g, K, i, j, table):
    """complex64 [K][2][N]: the group's windows of buoy i, and of buoy j under the hypothesis' table (the kernels' product)"""
    ws = slice(g * K, (g + 1) * K)
    return np.ascontiguousarray(np.stack([iq[ws, i], cr.rot_mul(iq[ws, j], table)], axis=1))


def bin_results(iq, grid, integrate, pairs=None, band=None, phat=False, lag_bounds=None):
    """integrated_batch of every hypothesis of every (group, pair): dict of peak float32, lag_int, lag_frac, lag_margin,
    flat_bound, each [G][P][D]"""
    iq = np.asarray(iq, np.complex64)
    K = int(integrate)
    W, B, N = iq.shape
    if K < 1 or W % K:
        raise ValueError(f"{W} windows are not a multiple of integrate = {K}")
    G = W // K
    pl = rq.pair_array(pairs, B)
    grid = np.asarray(grid, np.float64).reshape(-1)
    P, D = len(pl), len(grid)
    tables = [cr.libm_phasor(nu, N) for nu in grid]
    out = dict(peak=np.zeros((G, P, D), np.float32), lag_int=np.zeros((G, P, D), np.int32), lag_frac=np.zeros((G, P, D)),
               lag_margin=np.zeros((G, P, D)), flat_bound=np.zeros((G, P, D)))
    for g in range(G):
        for q, (i, j) in enumerate(pl.tolist()):
            bd, lb = group_request(g, q, K, W, band, lag_bounds)
            for d in range(D):
                x = rotated_group(iq, g, K, i, j, tables[d])
                li, lf, pk, mg, _, fb = ir.integrated_batch(x, K, bd, phat, lb, pairs=[(0, 1)], with_bound=True)
                out["lag_int"][g, q, d], out["lag_frac"][g, q, d], out["lag_margin"][g, q, d] = li[0, 0], lf[0, 0], mg[0, 0]
                out["flat_bound"][g, q, d] = fb[0, 0]
                out["peak"][g, q, d] = np.float32(pk[0, 0])
                assert float(out["peak"][g, q, d]) == pk[0, 0]        # the peaks ARE float32 values
    return out


def reference(iq, grid, integrate, pairs=None, band=None, phat=False, lag_bounds=None, refine=0):
    """Everything a test compares with: dict of dop / dop_frac / lag_int / lag_frac / peak [G][P] (the COARSE outputs),
    bin_peak [G][P][D], hyp_margin, lag_margin, flat_bound, dop_frac_bound, quality float64 [G][P][4], q_p0 / q_Et
    [G][P]; with refine = U also fine_int, fine_frac, fine_peak, fine_bound and full_max, each [G][P]."""
    iq = np.asarray(iq, np.complex64)
    K = int(integrate)
    W, B, N = iq.shape
    r = bin_results(iq, grid, K, pairs, band, phat, lag_bounds)
    pk = r["peak"]
    dop = cr.first_max(pk)
    base = dict(dop=dop, dop_frac=rq.dop_parabola(pk, dop), lag_int=cr.take(r["lag_int"], dop), lag_frac=cr.take(r["lag_frac"], dop),
                peak=cr.take(pk, dop), bin_peak=pk, hyp_margin=cr.hypothesis_margin(pk), lag_margin=cr.take(r["lag_margin"], dop),
                flat_bound=cr.take(r["flat_bound"], dop), dop_frac_bound=rq.dop_frac_bound(pk, dop))
    G, P = dop.shape
    pl = rq.pair_array(pairs, B)
    qual = np.zeros((G, P, 4))
    p0, et = np.zeros((G, P)), np.zeros((G, P))
    fine = {k: np.zeros((G, P)) for k in ("fine_frac", "fine_peak", "fine_bound", "full_max")}
    fine["fine_int"] = np.zeros((G, P), np.int64)
    tables = {}
    for g in range(G):
        for q, (i, j) in enumerate(pl.tolist()):
            d = int(dop[g, q])
            if d not in tables:
                tables[d] = cr.libm_phasor(grid[d], N)
            x = rotated_group(iq, g, K, i, j, tables[d])
            bd, lb = group_request(g, q, K, W, band, lag_bounds)
            v, det = qr.quality_batch(x, K, bd, phat, lb, pairs=[(0, 1)], detail=True)
            qual[g, q], p0[g, q], et[g, q] = v[0, 0], det["p0"][0, 0], det["Et"][0, 0]
            if refine:
                li, lf, fpk, _, fm, fb = rr.refined_batch(x, refine, K, bd, phat, lb, pairs=[(0, 1)])
                fine["fine_int"][g, q], fine["fine_frac"][g, q], fine["fine_peak"][g, q] = li[0, 0], lf[0, 0], fpk[0, 0]
                fine["fine_bound"][g, q], fine["full_max"][g, q] = fb[0, 0], fm[0, 0]
    base.update(quality=qual, q_p0=p0, q_Et=et)
    if refine:
        base.update(fine)
    return base


# ---- what the entry is for: a weak emitter heard by receivers with free-running oscillators --------------------------------
WEAK_DELAYS = (0, 7, -12)
WEAK_STEPS = (0, 2, -3)      # per-receiver offsets in grid steps of 0.5 / N
WEAK_N, WEAK_K, WEAK_D = 256, 16, 13
WEAK_LAGS = np.array([7, -12, -19])       # delays (0, 7, -12): pairs (0,1), (0,2), (1,2)
WEAK_HYPS = np.array([2, -3, -5]) + WEAK_D // 2


def weak_scene(seed, snr_db, N=WEAK_N, K=WEAK_K, D=WEAK_D):
    """3 buoys, one white emitter snr_db against unit noise per receiver, delayed by WEAK_DELAYS and offset by WEAK_STEPS
    grid steps of 0.5 / N cycles per sample, as one capture of K N samples cut into K windows.
    -> (iq complex64 [K][3][N], grid [D] = -(D // 2) .. D // 2 steps)"""
    rng = np.random.default_rng(seed)
    n, pad = N * K, 64
    t = np.arange(n)
    step = 0.5 / N

    def cn(m):
        return (rng.standard_normal(m) + 1j * rng.standard_normal(m)) / np.sqrt(2)
    s = cn(n + 2 * pad)
    x = np.stack([(10 ** (snr_db / 20) * s[pad - WEAK_DELAYS[b]: pad - WEAK_DELAYS[b] + n] * np.exp(2j * np.pi * WEAK_STEPS[b] * step * t)
                   + cn(n)) for b in range(3)]).astype(np.complex64)
    return ir.segments(x, K), (np.arange(D) - D // 2) * step


def weak_counts(seeds, snr_db):
    """Over the seeds' scenes x 3 pairs: how many integer lags are found by (integrate = K alone, the Doppler search on the
    first window alone, the search integrated over the K windows), and how many hypotheses the last one finds"""
    alone = first = both = hyp = 0
    for seed in seeds:
        iq, grid = weak_scene(seed, snr_db)
        alone += int((ir.integrated_batch(iq, WEAK_K)[0][0] == WEAK_LAGS).sum())
        first += int((rq.reference(iq[:1], grid)["lag_int"][0] == WEAK_LAGS).sum())
        r = bin_results(iq, grid, WEAK_K)
        dop = cr.first_max(r["peak"])
        ok = cr.take(r["lag_int"], dop)[0] == WEAK_LAGS
        both += int(ok.sum())
        hyp += int((ok & (dop[0] == WEAK_HYPS)).sum())
    return alone, first, both, hyp


# ---- the cases of tests/test_gpu_caf_integrated.py ----------------------------------------------------------------------------
# name -> (W, B, N, D, K, seed) of caf_ref.scene: the smallest shape that reaches each integrating body on each route.
# tests/test_caf_integrated_cpu.py checks the conditions on the inputs of each on the reference alone.
SCENES = {
    "n16k2": (6, 3, 16, 5, 2, 19), "n16k3": (6, 3, 16, 5, 3, 19),                  # small windows
    "n256k2": (6, 3, 256, 5, 2, 2560), "n256k3": (6, 3, 256, 5, 3, 2560),          # (n256k2: also chunks 2+2+2 under gen_chunk = 2)
    "n8192b4": (4, 4, 8192, 3, 2, 8204), "n8192b6": (4, 6, 8192, 3, 2, 8198),      # four-step: g_rows_inv / g_rows_anchor
    "seam8192": (6, 3, 8192, 3, 2, 81920),                                         # four-step, chunks 2+2+2 under gen_chunk = 2
    "one4": (4, 3, 4096, 3, 2, 21),                                                # N = 4096, every hypothesis in one launch
    # N = 4096 per hypothesis.  The option chunk_windows is a multiple of 8, at least 8: W = 16 under chunks of 8, and K = 3
    # under the same 8, which rounds down to whole groups -- chunks of 6
    "chunk16k2": (16, 3, 4096, 3, 2, 112), "chunk18k3": (18, 3, 4096, 3, 3, 118),
    "group256": (4, 3, 256, 5, 4, 260), "group4096": (4, 3, 4096, 3, 4, 44),       # one group: K = W
}
REFINE = 8
_LOADED, _REFERENCES = {}, {}


def scene_of(name):
    """-> (iq, raw uint8, grid, true delays [W][B]), seeded and read-only"""
    if name not in _LOADED:
        W, B, N, D, _, seed = SCENES[name]
        iq, raw, grid, k = cr.scene(W, B, N, D, seed)
        iq2, delays = rm.synth.make_windows(W, B, N, 2.4e6, seed=seed, snr_db=10.0, doppler_cps=k * (0.5 / N))[:2]
        assert np.array_equal(iq, iq2)
        _LOADED[name] = (iq, raw, grid, np.asarray(delays))
        for a in _LOADED[name]:
            a.setflags(write=False)
    return _LOADED[name]


def case(name, custom):
    """-> (iq, raw, grid, K, pairs or None, caf() keywords): the default pair list under per-group bounds + per-window
    bands + PHAT, the custom list (a reversed and a repeated pair) under PHAT alone"""
    iq, raw, grid, delays = scene_of(name)
    W, B, N = iq.shape
    K = SCENES[name][4]
    pairs = cr.custom_pairs(B) if custom else None
    if custom:
        return iq, raw, grid, K, pairs, dict(whiten=True)
    lags = rq.true_lags(delays, rq.pair_array(pairs, B)).reshape(W // K, K, -1)
    half = max(2, min(8, N // 8))
    r = np.rint(lags).astype(np.int64)
    nm1 = N - 1
    lb = np.stack([np.clip(r.min(1) - half, -nm1, nm1), np.clip(r.max(1) + half, -nm1, nm1)], -1).astype(np.int32)   # [G][P][2]
    return iq, raw, grid, K, pairs, dict(lag_bounds=lb, band=rq.window_bands(W), whiten=True)


def case_reference(name, custom, refine=REFINE):
    """reference() of a case, computed once per process and left unchanged"""
    key = (name, custom, refine)
    if key not in _REFERENCES:
        iq, _, grid, K, pairs, kw = case(name, custom)
        ref = reference(iq, grid, K, pairs, refine=refine, **rq.ref_kwargs(kw))
        for a in ref.values():
            a.setflags(write=False)
        _REFERENCES[key] = ref
    return _REFERENCES[key]


__all__ = ["reference", "bin_results", "case", "case_reference", "weak_scene", "weak_counts", "SCENES", "cq"]
