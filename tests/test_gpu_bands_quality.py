"""rmx_xcorr_batch_bands_quality on the GPU: the fine lag search and the quality figures of several bands per window over
one set of forward spectra -- against the reference (tests/bands_quality_ref.py) at the bars of the refined and the quality
entries on every layout and seam, bit for bit against the single-band quality call band by band, the identities, the launch
counts, single-bin bands on either side of a 16-byte load, device pointers, the refusals in their order and the seam with
share_qualified."""
import ctypes as C
import math

import numpy as np
import pytest

import bands_quality_ref as bq
import bands_ref as br
import quality_ref as qr
import radio_mapper_amd as rm
import weighted_ref as wr

pytestmark = pytest.mark.gpu
TOL = 1e-5      # the refined entry's bar (include/rmx.h)
QTOL = 1e-4     # the quality entry's


@pytest.fixture(scope="module")
def xc():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    if xcorr.device_count() < 1:
        pytest.fail("no GPU visible")
    return xcorr


@pytest.fixture
def opts(xc):
    xc.clear_default_options()
    yield xc.set_default_option
    xc.clear_default_options()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def _assert_refined(got, ref, N, lb, what):
    """the parity rule of rmx_xcorr_batch_refined on [W][M][P] arrays.  The reference's coarse top-two margin must exceed
    1e-5 on EVERY slot -- asserted first: the seeds below were chosen so that it leaves out none."""
    li, lf, pk = got[:3]
    ri, rf, rp, mg, fm, fb = ref[:6]
    assert np.all(mg > TOL), (what, "slots left out", int((mg <= TOL).sum()), float(mg.min()))
    assert np.all(np.isfinite(lf)) and np.all(np.isfinite(pk))
    lag, want = li + lf.astype(np.float64), ri + rf
    rel = np.abs(lag - want) / np.maximum(np.abs(want), 1.0)
    worst = int(np.argmax(rel))
    print("%s: worst |dlag| / max(|lag|, 1) = %.3e (flat-peak bound there %.3e), worst peak deviation %.3e relative"
          % (what, rel.max(), fb.ravel()[worst], float(np.max(np.abs(pk - rp) / np.maximum(rp, 1e-30) * (rp > 0)))))
    assert np.all((rel <= TOL) | (rel <= fb)), (what, float(rel.max()), float(fb.ravel()[worst]))
    assert np.all(np.abs(pk - rp) <= 1e-5 * rp + 1e-6 * fm), what
    if lb is not None:
        b = np.asarray(lb)
        b = b[:, None] if b.ndim == 3 else b[None, None]           # [W][1][P][2] / [1][1][P][2]: shared by the bands
        assert np.all(li >= b[..., 0]) and np.all(li <= b[..., 1]), what
    assert np.all(np.abs(li) <= N - 1) and np.all(np.abs(lf) <= 0.5), what


def _assert_quality(got, ref, N, what):
    """the parity rule of rmx_xcorr_batch_quality: coherence, rms_bw, n_eff within 1e-4 relative, psr through Et / p0^2"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got[..., [qr.COHERENCE, qr.RMS_BW, qr.NEFF]])) and not np.any(np.isnan(got)), what
    dev = {}
    for name, k in (("coherence", qr.COHERENCE), ("rms_bw", qr.RMS_BW), ("n_eff", qr.NEFF)):
        zero = ref[..., k] == 0
        assert np.all(got[..., k][zero] == 0), (what, name)
        dev[name] = float(np.max(np.abs(got[..., k] - ref[..., k])[~zero] / ref[..., k][~zero], initial=0.0))
    zero = ref[..., qr.PSR] == 0
    assert np.all(got[..., qr.PSR][zero] == 0), (what, "psr")
    ge, re_ = qr.et_over_p2(got[~zero], N), qr.et_over_p2(ref[~zero], N)
    dev["Et/p0^2"] = float(np.max(np.abs(ge - re_) / re_, initial=0.0))
    print("%s: worst relative deviation %s" % (what, ", ".join("%s %.2e" % kv for kv in dev.items())))
    for name, d in dev.items():
        assert d <= QTOL, (what, name, d)
    assert np.all(got[..., qr.COHERENCE] >= 0) and np.all(got[..., qr.COHERENCE] <= 1), what


def _random_bands(rng, shape, N):
    """uniformly random [lo, hi] bands at least 2 bins of the 2N-point transform wide"""
    a = rng.uniform(-0.5, 0.5, size=shape + (2,))
    lo, hi = a.min(-1), a.max(-1)
    lo = np.minimum(lo, 0.5 - 2.0 / (2 * N))
    return np.stack([lo, np.maximum(hi, lo + 2.0 / (2 * N))], -1)


MIN_WIDTH = 0.35   # cycles per sample, of the bands that are held to the refined entry's bar


def _wide_bands(rng, shape, N):
    """random [lo, hi] bands at least MIN_WIDTH wide.  The refined entry's bar is 1e-5 * max(|lag|, 1) on the lag, and a
    fine tap is a float32 sum of L terms: a few ulp, e = 2e-7 relative.  Around its peak |r(t)| = f0 (1 - (2 pi b t)^2 / 2)
    with b the rms bandwidth, so the parabola through three taps 1 / U apart turns a tap error e into a lag error of
    e U / (2 pi b)^2: at U = 16 the bar needs b >= 0.09, and a flat band of width w has b = w / sqrt(12): w >= 0.31.
    Narrower bands cannot meet that bar in float32 whatever the kernel (include/rmx.h: a narrow band is noise-limited and
    refinement gains nothing there); they are held to the single-band call bit for bit and to the quality bar in
    test_narrow_bands_against_the_single_band_call."""
    lo = rng.uniform(-0.5, 0.5 - MIN_WIDTH, size=shape)
    return np.stack([lo, lo + rng.uniform(MIN_WIDTH, 0.5 - lo)], -1)


def _bounds_around(rng, shape, N, true):
    """lag intervals [..][2] that hold the pair's true lag, now and then with the true lag on an edge (the fine grid is then
    one-sided)"""
    t = np.broadcast_to(np.rint(true).astype(np.int64), shape)
    reach = rng.integers(0, max(N // 2, 2), size=shape + (2,)) * rng.integers(0, 4, size=shape + (2,)).clip(0, 1)
    return np.stack([np.maximum(t - reach[..., 0], -(N - 1)), np.minimum(t + reach[..., 1], N - 1)], -1).astype(np.int32)


def _true_lags(delays, pairs, B):
    pairs = pairs or [(i, j) for i in range(B) for j in range(i + 1, B)]
    return np.stack([delays[:, j] - delays[:, i] for i, j in pairs], -1)       # [W][P]


# a cut of tests/test_gpu_bands.py's route table: every layout of the stored spectra (RefLayout, refine.hpp), every seam
# (route name, N, buoys, windows, bands, default options, engine options, forward families, pair family, chunks)
CUSTOM = [(1, 0), (0, 2), (2, 2), (0, 1)]   # a reversed pair and a self pair
ROUTES = [
    ("kRefKfwd", 4096, 3, 2, 3, {}, {}, ("k_fwd",), "k_win|k_pair", 1),
    # (the library rounds chunk_windows up to a multiple of 8 and caps it at the engine's windows: 5 windows are ONE chunk)
    ("kRefKfwd chunk_windows 2", 4096, 3, 5, 3, {}, {"chunk_windows": 2}, ("k_fwd",), "k_win|k_pair", 1),
    ("kRefKfwd chunk seam", 4096, 3, 11, 3, {}, {"chunk_windows": 8}, ("k_fwd",), "k_win|k_pair", 2),
    ("kRefKfwd k_pair_str", 4096, 4, 3, 2, {}, {"resident": 0}, ("k_fwd",), "k_win|k_pair", 1),
    ("kRefSmall N=16 gen_chunk 2", 16, 3, 5, 3, {"gen_chunk": 2}, {}, ("g_fwd_small",), "g_pair_small", 3),
    ("kRefSmall N=16 64 bands", 16, 3, 2, 64, {}, {}, ("g_fwd_small",), "g_pair_small", 1),
    ("kRefSmall N=256", 256, 4, 5, 3, {}, {}, ("g_fwd_small",), "g_pair_small", 1),
    ("kRefRows N=256 gen_chunk 2", 256, 3, 5, 3, {"small_maxl": 256, "gen_chunk": 2}, {}, ("g_cols_fwd", "g_rows_fwd"), "g_rows_inv", 3),
    ("kRefRows N=8192 3 buoys", 8192, 3, 2, 2, {}, {}, ("g_cols_fwd", "g_rows_fwd"), "g_rows_inv", 1),
    ("kRefRows N=8192 8 buoys", 8192, 8, 1, 2, {}, {}, ("g_cols_fwd", "g_rows_fwd"), "g_rows_inv", 1),
    ("kRefRows N=8192 8 buoys rows_anchor 0", 8192, 8, 1, 2, {"rows_anchor": 0}, {}, ("g_cols_fwd", "g_rows_fwd"), "g_rows_inv", 1),
]
ALL_U = ("kRefKfwd", "kRefSmall N=16 gen_chunk 2", "kRefRows N=256 gen_chunk 2")   # all four U on one route per layout
# the case generator's seed per route: the smallest for which the reference's own coarse top-two margin exceeds 1e-5 on
# every slot of every case (found on the CPU with the reference alone)
SEEDS = {"kRefKfwd": 1, "kRefKfwd chunk_windows 2": 1, "kRefKfwd chunk seam": 1, "kRefKfwd k_pair_str": 1, "kRefSmall N=16 gen_chunk 2": 1,
         "kRefSmall N=16 64 bands": 1, "kRefSmall N=256": 1, "kRefRows N=256 gen_chunk 2": 1, "kRefRows N=8192 3 buoys": 1,
         "kRefRows N=8192 8 buoys": 1, "kRefRows N=8192 8 buoys rows_anchor 0": 1}
FORBIDDEN = ("g_win_*", "g_rows_fused", "g_rows_anchor", "k16_fwd", "k16_pairs")


def _inputs(route):
    name, N, B, W = route[:4]
    return rm.synth.make_windows(W, B, N, 10e6, seed=len(name), snr_db=10, bandwidth=0.8, max_delay=min(40, N / 8), return_u8=True)


def _cases(route):
    """the calls of one route, (bands, PHAT, lag bounds, pair list, U): shared and per-window bands, NONE and PHAT, no /
    per-window / shared bounds, the default and a custom pair list, U = 2 and 16 -- and 4 and 8 on one route per layout"""
    name, N, B, W, M = route[:5]
    rng = np.random.default_rng(SEEDS[name])
    delays = _inputs(route)[1]
    shared = _wide_bands(rng, (M,), N)
    per_win = _wide_bands(rng, (W, M), N)
    P = B * (B - 1) // 2
    lb = _bounds_around(rng, (W, P), N, _true_lags(delays, None, B))
    lb_custom = _bounds_around(rng, (len(CUSTOM),), N, _true_lags(delays, CUSTOM, B)[0])
    lb_custom[..., 0] = np.minimum(lb_custom[..., 0], -min(42, N - 1))     # shared by the windows: holds every window's lag
    lb_custom[..., 1] = np.maximum(lb_custom[..., 1], min(42, N - 1))
    cases = [(shared, False, None, None, 2), (per_win, True, lb, None, 16), (per_win, False, lb_custom, CUSTOM, 16),
             (shared, True, None, CUSTOM, 2)]
    if name in ALL_U:
        cases += [(per_win, False, lb, None, 4), (shared, True, lb_custom, CUSTOM, 8)]
    return cases


def _direct(xc, eng, iq, bands, refine=0, quality=None, whiten=False, lag_bounds=None, outs=None):
    """rmx_xcorr_batch_bands_quality itself with host pointers and the default pair list -> (rc, text, outs)"""
    lib = xc.load_library()
    W, B = iq.shape[0], iq.shape[1]
    P = B * (B - 1) // 2
    bd = np.ascontiguousarray(bands, np.float64)
    M, pw = bd.shape[-2], int(bd.ndim == 3)
    lb = None if lag_bounds is None else np.ascontiguousarray(lag_bounds, np.int32)
    if outs is None:
        outs = [np.zeros((W, M, P), t) for t in (np.int32, np.float32, np.float32)]
    vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib.rmx_xcorr_batch_bands_quality(eng._ctx, vp(iq), W, None, P, vp(bd), M, pw, 1 if whiten else 0, vp(lb),
                                           0 if lb is None else int(lb.ndim == 3), refine, *[vp(o) for o in outs], vp(quality), 0)
    return rc, lib.rmx_last_error(eng._ctx).decode(), outs


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_against_the_reference_and_the_single_band_call(xc, opts, route):
    """Per route and case: parity with bands_quality_ref at the refined and the quality bars, no slot left out; [:, m] of
    all four arrays bit for bit correlate(band=bands[:, m], refine=U, quality=True) on an engine with the same options;
    quality leaves the three lag outputs alone; uint8 input and a repeated call bit-identical; ONE forward pass, one
    k_quality and one k_refine launch per chunk and none of the kernels that keep their spectra to themselves.
    One route is not held to the single-band call in full: four-step with the default pair list from 6 buoys on, where the
    weighted call's inverse rows are g_rows_anchor and its COARSE peak may differ from the banded call's in a last bit
    (tests/test_gpu_bands.py).  There coherence and psr, which are computed from the coarse peak, are held to the reference;
    rms_bw and n_eff, which depend on the spectra alone, are bit-identical, and so is the refined triple wherever the
    coarse lag agrees.  Found on the MI355X at N = 8192 with 8 buoys: the coarse lag agreed on all 28 slots of every band
    and case, and coherence / psr were bit-identical on 27 or 28 of the 28 (one coarse peak differs in its last bit)."""
    name, N, B, W, M, dopt, eopt, fwd, pair_family, chunks = route
    for k, v in dopt.items():
        opts(k, v)
    iq, _, raw = _inputs(route)
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        eng.set_option("timing", 1)
        for n_case, (bands, phat, bounds, pairs, U) in enumerate(_cases(route)):
            what = "%s case %d U=%d" % (name, n_case, U)
            got = eng.correlate_bands(iq, bands, pairs, lag_bounds=bounds, whiten=phat, refine=U, quality=True)
            tk = eng.last_timing_by_kernel()
            P = len(pairs) if pairs else B * (B - 1) // 2
            assert len(got) == 4 and got[0].shape == (W, M, P) and got[3].shape == (W, M, P, 4) and got[3].dtype == np.float32
            ref = bq.bands_quality_batch(iq, bands, U, phat, bounds, pairs)
            _assert_refined(got, ref, N, bounds, what)
            _assert_quality(got[3], ref[6], N, what)
            pw = br.per_window(bands, W)
            anchor = len(fwd) == 2 and B >= 6 and pairs is None and dopt.get("rows_anchor", 1) != 0
            for m in range(M):
                one = eng.correlate(iq, pairs, lag_bounds=bounds, band=pw[:, m], whiten=phat, refine=U, quality=True)
                tk1 = eng.last_timing_by_kernel()
                assert anchor == ("g_rows_anchor" in tk1), tk1
                if not anchor:
                    assert _same([g[:, m] for g in got], one), "%s: band %d differs from the single-band call" % (what, m)
                    continue
                assert np.array_equal(got[3][:, m][..., 2:], one[3][..., 2:]), "%s: rms_bw / n_eff of band %d" % (what, m)
                lag0 = eng.correlate_bands(iq, bands, pairs, lag_bounds=bounds, whiten=phat)[0][:, m]
                agree = lag0 == eng.correlate(iq, pairs, lag_bounds=bounds, band=pw[:, m], whiten=phat)[0]
                assert agree.mean() >= 0.9, (what, m, float(agree.mean()))
                assert all(np.array_equal(g[:, m][agree], o[agree]) for g, o in zip(got[:3], one[:3])), (what, m)
                print("%s band %d: coarse lag agrees on %d of %d slots; coherence / psr bit-identical on %d" %
                      (what, m, int(agree.sum()), agree.size, int(np.all(got[3][:, m][..., :2] == one[3][..., :2], axis=-1).sum())))
            four = {"g_cols_inv", "g_final"} if len(fwd) == 2 else set()
            assert set(tk) == set(fwd) | {pair_family, "k_refine", "k_quality"} | four, tk
            assert not set(tk) & set(FORBIDDEN)
            for f in fwd:
                assert tk[f]["launches"] == tk1[f]["launches"], (f, tk, tk1)
            assert tk["k_refine"]["launches"] == chunks and tk["k_quality"]["launches"] == chunks, tk
            no_q = eng.correlate_bands(iq, bands, pairs, lag_bounds=bounds, whiten=phat, refine=U)
            assert len(no_q) == 3 and _same(no_q, got[:3]), what + ": quality changed a lag output"
            assert "k_quality" not in eng.last_timing_by_kernel()
            assert _same(got, eng.correlate_bands(raw, bands, pairs, lag_bounds=bounds, whiten=phat, refine=U, quality=True)), "uint8 input"
            assert _same(got, eng.correlate_bands(iq, bands, pairs, lag_bounds=bounds, whiten=phat, refine=U, quality=True)), "twice"


@pytest.mark.parametrize("route", [ROUTES[0], ROUTES[4], ROUTES[6], ROUTES[7], ROUTES[8]], ids=lambda r: r[0])
def test_narrow_bands_against_the_single_band_call(xc, opts, route):
    """Random bands down to two bins wide, where the refined bar cannot hold in float32 (_wide_bands): all four arrays bit
    for bit the single-band call's, every U, and the quality figures at their bar."""
    name, N, B, W, M, dopt, eopt = route[:7]
    for k, v in dopt.items():
        opts(k, v)
    iq, delays, _ = _inputs(route)
    rng = np.random.default_rng(N + M)
    lb = _bounds_around(rng, (W, B * (B - 1) // 2), N, _true_lags(delays, None, B))
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        for U, phat, bounds in ((2, False, None), (4, True, lb), (8, False, lb), (16, True, None)):
            bands = _random_bands(rng, (W, M), N)
            got = eng.correlate_bands(iq, bands, lag_bounds=bounds, whiten=phat, refine=U, quality=True)
            for m in range(M):
                one = eng.correlate(iq, lag_bounds=bounds, band=bands[:, m], whiten=phat, refine=U, quality=True)
                assert _same([g[:, m] for g in got], one), (name, U, phat, m)
            _assert_quality(got[3], bq.bands_quality_batch(iq, bands, 0, phat, bounds)[6], N, "%s narrow U=%d" % (name, U))


@pytest.mark.parametrize("route", [ROUTES[0], ROUTES[2], ROUTES[4], ROUTES[7], ROUTES[8]], ids=lambda r: r[0])
def test_the_identities(xc, opts, route):
    """refine == 0 and quality == NULL is rmx_xcorr_batch_bands: the same launches, the same bits.  n_bands == 1 is
    rmx_xcorr_batch_quality with integrate = 1.  Quality alone (refine = 0) leaves the banded call's lags alone and meets
    the quality bar."""
    name, N, B, W, M, dopt, eopt, fwd, pair_family, chunks = route
    for k, v in dopt.items():
        opts(k, v)
    iq, delays, _ = _inputs(route)
    rng = np.random.default_rng(N + W)
    bands = _random_bands(rng, (W, M), N)
    lb = _bounds_around(rng, (W, B * (B - 1) // 2), N, _true_lags(delays, None, B))
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        eng.set_option("timing", 1)
        for phat, bounds in ((False, None), (True, lb)):
            old = eng.correlate_bands(iq, bands, lag_bounds=bounds, whiten=phat)              # rmx_xcorr_batch_bands
            t_old = eng.last_timing_by_kernel()
            rc, text, new = _direct(xc, eng, iq, bands, 0, None, phat, bounds)
            assert rc == 0, text
            assert _same(old, new)
            assert {k: v["launches"] for k, v in t_old.items()} == {k: v["launches"] for k, v in eng.last_timing_by_kernel().items()}
            q_only = eng.correlate_bands(iq, bands, lag_bounds=bounds, whiten=phat, quality=True)
            t_q = eng.last_timing_by_kernel()
            assert _same(old, q_only[:3]) and "k_refine" not in t_q and t_q["k_quality"]["launches"] == chunks
            for f in fwd:                                                                    # no second forward pass
                assert t_q[f]["launches"] == t_old[f]["launches"]
            _assert_quality(q_only[3], bq.bands_quality_batch(iq, bands, 0, phat, bounds)[6], N, name + " quality alone")
            a = eng.correlate_bands(iq, bands[:, :1], lag_bounds=bounds, whiten=phat, refine=8, quality=True)
            ta = eng.last_timing_by_kernel()
            b = eng.correlate(iq, lag_bounds=bounds, band=bands[:, 0], whiten=phat, refine=8, quality=True)
            assert _same([x[:, 0] for x in a], b)
            assert {k: v["launches"] for k, v in ta.items()} == {k: v["launches"] for k, v in eng.last_timing_by_kernel().items()}


# one kept bin on either side of a 16-byte load: two stored complex positions 2 f, 2 f + 1 hold the natural bins k and
# k + 512 where k_fwd stored the spectrum (bit 9 of k clear), k and k + N in the two generic layouts (k < N)
SINGLE = [("kRefKfwd", 4096, {}, 512), ("kRefSmall", 256, {}, 256), ("kRefRows N=256", 256, {"small_maxl": 256}, 256),
          ("kRefRows N=8192", 8192, {}, 8192)]


@pytest.mark.parametrize("route", SINGLE, ids=[r[0] for r in SINGLE])
def test_single_bin_bands_on_either_side_of_a_load(xc, opts, route):
    """Three one-bin bands of ONE window: the lower bin of a load, the upper bin of the same load (the other one dropped
    each time) and a bin of another load (neither of the first load's kept: it is skipped).  The lag interval is one lag
    wide, so the coarse call has a defined peak; a one-bin correlation has the same magnitude at every lag and every fine
    tap: peak = |X_j[s]| |X_i[s]| / L, coherence = 1, psr = 1, rms_bw = |s| / L, n_eff = 1.  Against the reference at its
    bars, against the closed forms, and bit for bit against the single-band call."""
    name, N, dopt, step = route
    for k, v in dopt.items():
        opts(k, v)
    L = 2 * N
    iq, _ = rm.synth.make_windows(1, 2, N, 10e6, seed=5)
    X = [np.fft.fft(iq[0, b].astype(np.complex128), L) for b in range(2)]
    strength = np.abs(X[0]) * np.abs(X[1])
    low = [k for k in range(1, N) if not k & step and k + step < L]
    k_lo = max(low, key=lambda k: min(strength[k], strength[k + step]))        # both bins of the load well above the rounding
    k_other = max((k for k in range(1, N) if k not in (k_lo, k_lo + step, k_lo ^ 1)), key=lambda k: strength[k] * (k % 7 == 3))
    bins = [k if k < N else k - L for k in (k_lo, k_lo + step, k_other)]
    bands = np.array([[s / L, s / L] for s in bins])
    with xc.XcorrEngine(2, N, 1) as eng:
        for lag in (0, -37 % N, N - 1, -(N - 1)):
            lb = np.array([[lag, lag]], np.int32)
            for U in (2, 16):
                li, lf, pk, ql = eng.correlate_bands(iq, bands, lag_bounds=lb, refine=U, quality=True)
                what = "%s bins %s lag %d U=%d" % (name, bins, lag, U)
                want = np.array([strength[s % L] / L for s in bins])
                print(what, pk[0, :, 0], want, ql[0, :, 0])
                assert np.all(li == lag) and np.all(lf == 0)
                ref = bq.bands_quality_batch(iq, bands, U, False, lb)
                _assert_refined((li, lf, pk), ref, N, lb, what)
                _assert_quality(ql, ref[6], N, what)
                assert np.allclose(pk[0, :, 0], want, rtol=1e-4, atol=0), what
                assert np.allclose(ql[0, :, 0, qr.NEFF], 1.0, rtol=QTOL) and np.allclose(ql[0, :, 0, qr.COHERENCE], 1.0, rtol=QTOL)
                assert np.allclose(ql[0, :, 0, qr.RMS_BW], np.abs(bins) / L, rtol=QTOL)
                assert np.allclose(qr.et_over_p2(ql[0, :, 0], N), L, rtol=QTOL)
                for m in range(3):
                    one = eng.correlate(iq, lag_bounds=lb, band=bands[m], refine=U, quality=True)
                    assert _same([li[:, m], lf[:, m], pk[:, m], ql[:, m]], one), (what, m)
        # a wider interval: whichever lag the flat coarse vector yields, every fine tap has the same magnitude
        li, lf, pk, ql = eng.correlate_bands(iq, bands, lag_bounds=np.array([[-5, 9]], np.int32), refine=8, quality=True)
        assert np.allclose(pk[0, :, 0], want, rtol=1e-4, atol=0) and np.all(li + lf >= -5) and np.all(li + lf <= 9)
        assert np.allclose(ql[0, :, 0, qr.NEFF], 1.0, rtol=QTOL)


@pytest.mark.parametrize("route", [ROUTES[0], ROUTES[3], ROUTES[6], ROUTES[8]], ids=lambda r: r[0])
def test_device_pointers_and_reuse_of_the_callers_arrays(xc, opts, route):
    torch = pytest.importorskip("torch")
    name, N, B, W, M, dopt, eopt = route[:7]
    for k, v in dopt.items():
        opts(k, v)
    iq, delays, raw = _inputs(route)
    P = B * (B - 1) // 2
    rng = np.random.default_rng(7)
    bands, lb = _random_bands(rng, (W, M), N), _bounds_around(rng, (W, P), N, _true_lags(delays, None, B))
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        host = eng.correlate_bands(iq, bands, lag_bounds=lb, whiten=True, refine=4, quality=True)
        for x, u8 in ((iq.view(np.float32), False), (raw, True)):
            d_iq = torch.from_numpy(x).cuda()
            outs = [torch.full((W, M, P), -7, dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.float32)]
            d_q = torch.full((W, M, P, 4), -7, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            mine, mine_lb = bands.copy(), lb.copy()
            eng.correlate_bands_device(d_iq.data_ptr(), W, mine, *[o.data_ptr() for o in outs], u8=u8, lag_bounds=mine_lb,
                                       whiten=True, refine=4, quality_ptr=d_q.data_ptr())
            mine[:] = (0.0, 0.0)                             # the caller may reuse its arrays at once
            mine_lb[:] = 0
            eng.synchronize()
            assert _same(host, [o.cpu().numpy() for o in outs] + [d_q.cpu().numpy()])


def test_refusals_in_their_order_leave_the_outputs_untouched(xc):
    N, W, M, P = 256, 4, 3, 3
    iq, _ = rm.synth.make_windows(W, 3, N, 10e6, seed=1)
    lib = xc.load_library()
    good = np.tile([[-0.5, 0.5], [0.0, 0.25], [-0.1, 0.1]], (W, 1, 1))
    with xc.XcorrEngine(3, N, W) as eng:
        block = np.full(8 * W * M * P, 77, np.float32)      # quality, and room to overlap the others with
        out = [np.full((W, M, P), 77, t) for t in (np.int32, np.float32, np.float32)]
        ql = block[:4 * W * M * P].reshape(W, M, P, 4)
        vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731

        def call(bands, n_bands=M, per_window=1, bounds=None, bounds_pw=0, weighting=0, iq_p=iq, refine=4, quality=ql, outs=out,
                 n_windows=W, pairs=None, n_pairs=P):
            b = None if bands is None else np.ascontiguousarray(bands, np.float64)
            lb = None if bounds is None else np.ascontiguousarray(bounds, np.int32)
            rc = lib.rmx_xcorr_batch_bands_quality(eng._ctx, vp(iq_p), n_windows, vp(pairs), n_pairs, vp(b), n_bands, per_window,
                                                   weighting, vp(lb), bounds_pw, refine, *[vp(o) for o in outs], vp(quality), 0)
            return rc, lib.rmx_last_error(eng._ctx).decode()
        assert call(good)[0] == 0 and not np.any(out[0] == 77) and not np.any(ql == 77)
        for o in out + [block]:
            o[:] = 77
        # rmx_xcorr_batch_bands' own refusals, in its order, each in front of a bad refine and an overlapping quality
        over = out[2].reshape(-1)[:1]
        for more in ({}, {"refine": 3}, {"refine": 3, "quality": over}):
            assert call(None, **more) == (-1, "NULL buffer") and call(good, iq_p=None, **more) == (-1, "NULL buffer")
            assert call(None, n_bands=0, **more)[1] == "NULL buffer"
            for n_bands in (0, 65, -1):
                rc, text = call(good, n_bands=n_bands, **more)
                assert rc == -1 and "n_bands" in text
            rc, text = call(good, weighting=2, **more)
            assert rc == -1 and "weighting" in text
            assert "n_bands" in call(good, n_bands=0, weighting=2, **more)[1]
            for bad in ([0.5, 0.5], [np.nan, 0.1], [0.2, 0.1], [-0.6, 0.1], [1e-9, 2e-9]):
                bands = good.copy()
                bands[2, 1] = bad
                rc, text = call(bands, **more)
                assert rc == -1 and "band 1 of window 2" in text, text
                rc, text = call(bands[2], per_window=0, **more)
                assert rc == -1 and "band 1 of window 0" in text and "shared" in text, text
            rc, text = call(good, n_pairs=2, **more)                       # the batch shape
            assert rc == -1 and "pairs == NULL needs" in text, text
            rc, text = call(good, n_windows=W + 1, **more)
            assert rc == -1 and "n_windows" in text, text
            for lo, hi in ((-N, 0), (0, N), (5, 4)):
                lb = np.tile(np.array([[-3, 3]], np.int32), (W, P, 1))
                lb[1, 2] = (lo, hi)
                rc, text = call(good, bounds=lb, bounds_pw=1, **more)
                assert rc == -1 and "lag_bounds of window 1, pair 2" in text, text
        # then refine, in front of the overlap
        for bad in (1, 3, -2, 32):
            rc, text = call(good, refine=bad, quality=over)
            assert rc == -1 and "refine = %d" % bad in text, text
        # then quality over another output, the array named -- with refine = 0 too
        for refine in (0, 8):
            for k, nm in enumerate(("lag_int", "lag_frac", "peak")):
                rc, text = call(good, refine=refine, quality=out[k].view(np.float32).reshape(-1)[-1:])
                assert rc == -1 and "quality overlaps " + nm in text, text
            outs = [out[0], out[1], block[4 * W * M * P - 1:].view(np.float32)]     # peak starts on quality's last float
            rc, text = call(good, refine=refine, outs=outs)
            assert rc == -1 and "quality overlaps peak" in text, text
        assert all(np.all(o == 77) for o in out) and np.all(block == 77), "a refused call wrote an output"
        with pytest.raises(xc.RmxError):
            eng.correlate_bands(iq, [[0.5, 0.5], [0.1, 0.2]], refine=4)
        # an empty batch returns RMX_OK and writes nothing
        assert call(good, n_windows=0)[0] == 0
        assert call(good, pairs=np.zeros((1, 2), np.int32), n_pairs=0)[0] == 0
        assert all(np.all(o == 77) for o in out) and np.all(block == 77)


def test_seam_share_qualified_gives_the_measurements_of_the_separate_calls(xc):
    """TDoAProcessor with band_limit, refine = 8 and min_psr on a two-transmitter capture of three buoys, N = 4096: the two
    frequency groups once as two windows of the quality call and once, share_captures + share_qualified, as one window
    under two bands -- identical measurements in the same order, and the banded call carried refine and quality."""
    from radio_mapper_amd import tdoa_processor as tp
    fs, N, fc = 2.048e6, 4096, 121.0e6
    lat0, lng0 = 37.0, -122.0
    buoys = [("B0", lat0, lng0), ("B1", lat0 + 0.3, lng0), ("B2", lat0, lng0 + 0.4)]
    xyz = [tp.GeodeticCalculator.lat_lng_to_xyz(la, lo, 0.0) for _, la, lo in buoys]
    tx = {"strong": (lat0 + 0.1, lng0 + 0.12), "weak": (lat0 + 0.22, lng0 + 0.3)}
    delays = {}
    for k, (la, lo) in tx.items():
        e = tp.GeodeticCalculator.lat_lng_to_xyz(la, lo, 0.0)
        d = [math.dist(e, x) / tp.TDoACalculator.SPEED_OF_LIGHT * fs for x in xyz]
        delays[k] = [int(round(v - min(d))) for v in d]
    iq, _, _ = wr.two_emitter_scene(N=N, d_strong=delays["strong"], d_weak=delays["weak"], seed=6)
    f_strong, f_weak = fc + 0.10 * fs, fc - 0.25 * fs
    t0 = 1_700_000_000_000_000_000

    def run(bound_lags, min_psr, **flags):
        p = tp.TDoAProcessor(band_limit=True, refine=8, min_psr=min_psr, correlation_confidence=True, **flags)
        p.tdoa_calculator.bound_lags = bound_lags
        for bid, la, lo in buoys:
            p.register_buoy(tp.BuoyPosition(bid, la, lo, 0.0, timing_accuracy_ns=20))
        calls, groups = [], []
        eng_of = p.tdoa_calculator._engine

        def engine(*a, **k):
            eng = eng_of(*a, **k)
            if not getattr(eng, "_recorded", False):
                for name in ("correlate", "correlate_bands"):
                    def rec(*aa, _f=getattr(eng, name), _n=name, **kk):
                        calls.append((_n, np.asarray(aa[0]).shape[0], kk.get("refine", 0), bool(kk.get("quality", False))))
                        return _f(*aa, **kk)
                    setattr(eng, name, rec)
                eng._recorded = True
            return eng
        p.tdoa_calculator._engine = engine
        p.hyperbolic_positioner.triangulate_position = lambda meas, pos: groups.append(
            [(m.buoy1_id, m.buoy2_id, m.frequency_mhz, m.time_difference_ns, m.confidence) for m in meas])
        dets = []
        for f in (f_strong, f_weak):
            dets += [tp.SignalDetection(bid, f / 1e6, -60.0, "t", t0, la, lo, 0.9, iq_samples=iq[0, b], sample_rate_hz=fs,
                                        center_freq_hz=fc, bandwidth_hz=0.1 * fs)
                     for b, (bid, la, lo) in enumerate(buoys)]
        p.process_signal_detections(dets)
        p.tdoa_calculator.close()
        return calls, groups

    for bound_lags in (False, True):
        for min_psr in (2.0, 1e9):         # every pair passes / every pair is dropped, on both sides alike
            calls_on, meas_on = run(bound_lags, min_psr, share_captures=True, share_qualified=True)
            calls_off, meas_off = run(bound_lags, min_psr, share_captures=False)
            assert calls_on == [("correlate_bands", 1, 8, True)] and calls_off == [("correlate", 2, 8, True)]
            assert meas_on == meas_off
            assert len(meas_on) == (2 if min_psr < 1e9 else 0)
            if meas_on:
                assert [len(g) for g in meas_on] == [3, 3]
                for g, k in zip(meas_on, ("strong", "weak")):
                    lag = np.array([m[3] * 1e-9 * fs for m in g])
                    assert np.all(np.abs(lag - wr.true_lags(delays[k])) < 0.5), (k, lag)
            # share_captures alone stands back, as before
            assert run(bound_lags, min_psr, share_captures=True)[0] == calls_off
