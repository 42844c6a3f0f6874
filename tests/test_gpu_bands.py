"""rmx_xcorr_batch_bands on the GPU: several bands per window over one set of forward spectra, against the float32
reference (tests/bands_ref.py) on every route that forms the product, bit for bit against the weighted call band by
band, the forward launch counts, the bin map of each product kernel, the two-emitter scene in ONE call, the refusals and
the seam with share_captures."""
import ctypes as C
import math

import numpy as np
import pytest

import bands_ref as br
import radio_mapper_amd as rm
import weighted_ref as wr

pytestmark = pytest.mark.gpu
TOL = 1e-5
MAX_LEFT_OUT = 0.02   # of a call's slots: the parity rule must not be satisfied by leaving slots out


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


def _left_out(ref):
    """the slots the parity rule leaves out: a reference top-two margin of at most 1e-5, or a slice that holds only the
    float32 transforms' rounding noise (tests/test_gpu_weighted.py: _assert_parity)"""
    _, _, rp, mg, fm, _ = ref
    return ~((mg > TOL) & (rp > 1e-5 * fm))


def _assert_parity(li, lf, pk, ref):
    """the parity rule of include/rmx.h (rmx_xcorr_batch_weighted), on [W][M][P] arrays: lag_int bit-exact where the
    reference's top-two margin exceeds 1e-5; lag_frac within 1e-5 * max(|lag|, 1), or within four one-ulp bounds of the
    reference's own taps (a flat peak); peak within 1e-5 relative + 1e-6 of the vector's maximum.  At most 2 % of the slots
    may be left out."""
    ri, rf, rp, mg, fm, fb = ref
    out = _left_out(ref)
    print("slots %d, left out %d" % (out.size, int(out.sum())))
    assert out.sum() <= MAX_LEFT_OUT * out.size, "the rule leaves out %d of %d slots" % (int(out.sum()), out.size)
    ok = ~out
    assert np.array_equal(li[ok], ri[ok]), "integer lags differ from the reference: %d" % int((li != ri)[ok].sum())
    got, want = li[ok] + lf[ok].astype(np.float64), ri[ok] + rf[ok]
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    assert np.all((rel <= TOL) | (rel <= 4.0 * fb[ok])), (rel.max(), fb[ok][np.argmax(rel)])
    assert np.all(np.abs(pk[ok] - rp[ok]) <= 1e-5 * rp[ok] + 1e-6 * fm[ok])


def _random_bands(rng, shape, N):
    """uniformly random [lo, hi] bands at least 2 bins of the 2N-point transform wide"""
    a = rng.uniform(-0.5, 0.5, size=shape + (2,))
    lo, hi = a.min(-1), a.max(-1)
    lo = np.minimum(lo, 0.5 - 2.0 / (2 * N))
    return np.stack([lo, np.maximum(hi, lo + 2.0 / (2 * N))], -1)


def _random_bounds(rng, shape, N, true=None):
    """random lag intervals [..][2]; true (the pairs' true lags, broadcast to `shape`): three intervals in four then hold
    it -- at an edge now and then: the parabola's edge rule -- so that the slice has a peak the parity rule can judge (a
    slice of side lobes alone is often flat to 1e-5: the reference's own top-two margin leaves it out)"""
    a = rng.integers(-(N - 1), N, size=shape + (2,))
    b = np.stack([a.min(-1), a.max(-1)], -1).astype(np.int64)
    if true is not None:
        t = np.broadcast_to(np.rint(true).astype(np.int64), shape)
        reach = rng.integers(0, max(N // 2, 2), size=shape + (2,)) * rng.integers(0, 4, size=shape + (2,)).clip(0, 1)
        around = np.stack([np.maximum(t - reach[..., 0], -(N - 1)), np.minimum(t + reach[..., 1], N - 1)], -1)
        b = np.where((rng.integers(0, 4, size=shape) > 0)[..., None], around, b)
    return b.astype(np.int32)


def _true_lags(delays, pairs, B):
    pairs = pairs or [(i, j) for i in range(B) for j in range(i + 1, B)]
    return np.stack([delays[:, j] - delays[:, i] for i, j in pairs], -1)       # [W][P]


# (route name, N, buoys, windows, bands, default options, engine options, forward families, pair family)
CUSTOM = [(1, 0), (0, 2), (2, 2), (0, 1)]   # a reversed pair and a self pair
ROUTES = [
    ("k_pair_res", 4096, 3, 2, 3, {}, {}, ("k_fwd",), "k_win|k_pair"),
    ("k_pair_res xcd_map", 4096, 8, 1, 8, {}, {}, ("k_fwd",), "k_win|k_pair"),
    ("k_pair_str", 4096, 4, 3, 2, {}, {"resident": 0}, ("k_fwd",), "k_win|k_pair"),
    ("k_pair_res chunk_windows 2", 4096, 3, 5, 3, {}, {"chunk_windows": 2}, ("k_fwd",), "k_win|k_pair"),
    ("k_pair_res chunk seam", 4096, 3, 11, 3, {}, {"chunk_windows": 8}, ("k_fwd",), "k_win|k_pair"),
    ("g_pair_small N=16", 16, 3, 5, 3, {}, {}, ("g_fwd_small",), "g_pair_small"),
    ("g_pair_small N=16 gen_chunk 2", 16, 3, 5, 3, {"gen_chunk": 2}, {}, ("g_fwd_small",), "g_pair_small"),
    ("g_pair_small N=256", 256, 4, 5, 3, {}, {}, ("g_fwd_small",), "g_pair_small"),
    ("g_pair_small generic4096", 4096, 3, 2, 3, {"generic4096": 1}, {}, ("g_fwd_small",), "g_pair_small"),
    ("g_pair_small N=16 64 bands", 16, 3, 2, 64, {}, {}, ("g_fwd_small",), "g_pair_small"),
    ("four-step N=8192 3 buoys", 8192, 3, 2, 2, {}, {}, ("g_cols_fwd", "g_rows_fwd"), "g_rows_inv"),
    ("four-step N=8192 8 buoys", 8192, 8, 1, 2, {}, {}, ("g_cols_fwd", "g_rows_fwd"), "g_rows_inv"),
    ("four-step N=8192 8 buoys rows_anchor 0", 8192, 8, 1, 2, {"rows_anchor": 0}, {}, ("g_cols_fwd", "g_rows_fwd"), "g_rows_inv"),
    ("four-step N=256 small_maxl 256", 256, 3, 4, 8, {"small_maxl": 256}, {}, ("g_cols_fwd", "g_rows_fwd"), "g_rows_inv"),
    ("four-step N=256 gen_chunk 2", 256, 3, 5, 3, {"small_maxl": 256, "gen_chunk": 2}, {}, ("g_cols_fwd", "g_rows_fwd"), "g_rows_inv"),
]
# the case generator's seed per route: the smallest for which the float32 reference's own top-two margin leaves out no slot
# of any case (found on the CPU with the reference alone)
SEEDS = {"k_pair_res": 1, "k_pair_res xcd_map": 1, "k_pair_str": 1, "k_pair_res chunk_windows 2": 1, "k_pair_res chunk seam": 3,
         "g_pair_small N=16": 1, "g_pair_small N=16 gen_chunk 2": 1, "g_pair_small N=256": 1, "g_pair_small generic4096": 1,
         "g_pair_small N=16 64 bands": 1, "four-step N=8192 3 buoys": 1, "four-step N=8192 8 buoys": 1, "four-step N=8192 8 buoys rows_anchor 0": 1,
         "four-step N=256 small_maxl 256": 4, "four-step N=256 gen_chunk 2": 3}
FORBIDDEN = ("g_win_*", "g_rows_fused", "g_rows_anchor", "k16_fwd", "k16_pairs")


def _cases(route):
    """the calls of one route: (bands, PHAT, lag bounds, pair list); few buoys get every combination, many a cut"""
    name, N, B, W, M = route[:5]
    rng = np.random.default_rng(SEEDS[name])
    delays = _inputs(route)[1]
    shared = _random_bands(rng, (M,), N)
    per_win = _random_bands(rng, (W, M), N)
    P = B * (B - 1) // 2
    lb = _random_bounds(rng, (W, P), N, _true_lags(delays, None, B))
    lb_shared = _random_bounds(rng, (P,), N, _true_lags(delays, None, B)[0])
    lb_custom = _random_bounds(rng, (W, len(CUSTOM)), N, _true_lags(delays, CUSTOM, B))
    cases = [(shared, False, None, None), (per_win, True, lb, None), (per_win, False, lb_shared, None), (shared, True, None, None),
             (per_win, False, None, CUSTOM), (shared, True, lb_custom, CUSTOM)]
    if B <= 4 and M <= 8:
        cases += [(per_win, False, None, None), (per_win, True, None, None), (shared, False, lb, None), (shared, True, lb_shared, None),
                  (per_win, True, None, CUSTOM), (per_win, False, lb_custom, CUSTOM)]
    return cases


def _inputs(route):
    name, N, B, W = route[:4]
    iq, delays, raw = rm.synth.make_windows(W, B, N, 10e6, seed=len(name), return_u8=True)
    return iq, delays, raw


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_against_the_reference_and_the_weighted_call(xc, opts, route):
    """Per route and case: parity with bands_ref; [:, m] bit for bit the weighted call with band m on an engine with the
    same options; uint8 input and a repeated call bit-identical; ONE forward pass (the forward families' launch counts are
    a single-band call's) and none of the kernels that keep their spectra to themselves.
    One route is held to bands_ref alone: four-step with the default pair list from 6 buoys on, where the weighted call's
    inverse rows are g_rows_anchor, a different kernel from the product-on-load g_rows that every banded call takes (the
    peaks differ in a last bit there; measured: 3002209.5 against 3002209.8).  With a custom pair list, or with option
    rows_anchor = 0, the weighted call takes g_rows too and the bits are the same."""
    name, N, B, W, M, dopt, eopt, fwd, pair_family = route
    for k, v in dopt.items():
        opts(k, v)
    iq, _, raw = _inputs(route)
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        eng.set_option("timing", 1)
        for bands, phat, bounds, pairs in _cases(route):
            got = eng.correlate_bands(iq, bands, pairs, lag_bounds=bounds, whiten=phat)
            tk = eng.last_timing_by_kernel()
            assert got[0].shape == (W, M, len(pairs) if pairs else B * (B - 1) // 2)
            _assert_parity(*got, br.bands_batch(iq, bands, phat, bounds, pairs, with_bound=True))
            pw = br.per_window(bands, W)
            anchor = len(fwd) == 2 and B >= 6 and pairs is None and dopt.get("rows_anchor", 1) != 0
            for m in range(M):
                one = eng.correlate(iq, pairs, lag_bounds=bounds, band=pw[:, m], whiten=phat)
                tk1 = eng.last_timing_by_kernel()
                assert anchor == ("g_rows_anchor" in tk1), tk1
                if not anchor:
                    assert _same([g[:, m] for g in got], one), "band %d differs from the weighted call" % m
            assert set(tk) == set(fwd) | {pair_family} | ({"g_cols_inv", "g_final"} if len(fwd) == 2 else set()), tk
            assert not set(tk) & set(FORBIDDEN)
            for f in fwd:
                assert tk[f]["launches"] == tk1[f]["launches"], (f, tk, tk1)
            assert _same(got, eng.correlate_bands(raw, bands, pairs, lag_bounds=bounds, whiten=phat)), "uint8 input"
            assert _same(got, eng.correlate_bands(iq, bands, pairs, lag_bounds=bounds, whiten=phat)), "the same call twice"


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_one_band_is_the_weighted_call(xc, opts, route):
    name, N, B, W, M, dopt, eopt, fwd, pair_family = route
    for k, v in dopt.items():
        opts(k, v)
    iq, _, _ = _inputs(route)
    rng = np.random.default_rng(N + W)
    bands = _random_bands(rng, (W, 1), N)
    lb = _random_bounds(rng, (W, B * (B - 1) // 2), N)
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        eng.set_option("timing", 1)
        for phat, bounds in ((False, None), (True, lb)):
            a = eng.correlate_bands(iq, bands, lag_bounds=bounds, whiten=phat)
            ta = eng.last_timing_by_kernel()
            b = eng.correlate(iq, lag_bounds=bounds, band=bands[:, 0], whiten=phat)
            tb = eng.last_timing_by_kernel()
            assert _same([x[:, 0] for x in a], b)
            assert {k: v["launches"] for k, v in ta.items()} == {k: v["launches"] for k, v in tb.items()}


@pytest.mark.parametrize("route", [ROUTES[0], ROUTES[2], ROUTES[7], ROUTES[10]], ids=lambda r: r[0])
def test_device_pointers_and_reuse_of_the_callers_arrays(xc, opts, route):
    torch = pytest.importorskip("torch")
    name, N, B, W, M, dopt, eopt, _, _ = route
    for k, v in dopt.items():
        opts(k, v)
    iq, _, raw = _inputs(route)
    P = B * (B - 1) // 2
    rng = np.random.default_rng(7)
    bands, lb = _random_bands(rng, (W, M), N), _random_bounds(rng, (W, P), N)
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        host = eng.correlate_bands(iq, bands, lag_bounds=lb, whiten=True)
        for x, u8 in ((iq.view(np.float32), False), (raw, True)):
            d_iq = torch.from_numpy(x).cuda()
            outs = [torch.full((W, M, P), -7, dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.float32)]
            torch.cuda.synchronize()
            mine, mine_lb = bands.copy(), lb.copy()
            eng.correlate_bands_device(d_iq.data_ptr(), W, mine, *[o.data_ptr() for o in outs], u8=u8, lag_bounds=mine_lb,
                                       whiten=True)
            mine[:] = (0.0, 0.0)                             # the caller may reuse its arrays at once
            mine_lb[:] = 0
            eng.synchronize()
            assert _same(host, [o.cpu().numpy() for o in outs])


SINGLE = [("k_pair_res", 4096, {}, {}), ("k_pair_str", 4096, {}, {"resident": 0}), ("g_pair_small", 256, {}, {}),
          ("g_pair_small generic4096", 4096, {"generic4096": 1}, {}), ("four-step rows", 8192, {}, {}),
          ("four-step rows N=256", 256, {"small_maxl": 256}, {})]


@pytest.mark.parametrize("route", SINGLE, ids=[r[0] for r in SINGLE])
def test_single_bin_bands_pin_each_product_kernels_bin_map(xc, opts, route):
    """single-bin bands as the M bands of ONE window: peak = |X_j[s]| |X_i[s]| / L (a single bin is a flat correlation:
    the lags are not compared)"""
    name, N, dopt, eopt = route
    for k, v in dopt.items():
        opts(k, v)
    L = 2 * N
    rng = np.random.default_rng(N)
    bins = [-N, -1, 0, 1, N - 1] + [int(v) for v in rng.integers(-N, N, size=6)]
    iq, _ = rm.synth.make_windows(1, 2, N, 10e6, seed=5)
    X = [np.fft.fft(iq[0, b].astype(np.complex128), L) for b in range(2)]
    bands = np.array([[s / L, s / L] for s in bins])
    with xc.XcorrEngine(2, N, 1) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        _, _, pk = eng.correlate_bands(iq, bands)
    want = np.array([abs(X[1][s % L]) * abs(X[0][s % L]) / L for s in bins])
    assert np.allclose(pk[0, :, 0], want, rtol=1e-4, atol=0), (bins, pk[0, :, 0], want)


@pytest.mark.parametrize("N", [4096, 16384])
def test_two_emitters_in_one_call(xc, N):
    """the scene the entry is for: ONE call, ONE window, two bands -> each emitter's own lags"""
    iq, ds, dw = wr.two_emitter_scene(N=N)
    bands = np.array([wr.STRONG_BAND, wr.WEAK_BAND])
    with xc.XcorrEngine(4, N, 1) as eng:
        li, lf, pk = eng.correlate_bands(iq, bands)
        _assert_parity(li, lf, pk, br.bands_batch(iq, bands, with_bound=True))
        assert np.all(np.abs(li[0, 0] + lf[0, 0] - wr.true_lags(ds)) < 0.5)
        assert np.all(np.abs(li[0, 1] + lf[0, 1] - wr.true_lags(dw)) < 0.5)


def test_refusals_leave_the_outputs_untouched(xc):
    N, W, M, P = 256, 4, 3, 3
    iq, _ = rm.synth.make_windows(W, 3, N, 10e6, seed=1)
    lib = xc.load_library()
    good = np.tile([[-0.5, 0.5], [0.0, 0.25], [-0.1, 0.1]], (W, 1, 1))
    with xc.XcorrEngine(3, N, W) as eng:
        out = [np.full((W, M, P), 77, t) for t in (np.int32, np.float32, np.float32)]

        def call(bands, n_bands=M, per_window=1, bounds=None, bounds_pw=0, weighting=0, iq_p=iq):
            b = None if bands is None else np.ascontiguousarray(bands, np.float64)
            lb = None if bounds is None else np.ascontiguousarray(bounds, np.int32)
            rc = lib.rmx_xcorr_batch_bands(eng._ctx, None if iq_p is None else iq_p.ctypes.data_as(C.c_void_p), W, None, P,
                                           None if b is None else b.ctypes.data_as(C.c_void_p), n_bands, per_window, weighting,
                                           None if lb is None else lb.ctypes.data_as(C.c_void_p), bounds_pw,
                                           *[o.ctypes.data_as(C.c_void_p) for o in out], 0)
            return rc, lib.rmx_last_error(eng._ctx).decode()
        assert call(good)[0] == 0 and not np.any(out[0] == 77)
        for o in out:
            o[:] = 77
        for n_bands in (0, 65, -1):
            rc, text = call(good, n_bands=n_bands)
            assert rc == -1 and "n_bands" in text
        assert call(None) == (-1, "NULL buffer") and call(good, iq_p=None) == (-1, "NULL buffer")
        assert call(None, n_bands=0)[1] == "NULL buffer"      # the NULL buffer is refused first
        for bad in ([0.5, 0.5], [np.nan, 0.1], [0.2, 0.1], [-0.6, 0.1], [1e-9, 2e-9]):
            bands = good.copy()
            bands[2, 1] = bad
            rc, text = call(bands)
            assert rc == -1 and "band 1 of window 2" in text, text
            rc, text = call(bands[2], per_window=0)
            assert rc == -1 and "band 1 of window 0" in text and "shared" in text, text
        assert "keeps no bin" in call(np.tile([[0.5, 0.5]], (W, M, 1)))[1]
        rc, text = call(good, weighting=2)
        assert rc == -1 and "weighting" in text
        rc, text = call(good, n_bands=0, weighting=2)          # n_bands is refused in front of the weighted entry's checks
        assert "n_bands" in text
        for lo, hi in ((-N, 0), (0, N), (5, 4)):
            lb = np.tile(np.array([[-3, 3]], np.int32), (W, P, 1))
            lb[1, 2] = (lo, hi)
            rc, text = call(good, bounds=lb, bounds_pw=1)
            assert rc == -1 and "lag_bounds of window 1, pair 2" in text, text
        assert all(np.all(o == 77) for o in out), "a refused call wrote an output"
        with pytest.raises(xc.RmxError):
            eng.correlate_bands(iq, [[0.5, 0.5]])
        # an empty batch returns RMX_OK and writes nothing
        assert lib.rmx_xcorr_batch_bands(eng._ctx, iq.ctypes.data_as(C.c_void_p), 0, None, P, good.ctypes.data_as(C.c_void_p), M, 1, 0,
                                         None, 0, *[o.ctypes.data_as(C.c_void_p) for o in out], 0) == 0
        pr = np.zeros((1, 2), np.int32)
        assert lib.rmx_xcorr_batch_bands(eng._ctx, iq.ctypes.data_as(C.c_void_p), W, pr.ctypes.data_as(C.c_void_p), 0,
                                         good.ctypes.data_as(C.c_void_p), M, 1, 0, None, 0,
                                         *[o.ctypes.data_as(C.c_void_p) for o in out], 0) == 0
        assert all(np.all(o == 77) for o in out)


def test_seam_share_captures_gives_the_measurements_of_the_separate_calls(xc):
    """TDoAProcessor with band_limit on a two-transmitter capture (tests/test_gpu_weighted.py:
    test_seam_band_limit_separates_two_transmitters), the two frequency groups once as two windows of the weighted call and
    once, share_captures, as one window under two bands: identical measurements, identical fixes, and the true positions"""
    from radio_mapper_amd import tdoa_processor as tp
    fs, N, fc = 2.048e6, 4096, 121.0e6
    lat0, lng0 = 37.0, -122.0
    buoys = [("B0", lat0, lng0), ("B1", lat0 + 0.3, lng0), ("B2", lat0, lng0 + 0.4), ("B3", lat0 + 0.3, lng0 + 0.4)]
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

    def run(share, bound_lags):
        p = tp.TDoAProcessor(band_limit=True, share_captures=share)
        p.tdoa_calculator.bound_lags = bound_lags
        for bid, la, lo in buoys:
            p.register_buoy(tp.BuoyPosition(bid, la, lo, 0.0, timing_accuracy_ns=20))
        calls, groups = [], {}
        eng_of = p.tdoa_calculator._engine

        def engine(*a, **k):
            eng = eng_of(*a, **k)
            if not getattr(eng, "_recorded", False):
                for name in ("correlate", "correlate_bands"):
                    def rec(*aa, _f=getattr(eng, name), _n=name, **kk):
                        calls.append((_n, np.asarray(aa[0]).shape[0]))
                        return _f(*aa, **kk)
                    setattr(eng, name, rec)
                eng._recorded = True
            return eng
        p.tdoa_calculator._engine = engine
        p.hyperbolic_positioner.triangulate_position = lambda meas, pos: groups.__setitem__(meas[0].frequency_mhz, meas)
        dets = []
        for f in (f_strong, f_weak):
            dets += [tp.SignalDetection(bid, f / 1e6, -60.0, "t", t0, la, lo, 0.9, iq_samples=iq[0, b], sample_rate_hz=fs,
                                        center_freq_hz=fc, bandwidth_hz=0.1 * fs)
                     for b, (bid, la, lo) in enumerate(buoys)]
        p.process_signal_detections(dets)
        p.tdoa_calculator.close()
        fixes = {}
        for f, meas in groups.items():
            k = "strong" if abs(f - f_strong / 1e6) < 0.01 else "weak"
            assert len(meas) == 6
            lag = np.array([[m.time_difference_ns * 1e-9 * fs for m in meas]])
            li = np.rint(lag).astype(np.int32)
            with xc.XcorrEngine(4, N, 1) as eng:
                pos, _, _ = eng.solve(np.array(xyz), li, (lag - li).astype(np.float32), fs)
            e = np.asarray(tp.GeodeticCalculator.lat_lng_to_xyz(tx[k][0], tx[k][1], 0.0))
            up = e / np.linalg.norm(e)
            err = pos[0] - e
            fixes[k] = (float(np.linalg.norm(err - np.dot(err, up) * up)), pos[0].tolist())
        meas = {f: [(m.buoy1_id, m.buoy2_id, m.time_difference_ns, m.confidence) for m in ms] for f, ms in groups.items()}
        return calls, meas, fixes

    for bound_lags in (False, True):
        calls_on, meas_on, fix_on = run(True, bound_lags)
        calls_off, meas_off, fix_off = run(False, bound_lags)
        assert calls_on == [("correlate_bands", 1)] and calls_off == [("correlate", 2)]
        assert meas_on == meas_off and fix_on == fix_off
        assert set(fix_on) == {"strong", "weak"} and fix_on["strong"][0] < 1000 and fix_on["weak"][0] < 1000, fix_on
