"""rmx_xcorr_batch_weighted on the GPU: band-limited and PHAT-weighted correlation against the float32 reference
(tests/weighted_ref.py) on every route, the bin map of each forward kernel, delegation to the plain calls, the two
scenarios the weighting exists for, the seam end to end, and argument errors."""
import math
import zlib

import numpy as np
import pytest

import radio_mapper_amd as rm
import weighted_ref as wr

pytestmark = pytest.mark.gpu
TOL = 1e-5


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


def _ref(*a, **k):
    return wr.weighted_batch(*a, with_bound=True, **k)


def _assert_parity(li, lf, pk, ref):
    """the parity rule of include/rmx.h: lag_int bit-exact where the reference's top-two margin exceeds 1e-5; lag_frac
    within 1e-5 * max(|lag|, 1), or within four one-ulp bounds of the reference's own taps (a flat peak).  A slice whose
    peak lies below 1e-5 of the whole vector's maximum holds only the float32 transforms' rounding noise (PHAT on the
    self pair (2, 2) with a lag window that excludes 0: r is a unit impulse at lag 0): peak is checked there, lags not."""
    ri, rf, rp, mg, fm, fb = ref
    ok = (mg > TOL) & (rp > 1e-5 * fm)
    assert np.array_equal(li[ok], ri[ok]), "integer lags differ from the reference: %d" % int((li != ri)[ok].sum())
    got, want = li[ok] + lf[ok].astype(np.float64), ri[ok] + rf[ok]
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    assert np.all((rel <= TOL) | (rel <= 4.0 * fb[ok])), (rel.max(), fb[ok][np.argmax(rel)])
    assert np.all(np.abs(pk[ok] - rp[ok]) <= 1e-5 * rp[ok] + 1e-6 * fm[ok])


def _random_band(rng, shape, N):
    """random [lo, hi] bands that keep at least one bin of the 2N-point transform (at least 2 / L wide)"""
    a = rng.uniform(-0.5, 0.5, size=shape + (2,))
    lo, hi = a.min(-1), a.max(-1)
    lo = np.minimum(lo, 0.5 - 2.0 / (2 * N))
    return np.stack([lo, np.maximum(hi, lo + 2.0 / (2 * N))], -1)


def _random_bounds(rng, shape, N):
    a = rng.integers(-(N - 1), N, size=shape + (2,))
    return np.stack([a.min(-1), a.max(-1)], -1).astype(np.int32)


# (route name, N, buoys, windows, default options, engine options, custom pair list, expected forward family)
ROUTES = [
    ("k_fwd 1 window", 4096, 8, 1, {}, {}, None, "k_fwd"),
    ("k_fwd 300 windows", 4096, 4, 300, {}, {}, None, "k_fwd"),
    ("k_fwd 1500 windows chunked", 4096, 3, 1500, {}, {"chunk_windows": 200}, None, "k_fwd"),
    ("k_fwd custom pairs", 4096, 5, 12, {}, {}, [(3, 1), (0, 4), (2, 2), (4, 0)], "k_fwd"),
    ("g_fwd_small N=16", 16, 3, 40, {}, {}, None, "g_fwd_small"),
    ("g_fwd_small N=256", 256, 4, 300, {}, {}, None, "g_fwd_small"),
    ("g_fwd_small N=2048", 2048, 8, 120, {}, {}, None, "g_fwd_small"),
    ("g_fwd_small generic4096", 4096, 3, 20, {"generic4096": 1}, {}, None, "g_fwd_small"),
    ("four-step N=8192 3 buoys", 8192, 3, 40, {}, {}, None, "g_rows_fwd"),
    ("four-step N=8192 8 buoys", 8192, 8, 64, {}, {}, None, "g_rows_fwd"),
    ("four-step N=16384 3 buoys", 16384, 3, 24, {}, {}, None, "g_rows_fwd"),
    ("four-step N=16384 8 buoys", 16384, 8, 24, {}, {}, None, "g_rows_fwd"),
    ("four-step N=2^18 3 buoys", 1 << 18, 3, 2, {}, {}, None, "g_rows_fwd"),
    ("four-step N=2^18 8 buoys", 1 << 18, 8, 1, {}, {}, None, "g_rows_fwd"),
]
FORBIDDEN = ("g_win_*", "g_rows_fused", "k16_fwd", "k16_pairs")


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_against_the_reference(xc, opts, route):
    name, N, B, W, dopt, eopt, pairs, fwd = route
    for k, v in dopt.items():
        opts(k, v)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    iq, _, raw = rm.synth.make_windows(W, B, N, 10e6, seed=len(name), return_u8=True)
    P = B * (B - 1) // 2 if pairs is None else len(pairs)
    shared = _random_band(rng, (), N)
    per_win = _random_band(rng, (W,), N)
    per_win[0] = (-0.5, 0.5)
    lb = _random_bounds(rng, (W, P), N)
    big = W * B * N > (1 << 21)      # (the reference is slow on large batches: fewer combinations there)
    cases = [(shared, False, None), (per_win, True, None), (per_win, False, lb), (None, True, lb)]
    if not big:
        cases += [(shared, True, lb), (None, True, None), (per_win, False, None)]
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        eng.set_option("timing", 1)
        for band, phat, bounds in cases:
            li, lf, pk = eng.correlate(iq, pairs, lag_bounds=bounds, band=band, whiten=phat)
            tk = eng.last_timing_by_kernel()
            fams = set(tk)
            assert fwd in fams and not (fams & set(FORBIDDEN)), fams
            if fwd == "k_fwd":   # k_win and k_pair share one timing family: one pair launch per k_fwd launch = no k_win
                assert tk["k_win|k_pair"]["launches"] == tk["k_fwd"]["launches"], tk
            _assert_parity(li, lf, pk, _ref(iq, band, phat, bounds, pairs))
            li8, lf8, pk8 = eng.correlate(raw, pairs, lag_bounds=bounds, band=band, whiten=phat)
            assert np.array_equal(li, li8) and np.array_equal(lf, lf8) and np.array_equal(pk, pk8)


SINGLE = [("k_fwd", 4096, {}), ("g_fwd_small", 256, {}), ("g_fwd_small 4096", 4096, {"generic4096": 1}),
          ("g_rows", 8192, {}), ("g_rows 2^18", 1 << 18, {})]


@pytest.mark.parametrize("route", SINGLE, ids=[r[0] for r in SINGLE])
def test_single_bin_bands_pin_each_bin_map(xc, opts, route):
    name, N, dopt = route
    for k, v in dopt.items():
        opts(k, v)
    L = 2 * N
    rng = np.random.default_rng(N)
    bins = [-N, -1, 0, 1, N - 1] + [int(v) for v in rng.integers(-N, N, size=6)]
    iq, _ = rm.synth.make_windows(1, 2, N, 10e6, seed=5)
    X = [np.fft.fft(iq[0, b].astype(np.complex128), L) for b in range(2)]
    band = np.array([[s / L, s / L] for s in bins])
    W = len(bins)
    with xc.XcorrEngine(2, N, W) as eng:
        _, _, pk = eng.correlate(np.repeat(iq, W, axis=0), band=band)
    want = np.array([abs(X[1][s % L]) * abs(X[0][s % L]) / L for s in bins])
    assert np.allclose(pk[:, 0], want, rtol=1e-4, atol=0), (bins, pk[:, 0], want)


@pytest.mark.parametrize("N,W,o", [(16, 5, {}), (256, 40, {}), (4096, 8, {}), (4096, 300, {}), (8192, 40, {"wscr": 2}),
                                   (16384, 12, {"kwin16k": 2}), (1 << 17, 2, {})])
def test_full_band_none_is_the_plain_call(xc, opts, N, W, o):
    for k, v in o.items():
        opts(k, v)
    iq, _, raw = rm.synth.make_windows(W, 3, N, 10e6, seed=N, return_u8=True)
    lb = _random_bounds(np.random.default_rng(N), (W, 3), N)
    with xc.XcorrEngine(3, N, W) as eng:
        for x in (iq, raw):
            a = eng.correlate(x)
            for band in ([-0.5, 0.5], np.tile([[-0.5, 0.5]], (W, 1))):
                b = eng.correlate(x, band=band)
                assert all(np.array_equal(u, v) for u, v in zip(a, b))
            c = eng.correlate(x, lag_bounds=lb)
            d = eng.correlate(x, lag_bounds=lb, band=[-0.5, 0.5])
            assert all(np.array_equal(u, v) for u, v in zip(c, d))


@pytest.mark.parametrize("N", [4096, 8192])
def test_dc_offset_scenario(xc, N):
    iq, d = wr.dc_offset_scene(N=N, delays=(0, 1100 * N // 4096, 2300 * N // 4096))
    t = wr.true_lags(d)
    with xc.XcorrEngine(3, N, 1) as eng:
        li, _, _ = eng.correlate(iq)
        assert np.all(np.abs(li[0]) < 20 * N // 4096)
        for band, phat in (((0.02, 0.5), False), (None, True)):
            li, lf, pk = eng.correlate(iq, band=band, whiten=phat)
            _assert_parity(li, lf, pk, _ref(iq, band, phat))
            assert np.all(np.abs(li[0] + lf[0] - t) < 0.5)


@pytest.mark.parametrize("N", [4096, 16384])
def test_two_emitter_scenario(xc, N):
    iq, ds, dw = wr.two_emitter_scene(N=N)
    with xc.XcorrEngine(4, N, 2) as eng:
        li, lf, _ = eng.correlate(iq)
        assert np.all(np.abs(li[0] + lf[0] - wr.true_lags(ds)) < 0.5)
        both = np.concatenate([iq, iq])
        band = np.array([wr.STRONG_BAND, wr.WEAK_BAND])
        li, lf, pk = eng.correlate(both, band=band)
        _assert_parity(li, lf, pk, _ref(both, band))
        assert np.all(np.abs(li[0] + lf[0] - wr.true_lags(ds)) < 0.5)
        assert np.all(np.abs(li[1] + lf[1] - wr.true_lags(dw)) < 0.5)


@pytest.mark.parametrize("N,W", [(4096, 1), (4096, 300), (256, 8), (8192, 4)])
def test_dead_receiver_under_phat(xc, N, W):
    iq, _ = rm.synth.make_windows(W, 3, N, 10e6, seed=9)
    iq[:, 1] = 0
    lb = np.array([[-(N - 1), N - 1], [-5, 9], [-(N - 1), N - 1]], np.int32)
    with xc.XcorrEngine(3, N, W) as eng:
        for bounds in (None, lb):
            li, lf, pk = eng.correlate(iq, band=[-0.3, 0.4], whiten=True, lag_bounds=bounds)
            assert np.all(np.isfinite(lf)) and np.all(np.isfinite(pk))
            dead = [0, 2]                                     # pairs (0,1), (1,2)
            lo = np.array([-(N - 1), -(N - 1)]) if bounds is None else lb[dead, 0]
            assert np.all(li[:, dead] == lo) and np.all(lf[:, dead] == 0) and np.all(pk[:, dead] == 0)
            assert np.all(pk[:, 1] > 0)


def test_device_pointers_reuse_and_repeats(xc):
    torch = pytest.importorskip("torch")
    N, B, W = 4096, 4, 300
    iq, _ = rm.synth.make_windows(W, B, N, 10e6, seed=11)
    band = _random_band(np.random.default_rng(3), (W,), N)
    with xc.XcorrEngine(B, N, W) as eng:
        host = eng.correlate(iq, band=band, whiten=True)
        again = eng.correlate(iq, band=band, whiten=True)
        assert all(np.array_equal(u, v) for u, v in zip(host, again))
        d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
        li = torch.zeros((W, 6), dtype=torch.int32, device="cuda")
        lf = torch.zeros((W, 6), dtype=torch.float32, device="cuda")
        pk = torch.zeros((W, 6), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        mine = band.copy()
        eng.correlate_device(d_iq.data_ptr(), W, li.data_ptr(), lf.data_ptr(), pk.data_ptr(), band=mine, whiten=True)
        mine[:] = (0.0, 0.0)                                 # the caller may reuse its array at once
        eng.synchronize()
        dev = (li.cpu().numpy(), lf.cpu().numpy(), pk.cpu().numpy())
    assert all(np.array_equal(u, v) for u, v in zip(host, dev))


def test_argument_errors_name_the_window(xc):
    N, W = 256, 4
    iq, _ = rm.synth.make_windows(W, 3, N, 10e6, seed=1)
    lib = xc.load_library()
    import ctypes as C
    with xc.XcorrEngine(3, N, W) as eng:
        out = [np.zeros((W, 3), t) for t in (np.int32, np.float32, np.float32)]

        def call(band, per_window, weighting=0):
            b = np.ascontiguousarray(band, np.float64)
            return lib.rmx_xcorr_batch_weighted(eng._ctx, iq.ctypes.data_as(C.c_void_p), W, None, 3,
                                                b.ctypes.data_as(C.c_void_p), per_window, weighting, None, 0,
                                                *[o.ctypes.data_as(C.c_void_p) for o in out], 0)
        for bad in ([0.2, 0.1], [-0.6, 0.1], [0.0, 0.7], [np.nan, 0.1], [0.5, 0.5]):
            band = np.tile([[-0.5, 0.5]], (W, 1))
            band[2] = bad
            assert call(band, 1) == -1
            assert "window 2" in lib.rmx_last_error(eng._ctx).decode()
            assert call(bad, 0) == -1
        assert call([-0.1, 0.1], 0, weighting=2) == -1
        assert "weighting" in lib.rmx_last_error(eng._ctx).decode()
        with pytest.raises(xc.RmxError):
            eng.correlate(iq, band=[0.5, 0.5])


def test_seam_band_limit_separates_two_transmitters(xc):
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
    f_strong = fc + 0.10 * fs           # the emitters' centres (STRONG_BAND, WEAK_BAND) and their widths
    f_weak = fc - 0.25 * fs
    t0 = 1_700_000_000_000_000_000

    def run(band_limit):
        """the processor's measurements per frequency group, each solved with the batched solver (scipy's BFGS stops on
        "precision loss" for four buoys in one plane) and judged in the local horizontal plane (the height is free)"""
        p = tp.TDoAProcessor(band_limit=band_limit)
        for bid, la, lo in buoys:
            p.register_buoy(tp.BuoyPosition(bid, la, lo, 0.0, timing_accuracy_ns=20))
        groups = {}
        p.hyperbolic_positioner.triangulate_position = lambda meas, pos: groups.__setitem__(meas[0].frequency_mhz, meas)
        dets = []
        for f in (f_strong, f_weak):
            dets += [tp.SignalDetection(bid, f / 1e6, -60.0, "t", t0, la, lo, 0.9, iq_samples=iq[0, b], sample_rate_hz=fs,
                                        center_freq_hz=fc, bandwidth_hz=0.1 * fs)
                     for b, (bid, la, lo) in enumerate(buoys)]
        p.process_signal_detections(dets)
        out = {}
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
            out[k] = float(np.linalg.norm(err - np.dot(err, up) * up))
        return out

    fixes = run(True)
    assert set(fixes) == {"strong", "weak"}
    assert fixes["strong"] < 1000 and fixes["weak"] < 1000, fixes
    plain = run(False)
    assert plain["weak"] > 5000, plain      # without a band the weak group gets the strong emitter's lags
