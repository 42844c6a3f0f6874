"""rmx_xcorr_batch_integrated on the GPU: noncoherent integration over groups of K consecutive windows against the float32
reference (tests/integrated_ref.py) on every route, K = 1 as the weighted call, copies and reversed groups, repeatability,
the two frequency-offset scenarios, the seam end to end, MultiXcorrEngine, and argument errors through the raw ABI.
The parity rule is the header's (that of tests/test_gpu_weighted.py), computed on the integrated vector."""
import ctypes as C
import zlib

import numpy as np
import pytest

import radio_mapper_amd as rm
import integrated_ref as ir
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


def _ref(iq, K, *a, **k):
    return ir.integrated_batch(iq, K, *a, with_bound=True, **k)


def _assert_parity(li, lf, pk, ref, what=""):
    """the parity rule of include/rmx.h on the integrated vector m: lag_int bit-exact where the reference's top-two margin
    inside the searched slice exceeds 1e-5; lag_frac within 1e-5 * max(|lag|, 1), or within four one-ulp bounds of the
    reference's own taps (a flat peak); peak within 1e-5 relative + 1e-6 of the vector's maximum.  A slice whose peak lies
    below 1e-5 of the whole vector's maximum holds only the float32 transforms' rounding noise: peak is checked there,
    lags are not (PHAT on a self pair with a lag window that excludes 0: r is a unit impulse at lag 0).  The pair-groups
    the margin excludes stay under 1 % of the test's."""
    ri, rf, rp, mg, fm, fb = ref
    assert li.shape == ri.shape, (li.shape, ri.shape)
    ok = (mg > TOL) & (rp > 1e-5 * fm)
    close = mg <= TOL
    dpk = np.abs(pk - rp) / (1e-5 * rp + 1e-6 * fm)
    got, want = li + lf.astype(np.float64), ri + rf
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    print("%s: %d pair-groups, %d noise slices, %d excluded by the margin, lag_int differs in %d, worst lag error %.2e, worst peak error %.2f of its bound"
          % (what, ok.size, int((rp <= 1e-5 * fm).sum()), int(close.sum()), int((li != ri)[ok].sum()), float(rel[ok].max()) if ok.any() else 0.0,
             float(dpk.max())))
    assert close.sum() <= 0.01 * ok.size, "the margin excludes %d of %d pair-groups" % (int(close.sum()), ok.size)
    assert np.array_equal(li[ok], ri[ok]), "integer lags differ from the reference: %d" % int((li != ri)[ok].sum())
    assert np.all((rel[ok] <= TOL) | (rel[ok] <= 4.0 * fb[ok])), (rel[ok].max(), fb[ok][np.argmax(rel[ok])])
    assert np.all(np.abs(pk - rp) <= 1e-5 * rp + 1e-6 * fm), dpk.max()


def _random_band(rng, shape, N):
    a = rng.uniform(-0.5, 0.5, size=shape + (2,))
    lo, hi = a.min(-1), a.max(-1)
    lo = np.minimum(lo, 0.5 - 2.0 / (2 * N))
    return np.stack([lo, np.maximum(hi, lo + 2.0 / (2 * N))], -1)


def _random_bounds(rng, shape, N):
    a = rng.integers(-(N - 1), N, size=shape + (2,))
    return np.stack([a.min(-1), a.max(-1)], -1).astype(np.int32)


# (route name, N, buoys, K, groups, default options, engine options, custom pair list, expected forward family)
ROUTES = [
    ("k_pair 1 group K=64", 4096, 8, 64, 1, {}, {}, None, "k_fwd"),
    ("k_pair 24 groups K=16", 4096, 4, 16, 24, {}, {}, None, "k_fwd"),
    ("k_pair chunked K=3", 4096, 3, 3, 50, {}, {"chunk_windows": 16}, None, "k_fwd"),        # 15 windows a chunk
    ("k_pair custom pairs K=2", 4096, 5, 2, 6, {}, {}, [(3, 1), (0, 4), (2, 2), (4, 0)], "k_fwd"),
    ("g_pair_small N=16 K=3", 16, 3, 3, 14, {}, {}, None, "g_fwd_small"),
    ("g_pair_small N=256 K=64", 256, 4, 64, 6, {}, {}, None, "g_fwd_small"),
    ("g_pair_small N=2048 K=16", 2048, 8, 16, 5, {}, {}, None, "g_fwd_small"),
    ("g_pair_small generic4096 K=2", 4096, 3, 2, 10, {"generic4096": 1}, {}, None, "g_fwd_small"),
    ("g_pair_small chunked K=2", 256, 3, 2, 9, {"gen_chunk": 5}, {}, [(2, 0), (1, 1), (0, 1)], "g_fwd_small"),  # 4 windows a chunk
    ("four-step N=8192 3 buoys K=16", 8192, 3, 16, 3, {}, {}, None, "g_rows_fwd"),
    ("four-step N=8192 8 buoys K=2", 8192, 8, 2, 8, {}, {}, None, "g_rows_fwd"),
    ("four-step N=16384 3 buoys K=64", 16384, 3, 64, 1, {}, {}, None, "g_rows_fwd"),
    ("four-step N=16384 8 buoys K=3", 16384, 8, 3, 2, {}, {}, None, "g_rows_fwd"),
    ("four-step N=16384 chunked K=2", 16384, 3, 2, 5, {"gen_chunk": 5}, {}, [(2, 1), (0, 0), (0, 2)], "g_rows_fwd"),
    ("four-step N=65536 3 buoys K=2", 65536, 3, 2, 2, {}, {}, None, "g_rows_fwd"),
]
FORBIDDEN = ("g_win_*", "g_rows_fused", "k16_fwd", "k16_pairs")


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_against_the_reference(xc, opts, route):
    name, N, B, K, G, dopt, eopt, pairs, fwd = route
    for k, v in dopt.items():
        opts(k, v)
    W = K * G
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    iq, _, raw = rm.synth.make_windows(W, B, N, 10e6, seed=len(name), return_u8=True)
    P = B * (B - 1) // 2 if pairs is None else len(pairs)
    shared_band = _random_band(rng, (), N)
    per_win = _random_band(rng, (W,), N)
    per_win[0] = (-0.5, 0.5)
    lb_shared = _random_bounds(rng, (P,), N)
    lb_group = _random_bounds(rng, (G, P), N)
    cases = [(None, False, None), (per_win, True, None), (None, False, lb_shared), (shared_band, True, lb_group)]
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        eng.set_option("timing", 1)
        for band, phat, bounds in cases:
            li, lf, pk = eng.correlate(iq, pairs, lag_bounds=bounds, band=band, whiten=phat, integrate=K)
            tk = eng.last_timing_by_kernel()
            fams = set(tk)
            assert fwd in fams and not (fams & set(FORBIDDEN)), fams
            if fwd == "k_fwd":   # k_win and k_pair share one timing family: one pair launch per k_fwd launch = no k_win
                assert tk["k_win|k_pair"]["launches"] == tk["k_fwd"]["launches"], tk
            else:
                assert ("g_pair_small" in fams) != ("g_cols_inv" in fams), fams
            _assert_parity(li, lf, pk, _ref(iq, K, band, phat, bounds, pairs), name)
            li8, lf8, pk8 = eng.correlate(raw, pairs, lag_bounds=bounds, band=band, whiten=phat, integrate=K)
            assert np.array_equal(li, li8) and np.array_equal(lf, lf8) and np.array_equal(pk, pk8)


ONE_PER_ROUTE = [("k_pair", 4096, {}), ("g_pair_small", 256, {}), ("g_pair_small 4096", 4096, {"generic4096": 1}),
                 ("four-step 8192", 8192, {}), ("four-step 16384", 16384, {})]


@pytest.mark.parametrize("route", ONE_PER_ROUTE, ids=[r[0] for r in ONE_PER_ROUTE])
def test_k1_is_the_weighted_call_bit_for_bit(xc, opts, route):
    name, N, dopt = route
    for k, v in dopt.items():
        opts(k, v)
    W, B = 6, 3
    rng = np.random.default_rng(N)
    iq, _ = rm.synth.make_windows(W, B, N, 10e6, seed=N)
    band = _random_band(rng, (W,), N)
    lb = _random_bounds(rng, (W, 3), N)
    lib = xc.load_library()
    with xc.XcorrEngine(B, N, W) as eng:
        for kw in ({}, {"band": band, "whiten": True}, {"lag_bounds": lb}, {"band": band, "whiten": True, "lag_bounds": lb}):
            a = eng.correlate(iq, **kw)
            b = eng.correlate(iq, integrate=1, **kw)
            out = [np.zeros((W, 3), t) for t in (np.int32, np.float32, np.float32)]
            bd = kw.get("band")
            bounds = kw.get("lag_bounds")
            rc = lib.rmx_xcorr_batch_integrated(
                eng._ctx, iq.ctypes.data_as(C.c_void_p), W, None, 3, 1,
                None if bd is None else bd.ctypes.data_as(C.c_void_p), 1, 1 if kw.get("whiten") else 0,
                None if bounds is None else bounds.ctypes.data_as(C.c_void_p), 1,
                *[o.ctypes.data_as(C.c_void_p) for o in out], 0)
            assert rc == 0
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
            assert all(np.array_equal(u, v) for u, v in zip(a, out))


@pytest.mark.parametrize("N,K", [(4096, 4), (4096, 16), (256, 16), (8192, 4)])
def test_copies_of_one_window(xc, N, K):
    """K copies of one window: the lags of the plain result of that window, sqrt(K) times its peak (not bit-exact: the
    in-order float32 sum x + x + x rounds)"""
    B = 4
    one, _ = rm.synth.make_windows(1, B, N, 10e6, seed=K)
    ref = wr.weighted_batch(one, with_bound=True)
    r = np.sqrt(np.float64(K))
    scaled = (ref[0], ref[1], ref[2] * r, ref[3], ref[4] * r, ref[5])
    with xc.XcorrEngine(B, N, K) as eng:
        li, lf, pk = eng.correlate(np.repeat(one, K, axis=0), integrate=K)
        pi, pf, pp = eng.correlate(one)
    _assert_parity(li, lf, pk, scaled, "copies")
    assert np.array_equal(li, pi)
    assert np.all(np.abs(pk - r * pp) <= 1e-5 * r * pp)


@pytest.mark.parametrize("N,K,G", [(4096, 16, 3), (2048, 3, 4), (8192, 4, 2)])
def test_reversed_groups_and_repeated_calls(xc, N, K, G):
    torch = pytest.importorskip("torch")
    B, P = 3, 3
    W = K * G
    rng = np.random.default_rng(N + K)
    iq, _ = rm.synth.make_windows(W, B, N, 10e6, seed=K)
    band = _random_band(rng, (W,), N)
    lb = _random_bounds(rng, (G, P), N)
    rev = iq.reshape(G, K, B, N)[:, ::-1].reshape(W, B, N).copy()
    rband = band.reshape(G, K, 2)[:, ::-1].reshape(W, 2).copy()
    ref = _ref(iq, K, band, True, lb)
    with xc.XcorrEngine(B, N, W) as eng:
        a = eng.correlate(iq, band=band, whiten=True, lag_bounds=lb, integrate=K)
        b = eng.correlate(iq, band=band, whiten=True, lag_bounds=lb, integrate=K)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))          # order of the additions is fixed: bit-identical
        _assert_parity(*a, ref, "forward")
        r = eng.correlate(rev, band=rband, whiten=True, lag_bounds=lb, integrate=K)
        _assert_parity(*r, ref, "reversed")                              # order matters only through rounding
        d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
        li = torch.zeros((G, P), dtype=torch.int32, device="cuda")
        lf = torch.zeros((G, P), dtype=torch.float32, device="cuda")
        pk = torch.zeros((G, P), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        mine = lb.copy()
        eng.correlate_device(d_iq.data_ptr(), W, li.data_ptr(), lf.data_ptr(), pk.data_ptr(), band=band, whiten=True,
                             lag_bounds=mine, integrate=K)
        mine[:] = 0                                                       # the caller may reuse its array at once
        eng.synchronize()
        dev = (li.cpu().numpy(), lf.cpu().numpy(), pk.cpu().numpy())
    assert all(np.array_equal(u, v) for u, v in zip(a, dev))


SCENES = [("64 x 1024 at -14 dB", 65536, 64, -14.0), ("16 x 1024 at 0 dB", 16384, 16, 0.0)]


@pytest.mark.parametrize("scene", SCENES, ids=[s[0] for s in SCENES])
def test_offset_scenarios(xc, scene):
    """frequency offsets of (0, 3, 8) cycles over the capture, 20 seeds x 3 pairs: the integrated lags are all correct, the
    plain correlation of the full-length window is wrong for at least 57 of 60"""
    _, n, K, snr = scene
    xs = [ir.offset_scene(n, seed, snr) for seed in range(20)]
    full = np.stack(xs)
    seg = np.concatenate([ir.segments(x, K) for x in xs])
    with xc.XcorrEngine(3, n // K, 20 * K) as eng:
        li, lf, pk = eng.correlate(seg, integrate=K)
    with xc.XcorrEngine(3, n, 20) as eng:
        ci, _, _ = eng.correlate(full)
    good, wrong = int((li == ir.TRUE_LAGS).sum()), int((ci != ir.TRUE_LAGS).sum())
    print("integrated correct %d / 60, coherent wrong %d / 60" % (good, wrong))
    assert li.shape == (20, 3) and good == 60
    assert wrong >= 57
    _assert_parity(li, lf, pk, _ref(seg, K), "scenario")


def test_seam_integrate_recovers_the_time_differences(xc):
    from radio_mapper_amd import tdoa_processor as tp
    fs, n, K = 2.048e6, 16384, 16
    x = ir.offset_scene(n, 4, 0.0)
    buoys = {"A": tp.BuoyPosition("A", 37.0, -122.0, 0.0, 100), "B": tp.BuoyPosition("B", 37.0, -121.9, 0.0, 200),
             "C": tp.BuoyPosition("C", 37.2, -122.0, 0.0, 50)}
    dets = [tp.SignalDetection(b, 121.5, -60.0, "t", 1_700_000_000_000_000_000, 0, 0, 0.9, iq_samples=x[k], sample_rate_hz=fs)
            for k, b in enumerate("ABC")]
    want_ns = ir.TRUE_LAGS / fs * 1e9
    calc = tp.TDoACalculator(integrate=K)
    try:
        meas = calc.calculate_tdoa_measurements(dets, buoys)
    finally:
        calc.close()
    assert [(m.buoy1_id, m.buoy2_id) for m in meas] == [("A", "B"), ("A", "C"), ("B", "C")]
    err = np.array([m.time_difference_ns for m in meas]) - want_ns
    assert np.all(np.abs(err) <= 1e9 / fs), err
    plain = tp.TDoACalculator()
    try:
        meas1 = plain.calculate_tdoa_measurements(dets, buoys)
    finally:
        plain.close()
    miss = np.abs(np.array([m.time_difference_ns for m in meas1]) - want_ns) > 1e9 / fs
    assert len(meas1) == 3 and miss.sum() >= 2, miss


def test_multi_engine_equals_the_single_engine(xc):
    from radio_mapper_amd import multi
    N, B, K, G = 256, 4, 4, 5                     # 5 groups over two contexts: 3 + 2
    W = K * G
    rng = np.random.default_rng(5)
    iq, _ = rm.synth.make_windows(W, B, N, 10e6, seed=5)
    band = _random_band(rng, (W,), N)
    lb = _random_bounds(rng, (G, 6), N)
    with xc.XcorrEngine(B, N, W) as eng:
        one = eng.correlate(iq, band=band, whiten=True, lag_bounds=lb, integrate=K)
        plain = eng.correlate(iq, integrate=K)
    with multi.MultiXcorrEngine(B, N, W, devices=[0, 0]) as m:
        two = m.correlate(iq, band=band, whiten=True, lag_bounds=lb, integrate=K)
        plain2 = m.correlate(iq, integrate=K)
    assert one[0].shape == (G, 6)
    assert all(np.array_equal(u, v) for u, v in zip(one, two))
    assert all(np.array_equal(u, v) for u, v in zip(plain, plain2))


def test_argument_errors_through_the_raw_abi(xc, opts):
    lib = xc.load_library()

    def run(eng, iq, W, K, bounds=None, per_group=0, P=3):
        out = [np.zeros((max(W, 1), P), t) for t in (np.int32, np.float32, np.float32)]
        rc = lib.rmx_xcorr_batch_integrated(eng._ctx, iq.ctypes.data_as(C.c_void_p), W, None, P, K, None, 0, 0,
                                            None if bounds is None else bounds.ctypes.data_as(C.c_void_p), per_group,
                                            *[o.ctypes.data_as(C.c_void_p) for o in out], 0)
        return rc, lib.rmx_last_error(eng._ctx).decode()

    for N in (256, 4096, 8192):
        W = 16
        iq, _ = rm.synth.make_windows(W, 3, N, 10e6, seed=1)
        with xc.XcorrEngine(3, N, W) as eng:
            rc, msg = run(eng, iq, W, 0)
            assert rc == -1 and "integrate = 0" in msg
            rc, msg = run(eng, iq, W, -2)
            assert rc == -1 and "integrate = -2" in msg
            rc, msg = run(eng, iq, W - 1, 4)
            assert rc == -1 and "15" in msg and "4" in msg and "multiple" in msg
            rc, msg = run(eng, iq, 0, 4)
            assert rc == -1 and "multiple" in msg
            rc, msg = run(eng, iq, 2 * W, 4)
            assert rc == -1 and "max_windows" in msg
            lb = np.tile(np.array([[-(N - 1), N - 1]], np.int32), (4, 3, 1))
            lb[2, 1] = (-N, 3)
            rc, msg = run(eng, iq, W, 4, lb, 1)
            assert rc == -1 and "group 2, pair 1" in msg
            lb[2, 1] = (5, 4)
            rc, msg = run(eng, iq, W, 4, lb, 1)
            assert rc == -1 and "group 2, pair 1" in msg
            rc, _ = run(eng, iq, W, 4)
            assert rc == 0
    # K over the chunk capacity: refused with a text that says so, never split
    iq, _ = rm.synth.make_windows(16, 3, 4096, 10e6, seed=1)
    with xc.XcorrEngine(3, 4096, 16) as eng:
        eng.set_option("chunk_windows", 8)
        rc, msg = run(eng, iq, 16, 16)
        assert rc == -1 and "chunk" in msg and "16" in msg
        rc, _ = run(eng, iq, 16, 8)
        assert rc == 0
    for N in (256, 8192):
        opts("gen_chunk", 2)
        iq, _ = rm.synth.make_windows(8, 3, N, 10e6, seed=1)
        with xc.XcorrEngine(3, N, 8) as eng:
            rc, msg = run(eng, iq, 8, 4)
            assert rc == -1 and "chunk" in msg and "4" in msg
            rc, _ = run(eng, iq, 8, 2)
            assert rc == 0
    with xc.XcorrEngine(3, 256, 8) as eng:
        with pytest.raises(xc.RmxError):
            eng.correlate(np.zeros((8, 3, 256), np.complex64), integrate=4, lag_bounds=np.full((3, 2), 256, np.int32))


@pytest.mark.parametrize("N", [256, 4096, 8192])
def test_no_call_leaves_anything_behind_for_the_next(xc, N):
    """A call's bounds, weighting and K are arguments of that call alone: after two refused calls (an integrated one whose
    band and K are fine and whose lag interval is not; a weighted one whose second band is not) and a successful band + PHAT +
    bounds + K = 2 call, the plain call and the Doppler search of the same engine return, bit for bit, what a fresh engine
    returns that never saw the others.  N = 256: the small generic kernels; 4096: the per-transform kernels; 8192: four-step."""
    B, W, P, K = 3, 4, 3, 2
    lib = xc.load_library()
    rng = np.random.default_rng(N)
    iq, _ = rm.synth.make_windows(W, B, N, 10e6, seed=N)
    dops = np.array([0.0, 1.0 / N])
    band = np.array([-0.2, 0.3])
    lb = _random_bounds(rng, (P,), N)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def raw(eng, entry, *args):
        out = [np.zeros((W, P), t) for t in (np.int32, np.float32, np.float32)]
        rc = entry(eng._ctx, vp(iq), W, None, P, *args, *[vp(o) for o in out], 0)
        return rc, lib.rmx_last_error(eng._ctx).decode()

    with xc.XcorrEngine(B, N, W) as fresh:
        want_plain = fresh.correlate(iq)
    with xc.XcorrEngine(B, N, W) as fresh:
        want_caf = fresh.caf(iq, dops)
    with xc.XcorrEngine(B, N, W) as eng:
        bad_lb = lb.copy()
        bad_lb[1] = (7, 6)
        rc, msg = raw(eng, lib.rmx_xcorr_batch_integrated, K, vp(band), 0, 1, vp(bad_lb), 0)
        assert rc == -1 and "lag_bounds of group" in msg and "pair 1" in msg, (rc, msg)   # RMX_E_INVAL; band and K accepted
        bad_band = np.tile(band, (W, 1))
        bad_band[1] = (0.2, 0.1)
        rc, msg = raw(eng, lib.rmx_xcorr_batch_weighted, vp(bad_band), 1, 1, None, 0)
        assert rc == -1 and "band of window 1" in msg, (rc, msg)
        li, lf, pk = eng.correlate(iq, band=band, whiten=True, lag_bounds=lb, integrate=K)
        _assert_parity(li, lf, pk, _ref(iq, K, band, True, lb), "band + PHAT + bounds + K = 2")
        got_plain = eng.correlate(iq)
        got_caf = eng.caf(iq, dops)
    assert all(np.array_equal(u, v) for u, v in zip(got_plain, want_plain))
    assert all(np.array_equal(u, v) for u, v in zip(got_caf, want_caf))
