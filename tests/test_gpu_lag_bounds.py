"""rmx_xcorr_batch_bounded on the GPU: the peak search restricted to a caller-given lag window per (window, pair),
against the sliced reference (tests/lag_bounds_ref.py), on every route that the dispatcher can take."""
import math
import zlib

import numpy as np
import pytest

import radio_mapper_amd as rm
from conftest import near_tie_windows
from lag_bounds_ref import bounded_batch, full_magnitude

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


def _windows(W, B, N, seed):
    iq, _ = rm.synth.make_windows(W, B, N, 10e6, seed=seed)
    return iq


def _random_bounds(rng, shape, N):
    a = rng.integers(-(N - 1), N, size=shape + (2,))
    lo, hi = np.minimum(a[..., 0], a[..., 1]), np.maximum(a[..., 0], a[..., 1])
    return np.stack([lo, hi], -1).astype(np.int32)


def _assert_sliced(li, lf, pk, ref):
    ri, rf, rp, mg, fm = ref
    ok = mg > TOL                                      # the parity rule: bit-exact where the slice's top two differ
    assert np.array_equal(li[ok], ri[ok]), "integer lags differ from the sliced reference: %d" % int((li != ri)[ok].sum())
    got, want = li[ok] + lf[ok].astype(np.float64), ri[ok] + rf[ok]
    assert np.all(np.abs(got - want) <= TOL * np.maximum(np.abs(want), 1.0)), np.abs(got - want).max()
    # a slice far from the window's peak holds small values; a float32 FFT's error scales with the whole vector
    assert np.all(np.abs(pk[ok] - rp[ok]) <= 1e-5 * rp[ok] + 1e-6 * fm[ok])


@pytest.mark.parametrize("N", [16, 256, 1024, 4096, 8192, 16384, 1 << 18])
def test_full_interval_equals_unbounded_bit_for_bit(xc, N):
    W = 3 if N >= 1 << 18 else 6
    iq, _, raw = rm.synth.make_windows(W, 3, N, 10e6, seed=N, return_u8=True)
    full = np.tile(np.array([[-(N - 1), N - 1]], np.int32), (3, 1))
    with xc.XcorrEngine(3, N, W) as eng:
        for x in (iq, raw):
            a = eng.correlate(x)
            b = eng.correlate(x, lag_bounds=full)
            c = eng.correlate(x, lag_bounds=np.broadcast_to(full, (W, 3, 2)).copy())
            for u, v, w in zip(a, b, c):
                assert np.array_equal(u, v) and np.array_equal(u, w)
            if N in (256, 1024):
                continue   # (these batches run g_win_fused unbounded, which a bounded call avoids)
            # the bounded kernels themselves: pair 0 one lag short of the full interval, pairs 1, 2 full -> unchanged
            near = full.copy()
            near[0, 1] = N - 2
            d = eng.correlate(x, lag_bounds=near)
            for u, v in zip(a, d):
                assert np.array_equal(u[:, 1:], v[:, 1:])


# (route name, N, buoys, windows, default options, custom pair list)
ROUTES = [
    ("k_win", 4096, 8, 300, {}, None),
    ("k_win pipelined >512 host windows", 4096, 4, 600, {"small4096": 0}, None),
    ("small4096", 4096, 8, 8, {}, None),
    ("k_pair fused=0 custom pairs", 4096, 5, 12, {"fused": 0}, [(3, 1), (0, 4), (2, 2), (4, 0)]),
    ("k_win8kl", 8192, 4, 40, {"wscr": 2}, None),
    ("k_win8kl + four-step tail", 8192, 8, 300, {}, None),
    ("k16_pairs", 16384, 3, 24, {"kwin16k": 2}, None),
    ("wscr steered (N=1024)", 1024, 3, 40, {"wscr": 2}, None),
    ("g_win_eo15 steered (N=16384)", 16384, 3, 12, {"wscr": 2, "kwin16k": 0}, None),
    ("four-step", 1 << 17, 3, 4, {}, None),
]


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_parity_on_random_intervals(xc, opts, route):
    name, N, B, W, o, pairs = route
    for k, v in o.items():
        opts(k, v)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    iq = _windows(W, B, N, seed=len(name))
    P = B * (B - 1) // 2 if pairs is None else len(pairs)
    lbw = _random_bounds(rng, (W, P), N)
    lbs = _random_bounds(rng, (P,), N)
    with xc.XcorrEngine(B, N, W) as eng:
        if N == 8192 and W == 300:
            eng.set_option("timing", 1)
        for lb in (lbw, lbs):
            li, lf, pk = eng.correlate(iq, pairs, lag_bounds=lb)
            assert np.all((li >= lb[..., 0]) & (li <= lb[..., 1]))
            _assert_sliced(li, lf, pk, bounded_batch(iq, lb, pairs))


def test_small_chunks_and_device_output(xc):
    torch = pytest.importorskip("torch")
    N, B, W = 4096, 4, 300
    iq = _windows(W, B, N, seed=11)
    lb = _random_bounds(np.random.default_rng(5), (W, 6), N)
    ref = bounded_batch(iq, lb)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("chunk_windows", 64)
        _assert_sliced(*eng.correlate(iq, lag_bounds=lb), ref)
    with xc.XcorrEngine(B, N, W) as eng:
        d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
        li = torch.zeros((W, 6), dtype=torch.int32, device="cuda")
        lf = torch.zeros((W, 6), dtype=torch.float32, device="cuda")
        pk = torch.zeros((W, 6), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        mine = lb.copy()
        eng.correlate_device(d_iq.data_ptr(), W, li.data_ptr(), lf.data_ptr(), pk.data_ptr(), lag_bounds=mine)
        mine[:] = 0                                        # the caller may reuse its array at once
        eng.synchronize()
        _assert_sliced(li.cpu().numpy(), lf.cpu().numpy(), pk.cpu().numpy(), ref)


@pytest.mark.parametrize("N,W,o", [(4096, 8, {}), (4096, 300, {}), (8192, 40, {"wscr": 2}), (16384, 12, {"kwin16k": 2}),
                                   (1 << 17, 2, {})])
def test_edge_cases(xc, opts, N, W, o):
    for k, v in o.items():
        opts(k, v)
    B = 3
    iq = _windows(W, B, N, seed=3)
    m = full_magnitude(iq[0, 0], iq[0, 1])
    k = int(np.argmax(m))
    lag_true = k - (N - 1)
    lb = np.zeros((W, 3, 2), np.int32)
    lb[..., 0], lb[..., 1] = -(N - 1), N - 1
    lb[0, 0] = (lag_true + 1, lag_true + 40) if lag_true + 40 <= N - 1 else (lag_true - 40, lag_true - 1)   # edge beside the peak
    lb[0, 1] = (5, 5)                                                                                       # lo == hi
    lb[0, 2] = (N - 20, N - 1)                                                                              # ends at N-1
    if W > 1:
        lb[1, 0] = (-(N - 1), -(N - 30))                                                                    # starts at -(N-1)
    zero = iq.copy()
    zero[W - 1] = 0                                                                                         # all-zero window
    lb[W - 1, 1] = (-7, 9)
    with xc.XcorrEngine(B, N, W) as eng:
        li, lf, pk = eng.correlate(zero, lag_bounds=lb)
    edge = lb[0, 0, 0] if lag_true < lb[0, 0, 0] else lb[0, 0, 1]
    assert li[0, 0] == edge and lf[0, 0] == 0.0
    assert li[0, 1] == 5 and lf[0, 1] == 0.0
    assert li[W - 1, 1] == -7 and lf[W - 1, 1] == 0.0 and pk[W - 1, 1] == 0.0
    _assert_sliced(li, lf, pk, bounded_batch(zero, lb))


def test_near_ties_inside_the_interval(xc):
    N = 4096
    e = near_tie_windows(N, 9)
    W = e.shape[0]
    lbs = []
    for w in range(W):
        m = full_magnitude(e[w, 0], e[w, 1])
        top = np.argsort(m)[-2:] - (N - 1)
        lbs.append([[int(top.min()) - 3, int(top.max()) + 3]])
    lb = np.asarray(lbs, np.int32)
    with xc.XcorrEngine(2, N, W) as eng:
        li, lf, pk = eng.correlate(e, lag_bounds=lb)
        ui, uf, up = eng.correlate(e)
    # both peaks lie inside: the bounded search agrees with the unbounded one, whichever candidate that picked
    assert np.array_equal(li, ui) and np.array_equal(lf, uf) and np.array_equal(pk, up)


def _decoy_scene(N, d, echo, gain, seed, noise=0.05):
    """windows x_b[n] = s[n - d_b] (+ gain * s[n - d_b - echo] on buoys listed in echo) + noise"""
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal(4 * N) + 1j * rng.standard_normal(4 * N)).astype(np.complex64) * 30
    base = 2 * N
    out = np.zeros((len(d), N), np.complex64)
    for b, db in enumerate(d):
        out[b] = s[base - db:base - db + N]
        if b in echo:
            out[b] += gain * s[base - db - echo[b]:base - db - echo[b] + N]
        out[b] += (noise * 30 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))).astype(np.complex64)
    return out


@pytest.mark.parametrize("N,W,o", [(4096, 1, {}), (4096, 300, {}), (8192, 40, {"wscr": 2}), (16384, 12, {"kwin16k": 2})])
def test_decoy_outside_the_physical_interval(xc, opts, N, W, o):
    """A delayed echo stronger than the direct path, outside the physical interval: the unbounded call returns the
    decoy, the bounded one the true lag (and matches the sliced reference)."""
    for k, v in o.items():
        opts(k, v)
    d = [0, 17, 120]
    iq = np.stack([_decoy_scene(N, d, {2: 1500}, 2.0, seed=w) for w in range(W)])
    lb = np.array([[-200, 200]] * 3, np.int32)
    with xc.XcorrEngine(3, N, W) as eng:
        ui, _, _ = eng.correlate(iq)
        li, lf, pk = eng.correlate(iq, lag_bounds=lb)
    # pairs (0,1), (0,2), (1,2): true lags d_j - d_i
    assert np.all(ui[:, 1] == 1500 + 120) and np.all(ui[:, 2] == 1500 + 103)   # the decoy bites without bounds
    assert np.all(li[:, 0] == 17) and np.all(li[:, 1] == 120) and np.all(li[:, 2] == 103)
    _assert_sliced(li, lf, pk, bounded_batch(iq, lb))


def test_seam_bound_lags_removes_the_decoy(xc):
    from radio_mapper_amd import tdoa_processor as tp
    fs, N = 10e6, 4096
    lat0, lng0 = 37.0, -122.0
    buoys = [("B0", lat0, lng0), ("B1", lat0 + 0.03, lng0), ("B2", lat0, lng0 + 0.04), ("B3", lat0 + 0.03, lng0 + 0.04)]
    emitter = tp.GeodeticCalculator.lat_lng_to_xyz(lat0 + 0.012, lng0 + 0.015, 0.0)
    xyz = [tp.GeodeticCalculator.lat_lng_to_xyz(la, lo, 0.0) for _, la, lo in buoys]
    d = [int(round(math.dist(emitter, x) / tp.TDoACalculator.SPEED_OF_LIGHT * fs)) for x in xyz]
    dmin = min(d)
    d = [v - dmin for v in d]
    win = _decoy_scene(N, d, {3: 2200}, 4.0, seed=4)
    t0 = 1_700_000_000_000_000_000

    def run(bound):
        p = tp.TDoAProcessor()
        for (bid, la, lo) in buoys:
            p.register_buoy(tp.BuoyPosition(bid, la, lo, 0.0, timing_accuracy_ns=20))
        p.tdoa_calculator.bound_lags = bound
        dets = [tp.SignalDetection(bid, 121.5, -60.0, "t", t0, la, lo, 0.9, iq_samples=win[b], sample_rate_hz=fs)
                for b, (bid, la, lo) in enumerate(buoys)]
        meas = p.tdoa_calculator.calculate_tdoa_measurements(dets, p.buoy_positions)
        return meas, None

    true = {(buoys[i][0], buoys[j][0]): (d[j] - d[i]) / fs * 1e9 for i in range(4) for j in range(i + 1, 4)}
    meas, fixes = run(True)
    assert len(meas) == 6
    for m in meas:
        assert abs(m.time_difference_ns - true[(m.buoy1_id, m.buoy2_id)]) <= 1e9 / fs, (m, true)
    # the fix from these measurements (the batched solver: scipy's BFGS stops on "precision loss" for four buoys in one
    # plane, with or without bounds)
    lag = np.array([[m.time_difference_ns * 1e-9 * fs for m in meas]])
    li = np.rint(lag).astype(np.int32)
    with xc.XcorrEngine(4, N, 1) as eng:
        pos, _, _ = eng.solve(np.array(xyz), li, (lag - li).astype(np.float32), fs)
    # four buoys in one plane leave the height free (the solve settles about 2 km below the emitter): the fix is judged
    # in the local horizontal plane
    up = np.asarray(emitter) / np.linalg.norm(emitter)
    err = pos[0] - np.asarray(emitter)
    assert np.linalg.norm(err - np.dot(err, up) * up) < 500.0, (pos, emitter)
    meas_u, _ = run(False)
    wrong = [m for m in meas_u if abs(m.time_difference_ns - true[(m.buoy1_id, m.buoy2_id)]) > 1e9 / fs]
    assert wrong and all("B3" in (m.buoy1_id, m.buoy2_id) for m in wrong)
