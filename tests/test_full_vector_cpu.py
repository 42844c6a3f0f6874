"""tests/full_vector_ref.py on the CPU: the float64 vectors against the references they restate, the coverage planners
of tests/test_gpu_every_lag.py and tests/test_gpu_every_bin.py, and the honesty of the bars those two files hold the GPU to
(the float32 oracle must stay far inside them on every lag and every bin)."""
import numpy as np
import pytest
from scipy import fft as sp_fft

import caf_request_ref as rr
import far_lag_ref as F
import full_vector_ref as V
import integrated_ref as ir
import quality_ref as qr
import weighted_ref as wr
from oracle import xcorr_ref as orc


# ---- the vectors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 256, 1024])
def test_full64_is_ref64_at_the_maximum(N):
    for scene in V.SCENES:
        iq = V.scenes(N)[scene][0]
        for w in range(2):
            for i, j in ((0, 1), (1, 0)):
                m = V.full64(iq[w, i], iq[w, j])
                lag, _, peak, _ = F.ref64(iq[w, i], iq[w, j])
                assert m.shape == (2 * N - 1,) and int(np.argmax(m)) - (N - 1) == lag and m.max() == peak
                assert np.array_equal(m, V.vectors(N, scene)[w, 2 * i + j])


def test_the_scenes_are_what_they_say():
    for N in (256, 4096):
        sc = V.scenes(N)
        for name in V.SCENES:
            iq, raw = sc[name]
            assert iq.shape == (2, 2, N) and raw.shape == (2, 2, 2 * N) and raw.dtype == np.uint8
            dec = (raw[..., 0::2].astype(np.float32) - np.float32(127.5)) + 1j * (raw[..., 1::2].astype(np.float32) - np.float32(127.5))
            assert np.array_equal(dec.astype(np.complex64), iq)
            assert not np.array_equal(iq[0], iq[1])
        m = V.vectors(4096, "emitter")[:, 1]
        assert np.all(np.abs(np.argmax(m, axis=-1) - 4095) <= 80)                        # delays inside +-40
        n = V.vectors(4096, "noise")[:, 1]
        ratio = n.max(axis=-1) / np.sqrt((n ** 2).mean(axis=-1))
        assert np.all(ratio > 1.5) and np.all(ratio < 6.0), ratio                        # no peak: the largest of 2N noise values
        assert np.all(m.max(axis=-1) / np.sqrt((m ** 2).mean(axis=-1)) > 20.0)           # the emitter's stands far above them
    t = V.tile(V.scenes(256)["emitter"][0], 5, 3)
    assert t.shape == (5, 3, 256) and np.array_equal(t[3, 2], V.scenes(256)["emitter"][0][1, 0])


@pytest.mark.parametrize("N", [16, 256, 1024])
def test_weighted_integrated_and_derotated_forms_agree_with_their_float32_references(N):
    band = (-0.3, 0.3)
    for scene in V.SCENES:
        iq = V.scenes(N)[scene][0]
        for bd, phat in ((band, True), (band, False), (None, True)):
            got = V.full64(iq[0, 0], iq[0, 1], bd, phat)
            ref = wr.weighted_full(iq[0, 0], iq[0, 1], bd, phat).astype(np.float64)
            assert np.all(np.abs(got - ref) <= V.bar(got, got.max())), (N, scene, bd, phat)
            assert np.array_equal(V.kept(*band, N), wr.mask(*band, N))
        g = V.tile(iq, 3, 2)
        got = V.integrated64(g[:, 0], g[:, 1], band, True)
        ref = ir.integrated_full(g, 0, 1, band, True).astype(np.float64)
        assert np.all(np.abs(got - ref) <= V.bar(got, got.max())), (N, scene)
        m = V.vectors(N, scene, band, True)
        assert np.allclose(got, np.sqrt(2 * m[0, 1] ** 2 + m[1, 1] ** 2), rtol=1e-12, atol=0)
        # the de-rotated buoy: the float32 restatement's per-hypothesis peak inside a one-lag interval
        grid = (np.arange(5) - 2) * (0.5 / N)
        lags = np.array([0, -(N - 1), N // 3])
        lb = np.stack([lags, lags], -1)[:, None, :]
        x = np.repeat(iq[:1], 3, axis=0)
        r = rr.bin_results(x, grid, pairs=[(0, 1)], lag_bounds=lb)
        for d in range(5):
            m_d = V.derotated64(iq[0, 0], iq[0, 1], grid[d])
            want = m_d[lags + N - 1]
            assert np.all(np.abs(r["peak"][:, 0, d] - want) <= V.bar(want, m_d.max())), (N, scene, d)
            assert np.array_equal(r["lag_int"][:, 0, d], lags)


def test_bin_product_is_the_peak_of_a_one_bin_band():
    N = 256
    iq = V.scenes(N)["emitter"][0]
    X = V.spectra64(iq[0])
    for s in (-N, -1, 0, 1, 77, N - 1):
        bd = V.one_bin_bands([s], N)[0]
        m = V.full64(iq[0, 0], iq[0, 1], bd)
        assert np.allclose(m, V.bin_product(X[0], X[1], s), rtol=1e-10, atol=0)          # flat: the same at every lag
        m = V.full64(iq[0, 0], iq[0, 1], bd, True)
        assert np.allclose(m, 1.0 / (2 * N), rtol=1e-10, atol=0)
        assert V.kept(bd[0], bd[1], N).sum() == 1 and V.kept(bd[0], bd[1], N)[s % (2 * N)]


# ---- the planners ---------------------------------------------------------------------------------------------------
def _every(N):
    return set(range(-(N - 1), N))


def test_lag_plans_of_the_gpu_routes_hold_what_they_claim():
    """every row of test_gpu_every_lag.ROUTES and LAYOUTS: exhaustive plans hold every lag under (0, 1) and the mirror set
    under (1, 0); sampled ones the seams under both orders and the seeded lags; the slot budgets are those of the table"""
    import test_gpu_every_lag as T
    rows = [(r[0], r[1], r[2], r[3], r[4], r[5], r[9]) for r in T.ROUTES]
    rows += [("layout " + l[0], l[1], 2, l[2], l[3], l[4], l[6]) for l in T.LAYOUTS]
    for name, N, B, W, custom, per_window, exhaustive in rows:
        pl, pairs, lags, kinds = T.plan_of(N, B, W, custom, per_window, exhaustive)
        assert lags.shape == ((W if per_window else 1), len(pl)) and np.all(np.abs(lags) <= N - 1), name
        if "k_win8kl" in name or "k16" in name:
            assert len(pl) <= 640, name                      # the kernels' LDS copy of the pair list (max_pairs8, max_pairs16)
        first = set(lags.ravel()[kinds == V.ORDER01].tolist())
        second = set(lags.ravel()[kinds == V.MIRROR10].tolist())
        seam = set(V.seams(N))
        assert seam <= first and seam <= second, name
        assert {-(N - 1), -(N - 2), N - 2, N - 1} <= first & second, name
        if exhaustive:
            assert first == _every(N), name
            assert set(V.mirror_lags(N).tolist()) <= second
            assert all({l - 1, l + 1} & _every(N) <= second for l in seam), name
        else:
            assert {0, 1, -1} <= first & second and set(V.seeded_lags(N).tolist()) <= set(lags.ravel().tolist()), name
            assert len(set(V.seeded_lags(N).tolist())) > 1900
        assert lags.size <= 36000, (name, lags.size)


def test_every_seam_of_every_stride_is_in_the_seam_list():
    for N, strides in F.STRIDES.items():
        s = set(V.seams(N))
        for st in strides:
            if F.top_lag(N) // st >= 1:
                assert {st, st - 1, -st, -st + 1} <= s, (N, st)
    assert V.seams(16) == [] and set(V.mirror_lags(16).tolist()) == _every(16)


def test_lag_plan_refuses_too_few_slots():
    with pytest.raises(ValueError):
        V.lag_plan(256, V.kinds_of(V.pair_list(64, 2), 2), True)
    with pytest.raises(ValueError):
        V.lag_plan(8192, V.kinds_of(V.pair_list(640, 2), 3), False)


def test_bin_plans_hold_what_they_claim():
    for N in (16, 256, 4096):
        assert np.array_equal(V.bin_plan(N, True), np.arange(-N, N))
    for N, L1 in ((8192, V.default_l1(8192)), (65536, V.default_l1(65536))):
        assert (N, L1) in ((8192, 32), (65536, 128))
        L = 2 * N
        b = set(V.bin_plan(N, False, ("rows", L1)).tolist())
        assert {-N, -1, 0, 1, N - 1} <= b and min(b) >= -N and max(b) <= N - 1
        k = 1
        while (1 << k) <= N:
            want = {(1 << k) - 1, (1 << k) + 1, -(1 << k) - 1, -(1 << k) + 1}
            assert {s for s in want if -N <= s <= N - 1} <= b
            k += 1
        nat = {s % L for s in b}
        k1_of = lambda fixed: {k % L1 for k in nat if k // L1 == fixed}      # noqa: E731
        k2_of = lambda fixed: {k // L1 for k in nat if k % L1 == fixed}      # noqa: E731
        assert sum(k1_of(f) == set(range(L1)) for f in range(L // L1)) >= 2
        assert sum(k2_of(f) == set(range(L // L1)) for f in range(L1)) >= 2
        assert 1000 < len(b) < 4096
    b = V.bin_plan(4096, False, "kfwd")
    nat = b % 8192
    p, u = nat % 2, nat // 2
    k0, k1, slot = u % 16, (u // 16) % 16, u // 256
    for field in (k0, k1, slot):
        others = [f for f in (k0, k1, slot) if f is not field]
        full = [(a, c) for a in range(16) for c in range(16)
                if set(field[(others[0] == a) & (others[1] == c)].tolist()) == set(range(16))]
        assert len(full) >= 2
    assert set(p.tolist()) == {0, 1}


def test_bin_budgets_of_the_gpu_file():
    import test_gpu_every_bin as T
    for name, N, exhaustive, layout in T.bin_rows():
        bins = V.bin_plan(N, exhaustive, layout)
        if exhaustive:
            assert len(bins) == 2 * N
        assert len(bins) <= 16384, name


# ---- the bars are honest --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 256, 4096, 16384, 65536])
def test_the_float32_oracle_stays_far_inside_the_bars(N):
    """every lag against xcorr_full_scipy, every bin against scipy.fft in complex64: at most a quarter of each bar"""
    for scene in V.SCENES:
        iq = V.scenes(N)[scene][0]
        for w in range(2):
            m = V.vectors(N, scene)[w, 1]
            o = np.abs(np.asarray(orc.xcorr_full_scipy(iq[w, 0], iq[w, 1]))).astype(np.float64)
            assert o.shape == m.shape
            lag_ratio = float((np.abs(o - m) / V.bar(m, m.max())).max())
            X = V.spectra64(iq[w])
            want = V.bin_product(X[0], X[1], np.arange(-N, N))
            X32 = [sp_fft.fft(iq[w, b].astype(np.complex64), 2 * N) for b in range(2)]
            assert X32[0].dtype == np.complex64
            got = (np.abs(X32[1]) * np.abs(X32[0]) / np.float32(2 * N)).astype(np.float64)[np.arange(-N, N) % (2 * N)]
            bin_ratio = float((np.abs(got - want) / V.bar(want, want.max())).max())
            print("N = %d %s window %d: float32 oracle at %.3f of the lag bar, %.3f of the bin bar" % (N, scene, w, lag_ratio, bin_ratio))
            assert lag_ratio <= 0.25 and bin_ratio <= 0.25


@pytest.mark.parametrize("N", [256, 4096])
def test_the_doppler_rule_excuses_few_slots_on_the_reference_alone(N):
    """five hypotheses 0.5 / N apart at every lag: the float64 gap between the two largest m_d[k] is within twice the bar
    of the larger on at most 1.5 % of the slots"""
    grid = (np.arange(5) - 2) * (0.5 / N)
    for scene in V.SCENES:
        iq = V.scenes(N)[scene][0]
        for w in range(2):
            for i, j in ((0, 1), (1, 0)):
                md = np.stack([V.derotated64(iq[w, i], iq[w, j], nu) for nu in grid])          # [D][2N - 1]
                bars = V.bar(md, md.max(axis=-1, keepdims=True))
                order = np.argsort(-md, axis=0, kind="stable")
                v1, v2 = np.take_along_axis(md, order[:1], 0)[0], np.take_along_axis(md, order[1:2], 0)[0]
                b1 = np.take_along_axis(bars, order[:1], 0)[0]
                share = float(((v1 - v2) <= 2.0 * b1).mean())
                print("N = %d %s window %d pair (%d, %d): excused share %.4f" % (N, scene, w, i, j, share))
                assert share <= 0.015


# ---- the analytic figures of a one-bin band -------------------------------------------------------------------------
def test_one_bin_quality_figures_are_analytic_on_the_reference():
    N = 256
    L = 2 * N
    iq = V.scenes(N)["emitter"][0][:1]
    bins = np.unique(np.concatenate([[-N, -1, 0, 1, N - 1], np.random.default_rng(3).integers(-N, N, size=32)]))
    for s in bins.tolist():
        bd = V.one_bin_bands([s], N)[0]
        lb = np.array([[7, 7]])
        q = qr.quality_batch(iq, band=bd, lag_bounds=lb)
        assert abs(q[0, 0, qr.COHERENCE] - 1.0) <= 1e-4 and abs(q[0, 0, qr.NEFF] - 1.0) <= 1e-4
        assert abs(qr.et_over_p2(q, N)[0, 0] - L) <= 1e-4 * L
        assert abs(q[0, 0, qr.RMS_BW] - abs(s) / L) <= (1e-4 * abs(s) / L if s else 1e-7)
