"""The quality figures of rmx_xcorr_batch_quality without a GPU: the restatement (tests/quality_ref.py) against Parseval and
its closed forms, the ranges the figures take on signal and noise-only scenes, psr_threshold and lag_sigma against them,
the seam (MultiXcorrEngine, TDoACalculator) on stub engines, and the library's new symbol."""
import logging
import math

import numpy as np
import pytest

import quality_ref as qr
import radio_mapper_amd as rm
import refined_ref as rr
import weighted_ref as wr
from radio_mapper_amd import multi, xcorr
from radio_mapper_amd import tdoa_processor as tp

PAIRS3 = ((0, 1), (0, 2), (1, 2))


def _scene(W, N, snr_db, B=3, **kw):
    return rm.synth.make_windows(W, B, N, 10e6, seed=7, snr_db=snr_db, bandwidth=0.8, max_delay=min(40, N / 8), **kw)


@pytest.fixture(scope="module")
def scenes():
    """(iq, delays, quality, detail) of the signal scenes, computed once: (N, snr_db) -> ..."""
    out = {}
    for N, W in ((1024, 16), (4096, 8)):
        for snr in (10, 0):
            iq, delays = _scene(W, N, snr)
            out[N, snr] = (iq, delays) + qr.quality_batch(iq, detail=True)
    return out


# -- the restatement itself -------------------------------------------------------------------------------------------------
def test_parseval(scenes):
    """Et = sum over all L circular lags of |r|^2, r = IFFT_L(P)"""
    iq, _, _, det = scenes[1024, 10]
    for w in (0, 5):
        spec = [np.asarray(wr.weighted_spectrum(iq[w, b]), np.complex128) for b in range(3)]
        for q, (i, j) in enumerate(PAIRS3):
            r = np.fft.ifft(spec[j] * np.conj(spec[i]))
            assert det["Et"][w, q] == pytest.approx(float((np.abs(r) ** 2).sum()), rel=1e-10)
    spec = [np.asarray(wr.weighted_spectrum(iq[0, b], (-0.2, 0.3), True), np.complex128) for b in range(2)]
    et = qr.quality_batch(iq[:1, :2], band=(-0.2, 0.3), phat=True, detail=True)[1]["Et"][0, 0]
    assert et == pytest.approx(float((np.abs(np.fft.ifft(spec[1] * np.conj(spec[0]))) ** 2).sum()), rel=1e-10)


def test_identical_windows_have_coherence_1(scenes):
    iq = scenes[1024, 10][0][:2].copy()
    iq[:, 1] = iq[:, 0]
    iq[:, 2] = iq[:, 0]
    for K in (1, 2):
        q = qr.quality_batch(iq, integrate=K)
        assert np.all(np.abs(q[..., qr.COHERENCE] - 1.0) <= 1e-6), q[..., qr.COHERENCE]


def test_full_band_phat_has_n_eff_L_and_coherence_by_kept_bins(scenes):
    iq = scenes[1024, 10][0][:2]
    q, det = qr.quality_batch(iq, phat=True, detail=True)
    assert np.all(np.abs(q[..., qr.NEFF] / 2048.0 - 1.0) <= 1e-6)
    assert np.all(np.abs(q[..., qr.COHERENCE] - det["p0"]) <= 1e-6)          # p0 L / kept bins, every bin kept
    q, det = qr.quality_batch(iq, band=(-0.25, 0.25), phat=True, detail=True)
    kept = wr.mask(-0.25, 0.25, 1024).sum()
    assert np.all(np.abs(q[..., qr.NEFF] / kept - 1.0) <= 1e-6)
    assert np.all(np.abs(q[..., qr.COHERENCE] - det["p0"] * 2048.0 / kept) <= 1e-6)
    q4 = qr.quality_batch(np.concatenate([iq, iq]), integrate=4, phat=True)   # K L when K windows are integrated
    assert np.all(np.abs(q4[..., qr.NEFF] / (4 * 2048.0) - 1.0) <= 1e-6)


@pytest.mark.parametrize("phat", [False, True])
def test_zeros_give_zeros(scenes, phat):
    iq = scenes[1024, 10][0][:2].copy()
    iq[:, 1] = 0
    q = qr.quality_batch(iq, phat=phat)
    assert np.all(np.isfinite(q))
    assert np.all(q[:, [0, 2]] == 0) and np.all(q[:, 1] > 0)
    assert np.all(qr.quality_batch(np.zeros((2, 3, 64), np.complex64), integrate=2, phat=phat) == 0)


# -- what the figures say on scenes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snr,coh_lo,coh_hi,psr_min", [(10, 0.6, 0.95, 400.0), (0, 0.3, 0.6, 150.0)])
def test_signal_scenes(scenes, snr, coh_lo, coh_hi, psr_min):
    q = scenes[1024, snr][2]
    coh, psr = q[..., qr.COHERENCE], q[..., qr.PSR]
    print("%d dB: coherence %.3f .. %.3f, psr %.0f .. %.0f" % (snr, coh.min(), coh.max(), psr.min(), psr.max()))
    assert np.all(coh >= coh_lo) and np.all(coh <= coh_hi)
    assert np.all(psr > psr_min)
    assert np.all(psr > xcorr.psr_threshold(2047, 1e-3))


def test_noise_only_scene_stays_below_the_threshold():
    rng = np.random.default_rng(3)
    iq = (rng.standard_normal((32, 3, 1024)) + 1j * rng.standard_normal((32, 3, 1024))).astype(np.complex64)
    q = qr.quality_batch(iq)
    t = xcorr.psr_threshold(2047, 1e-3)
    assert t == pytest.approx(29.06, abs=0.01)
    print("noise only: max psr %.2f (threshold %.2f), max coherence %.3f" % (q[..., qr.PSR].max(), t, q[..., qr.COHERENCE].max()))
    assert q[..., qr.PSR].size == 96
    assert np.all(q[..., qr.PSR] < t)
    assert np.all(q[..., qr.COHERENCE] < 0.2)


def test_integrated_scene_n_eff():
    N, K, G = 1024, 4, 2
    iq, _ = _scene(G * K, N, 0)      # (n_eff reads magnitudes only: the windows' own delays do not enter)
    q = qr.quality_batch(iq, integrate=K)
    print("integrate = 4, 0 dB: n_eff / N = %s" % np.round(q[..., qr.NEFF] / N, 2).tolist())
    assert q.shape == (G, 3, 4)
    assert np.all(q[..., qr.NEFF] / N >= 3.0) and np.all(q[..., qr.NEFF] / N <= 5.5)


# -- the helpers of the package ------------------------------------------------------------------------------------------------
def test_psr_threshold():
    assert xcorr.psr_threshold(2047, 1e-3) == pytest.approx(2.0 * math.log(2047 / 1e-3), rel=1e-12)
    for K in (2, 4, 16):     # n_lags Q(K, K T / 2) = pfa, checked by putting T back
        T = xcorr.psr_threshold(2047, 1e-3, K)
        x = K * T / 2.0
        tail = math.exp(-x) * sum(x ** n / math.factorial(n) for n in range(K))
        assert 2047 * tail == pytest.approx(1e-3, rel=1e-9)
    ts = [xcorr.psr_threshold(2047, 1e-3, K) for K in (1, 2, 4, 16)]
    assert ts == sorted(ts, reverse=True) and ts[-1] > 1.0      # integration lowers the bar, never below the floor
    assert xcorr.psr_threshold(8191, 1e-3) > xcorr.psr_threshold(2047, 1e-3) > xcorr.psr_threshold(2047, 1e-2)
    for bad in ((0, 1e-3, 1), (10, 0.0, 1), (10, 1.0, 1), (10, 1e-3, 0), (10, 1e-3, 1.5)):
        with pytest.raises(ValueError):
            xcorr.psr_threshold(*bad)


def test_lag_sigma_edges():
    q = np.array([[0.8, 500.0, 0.23, 1700.0], [0.0, 0.0, 0.0, 0.0], [1.0, 9.0, 0.2, 100.0], [0.5, 9.0, 0.0, 100.0]])
    s = xcorr.lag_sigma(q)
    assert s[0] == pytest.approx(math.sqrt((1 - 0.64) / (0.64 * 1700.0)) / (2 * math.pi * 0.23), rel=1e-12)
    assert np.isinf(s[1]) and s[2] == 0.0 and np.isinf(s[3])
    assert xcorr.lag_sigma(np.zeros((2, 3, 4))).shape == (2, 3)
    with pytest.raises(ValueError):
        xcorr.lag_sigma(np.zeros((2, 3)))


@pytest.mark.parametrize("N,snr", [(1024, 10), (4096, 10), (1024, 0), (4096, 0)])
def test_lag_sigma_against_the_observed_error(scenes, N, snr):
    """observed rms error of the refined lag (refine = 8) over the predicted rms: a rough indicator, within [0.25, 2]"""
    iq, delays, q, _ = scenes[N, snr]
    li, lf = rr.refined_batch(iq, 8)[:2]
    true = np.stack([delays[:, j] - delays[:, i] for i, j in PAIRS3], axis=1)
    observed = float(np.sqrt(np.mean((li + lf - true) ** 2)))
    predicted = float(np.sqrt(np.mean(xcorr.lag_sigma(q) ** 2)))
    print("N = %d, %d dB: observed %.4f / predicted %.4f = %.2f" % (N, snr, observed, predicted, observed / predicted))
    assert 0.25 <= observed / predicted <= 2.0


# -- the seam, on stub engines -----------------------------------------------------------------------------------------------
class _Stub:
    def __init__(self, b, n, w, device):
        self.n_buoys, self.n_samples, self.max_windows, self.device = b, n, w, device
        self.calls = []

    def correlate(self, iq, pairs=None, lag_bounds=None, band=None, whiten=False, integrate=1, refine=0, quality=False):
        self.calls.append(dict(W=iq.shape[0], integrate=integrate, refine=refine, quality=quality))
        G, P = iq.shape[0] // integrate, 3
        first = np.round(iq[::integrate, 0, 0].real).astype(np.int32)       # the window's own number
        li = np.repeat(first[:, None], P, axis=1)
        out = (li, np.zeros((G, P), np.float32), np.ones((G, P), np.float32))
        if quality:
            out += (li[..., None].astype(np.float32) + np.arange(4, dtype=np.float32) / 4,)
        return out

    def close(self):
        pass


@pytest.mark.parametrize("K", [1, 2])
def test_multi_engine_gathers_the_fourth_array(K):
    W = 12
    iq = np.zeros((W, 3, 16), np.complex64)
    iq[:, 0, 0] = np.arange(W)
    m = multi.MultiXcorrEngine(3, 16, W, devices=[0, 1, 2], engine_factory=_Stub)
    li, lf, pk, q = m.correlate(iq, integrate=K, refine=4, quality=True)
    assert q.shape == (W // K, 3, 4) and q.dtype == np.float32
    assert np.array_equal(li[:, 0], np.arange(0, W, K))
    assert np.array_equal(q, li[..., None] + np.arange(4, dtype=np.float32) / 4)
    assert all(c["quality"] and c["refine"] == 4 and c["integrate"] == K for e in m._engines for c in e.calls)
    assert len(m.correlate(iq, integrate=K)) == 3
    m.close()


def _seam(min_psr=None, correlation_confidence=False, processor=False):
    """three buoys, one group with IQ; the stub engine answers lags (5, 9, 4) and a low psr on pair (0, 2)"""
    buoys = [("B0", 35.0, -97.0, 0.0, 100.0), ("B1", 35.1, -97.0, 0.0, 100.0), ("B2", 35.0, -97.1, 0.0, 100.0)]
    rng = np.random.default_rng(0)
    dets = [tp.SignalDetection(b[0], 121.5, -50, "t", 1_000_000 + 1000 * k, b[1], b[2], 0.9, "beacon",
                               (rng.standard_normal(64) + 1j * rng.standard_normal(64)).astype(np.complex64), 2.4e6)
            for k, b in enumerate(buoys)]
    seen = []

    class Eng:
        max_windows = 64

        def correlate(self, iq, pairs=None, **kw):
            seen.append(kw)
            W = iq.shape[0]
            out = (np.tile(np.array([5, 9, 4], np.int32), (W, 1)), np.zeros((W, 3), np.float32), np.ones((W, 3), np.float32))
            if kw.get("quality"):
                q = np.array([[0.8, 600.0, 0.2, 900.0], [0.1, 12.0, 0.2, 900.0], [0.5, 300.0, 0.2, 900.0]], np.float32)
                out += (np.tile(q, (W, 1, 1)),)
            return out

        def close(self):
            pass

    if processor:
        p = tp.TDoAProcessor(min_psr=min_psr, correlation_confidence=correlation_confidence)
        calc = p.tdoa_calculator
    else:
        calc = tp.TDoACalculator(min_psr=min_psr, correlation_confidence=correlation_confidence)
    calc._engine = lambda b, n, w=1: Eng()
    pos = {b[0]: tp.BuoyPosition(*b) for b in buoys}
    if processor:
        for b in pos.values():
            p.register_buoy(b)
        got = []
        p.hyperbolic_positioner.triangulate_position = lambda meas, positions: got.extend(meas)
        p.process_signal_detections(dets)
        return got, seen
    return calc.calculate_tdoa_measurements(dets, pos), seen


@pytest.mark.parametrize("processor", [False, True])
def test_calculator_defaults_are_unchanged_and_ask_for_no_quality(processor):
    meas, seen = _seam(processor=processor)
    assert len(meas) == 3 and seen == [{}]
    base = tp.TDoACalculator()
    conf = 0.9 * min(math.exp(-math.hypot(100.0, 100.0) / 100000), 1.0)
    assert [m.confidence for m in meas] == [conf] * 3
    assert [m.time_difference_ns for m in meas] == [1000 * (j - i) + int(round(lag / 2.4e6 * 1e9))
                                                    for (i, j), lag in zip(PAIRS3, (5, 9, 4))]
    assert base.min_psr is None and base.correlation_confidence is False


@pytest.mark.parametrize("processor", [False, True])
def test_calculator_min_psr_drops_the_low_pair(processor, caplog):
    plain, _ = _seam(processor=processor)
    with caplog.at_level(logging.WARNING):
        meas, seen = _seam(min_psr=29.06, processor=processor)
    assert len(seen) == 1 and seen[0].get("quality") is True and not seen[0].get("refine")
    assert [(m.buoy1_id, m.buoy2_id) for m in meas] == [("B0", "B1"), ("B1", "B2")]
    assert [m.confidence for m in meas] == [plain[0].confidence, plain[2].confidence]       # dropped, not reweighted
    assert [m.time_difference_ns for m in meas] == [plain[0].time_difference_ns, plain[2].time_difference_ns]
    assert "B0-B2 dropped" in caplog.text and "min_psr" in caplog.text


@pytest.mark.parametrize("processor", [False, True])
def test_calculator_correlation_confidence_scales(processor):
    plain, _ = _seam(processor=processor)
    meas, seen = _seam(correlation_confidence=True, processor=processor)
    assert len(seen) == 1 and seen[0].get("quality") is True and len(meas) == 3
    for m, p, coh in zip(meas, plain, (0.8, 0.1, 0.5)):
        assert m.confidence == pytest.approx(p.confidence * float(np.float32(coh)), rel=1e-12)
        assert m.time_difference_ns == p.time_difference_ns
    both, _ = _seam(min_psr=100.0, correlation_confidence=True, processor=processor)
    assert [m.confidence for m in both] == [meas[0].confidence, meas[2].confidence]


# -- the library ----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_quality_entry():
    import __graft_entry__ as g
    g.build()
    lib = xcorr.load_library()
    assert getattr(lib, "rmx_xcorr_batch_quality") is not None
    assert "rmx_xcorr_batch_quality" in xcorr.EXPORTS
    assert lib.rmx_xcorr_batch_quality(None, None, 0, None, 0, 1, None, 0, 0, None, 0, 0, None, None, None, None, 0) == -1
