"""rmx_xcorr_batch_integrated without a GPU: the float32 reference of the noncoherent integration
(tests/integrated_ref.py) against a float64 restatement and the weighted helper, the two scenarios integration exists for,
the export and argument checks of the C entry and of the Python binding, the sharding of whole groups in MultiXcorrEngine,
and the integrate setting of TDoACalculator / TDoAProcessor (segments, bounds and band for N // K, refusals)."""
import ctypes as C
import os

import numpy as np
import pytest

import integrated_ref as ir
import weighted_ref as wr
from conftest import ROOT
from radio_mapper_amd import multi
from radio_mapper_amd import tdoa_processor as tp
from radio_mapper_amd import xcorr


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return xcorr.load_library()


# -- the reference ---------------------------------------------------------------------------------------------------
def _f64_full(group, i, j, band, phat):
    """sqrt(sum_w |c_w|^2) in float64, 'full' order"""
    K, _, N = group.shape
    L = 2 * N
    s = np.fft.fftfreq(L, 1.0 / L)
    acc = np.zeros(2 * N - 1)
    for w in range(K):
        bd = None if band is None else np.broadcast_to(np.asarray(band, np.float64), (K, 2))[w]
        keep = np.ones(L, bool) if bd is None else (s / L >= bd[0]) & (s / L <= bd[1])

        def y(x):
            X = np.fft.fft(x.astype(np.complex128), L)
            if phat:
                a = np.abs(X)
                X = np.where(a > 0, X / np.where(a > 0, a, 1.0), 0)
            return np.where(keep, X, 0)
        r = np.fft.ifft(y(group[w, j]) * np.conj(y(group[w, i])))
        acc += np.abs(np.concatenate([r[L - (N - 1):], r[:N]])) ** 2
    return np.sqrt(acc)


@pytest.mark.parametrize("N,K", [(16, 2), (64, 3), (256, 16), (1024, 4)])
@pytest.mark.parametrize("band,phat", [(None, False), (None, True), ((-0.1, 0.3), False), ("per window", True)])
def test_helper_matches_a_float64_restatement(N, K, band, phat):
    import radio_mapper_amd as rm
    iq, _ = rm.synth.make_windows(K, 3, N, 10e6, seed=N + K)
    if isinstance(band, str):
        band = np.stack([np.linspace(-0.4, 0.0, K), np.linspace(0.1, 0.5, K)], -1)
    m32 = ir.integrated_full(iq, 0, 2, band, phat)
    m64 = _f64_full(iq, 0, 2, band, phat)
    assert m32.dtype == np.float32
    assert np.allclose(m32, m64, rtol=1e-4, atol=1e-5 * m64.max())
    # the batch form searches the same vector: peak, lag and margin of pair (0, 2) = index 1
    li, lf, pk, mg, fm = ir.integrated_batch(iq, K, band, phat)
    assert li.shape == (1, 3)
    assert fm[0, 1] == float(m32.max()) and pk[0, 1] == float(m32.max())
    assert li[0, 1] == int(np.argmax(m32)) - (N - 1)


def test_helper_k1_is_the_weighted_helper_exactly():
    import radio_mapper_amd as rm
    for N in (16, 256):
        iq, _ = rm.synth.make_windows(4, 3, N, 10e6, seed=N)
        lb = np.array([[-3, 5], [-(N - 1), N - 1], [0, 0]])
        for kw in ({}, {"band": (-0.2, 0.3), "phat": True, "lag_bounds": lb}):
            a = ir.integrated_batch(iq, 1, with_bound=True, **kw)
            b = wr.weighted_batch(iq, with_bound=True, **kw)
            assert len(a) == len(b) == 6 and all(np.array_equal(u, v) for u, v in zip(a, b))


def test_helper_groups_bounds_and_pairs():
    import radio_mapper_amd as rm
    N, K, G = 64, 4, 3
    iq, _ = rm.synth.make_windows(K * G, 3, N, 10e6, seed=3)
    pairs = [(2, 0), (1, 1)]
    lb = np.array([[[-5, 5], [1, 9]], [[-(N - 1), N - 1], [-9, -1]], [[0, 0], [-2, 2]]])
    li, lf, pk, mg, fm, fb = ir.integrated_batch(iq, K, lag_bounds=lb, pairs=pairs, with_bound=True)
    assert li.shape == (G, 2)
    for g in range(G):
        for q, (i, j) in enumerate(pairs):
            m = ir.integrated_full(iq[g * K:(g + 1) * K], i, j)
            lo, hi = lb[g, q]
            k = int(np.argmax(m[lo + N - 1:hi + N])) + lo
            assert li[g, q] == k and pk[g, q] == float(m[k + N - 1]) and lo <= k <= hi
            if k in (lo, hi):
                assert lf[g, q] == 0.0
    with pytest.raises(ValueError):
        ir.integrated_batch(iq, 5)


# -- the scenarios (the table of the issue; the generator is ir.offset_scene) ------------------------------------------
SCENES = [("64 x 1024 at -14 dB", 65536, 64, -14.0), ("16 x 1024 at 0 dB", 16384, 16, 0.0)]


@pytest.mark.parametrize("scene", SCENES, ids=[s[0] for s in SCENES])
def test_offset_scenarios_on_the_helper(scene):
    """per-receiver frequency offsets of (0, 3, 8) cycles over the capture: the coherent correlation of the whole capture
    finds at most 3 of 60 integer lags, the integration over 1024-sample segments all 60"""
    _, n, K, snr = scene
    coherent = integrated = 0
    worst = np.inf
    for seed in range(20):
        x = ir.offset_scene(n, seed, snr)
        li, _, _, _, _ = wr.weighted_batch(x[None])
        coherent += int((li[0] == ir.TRUE_LAGS).sum())
        li, _, _, mg, _ = ir.integrated_batch(ir.segments(x, K), K)
        integrated += int((li[0] == ir.TRUE_LAGS).sum())
        worst = min(worst, float(mg.min()))
    print("coherent %d / 60, integrated %d / 60, smallest top-two margin %.3f" % (coherent, integrated, worst))
    assert coherent <= 3
    assert integrated == 60


# -- C entry and binding -----------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_integrated_entry(lib):
    hdr = open(os.path.join(ROOT, "include", "rmx.h")).read()
    assert "int rmx_xcorr_batch_integrated(" in hdr and "int integrate," in hdr
    assert "rmx_xcorr_batch_integrated" in xcorr.EXPORTS
    assert hasattr(lib, "rmx_xcorr_batch_integrated")
    import __graft_entry__ as g
    assert "integrate.hpp" in g.SOURCES


@pytest.mark.parametrize("K", [0, -3, 1, 4])
def test_null_ctx_is_rejected_whatever_k(lib, K):
    li, lf, pk = C.c_int32(), C.c_float(), C.c_float()
    rc = lib.rmx_xcorr_batch_integrated(None, C.byref(li), 4, None, 0, K, None, 0, 0, None, 0, C.byref(li), C.byref(lf),
                                        C.byref(pk), 0)
    assert rc == -1   # RMX_E_INVAL


@pytest.mark.parametrize("bad,W", [(0, 8), (-1, 8), (3, 8), (16, 8), (2.0, 8), ("2", 8), (None, 8), (True, 8), (2.5, 10)])
def test_check_integrate_rejects_before_any_call(bad, W):
    with pytest.raises(ValueError):
        xcorr.check_integrate(bad, W)

    class NoCall(xcorr.XcorrEngine):
        def __init__(self):   # no library, no ctx: a C call would fail with AttributeError, not ValueError
            self.n_buoys, self.n_samples = 3, 16

        def _check_iq(self, iq):
            return iq, 0

        def __del__(self):
            pass
    with pytest.raises(ValueError):
        NoCall().correlate(np.zeros((W, 3, 16), np.complex64), integrate=bad)
    with pytest.raises(ValueError):
        NoCall().correlate_device(0, W, 0, 0, 0, integrate=bad)


def test_check_integrate_accepts():
    assert xcorr.check_integrate(1, 7) == 1
    assert xcorr.check_integrate(np.int64(4), 8) == 4
    assert xcorr.check_integrate(8, 8) == 8
    assert xcorr.check_integrate(5, 0) == 5


def test_bounds_with_integrate_are_per_group():
    class NoCall(xcorr.XcorrEngine):
        def __init__(self):
            self.n_buoys, self.n_samples = 3, 16

        def _check_iq(self, iq):
            return iq, 0

        def __del__(self):
            pass
    with pytest.raises(ValueError):      # [W][P][2] is not a form of an integrated call's bounds: [W // K][P][2] is
        NoCall().correlate(np.zeros((8, 3, 16), np.complex64), integrate=4, lag_bounds=np.zeros((8, 3, 2), np.int32))


class _Stub:
    """lag_int = index of the group's first window within the whole batch (read out of the samples), peak = K"""

    def __init__(self, b, n, w, device=0):
        self.max_windows = w
        self.calls = []

    def correlate(self, iq, pairs=None, lag_bounds=None, band=None, whiten=False, integrate=1):
        W = iq.shape[0]
        assert W % integrate == 0 and W <= self.max_windows
        G = W // integrate
        self.calls.append({"W": W, "K": integrate, "lb": lag_bounds, "band": band})
        first = iq[::integrate, 0, 0].real.astype(np.int32)
        if lag_bounds is not None and np.asarray(lag_bounds).ndim == 3:
            assert np.asarray(lag_bounds).shape[0] == G
            first = first + 1000 * np.asarray(lag_bounds)[:, 0, 0]
        if band is not None and np.asarray(band).ndim == 2:
            assert np.asarray(band).shape[0] == W
        return (np.broadcast_to(first[:, None], (G, 3)).astype(np.int32), np.zeros((G, 3), np.float32),
                np.full((G, 3), float(integrate), np.float32))

    def close(self):
        pass


def test_multi_engine_shards_whole_groups():
    K, G = 4, 5                                   # 5 groups over 2 devices: 3 + 2
    W = K * G
    m = multi.MultiXcorrEngine(3, 16, W, devices=[0, 1], engine_factory=_Stub)
    iq = np.zeros((W, 3, 16), np.complex64)
    iq[:, 0, 0] = np.arange(W)
    li, lf, pk = m.correlate(iq, integrate=K)
    assert li.shape == (G, 3) and np.array_equal(li[:, 0], np.arange(G) * K) and np.all(pk == K)
    # every call held whole groups and fitted its engine (sized for an even split of the windows: 10 -> two groups a call)
    calls = [c for e in m._engines for c in e.calls]
    assert all(c["W"] % K == 0 and c["K"] == K for c in calls) and sum(c["W"] for c in calls) == W
    lb = np.zeros((G, 3, 2), np.int32)
    lb[:, :, 0] = -np.arange(G)[:, None]
    band = np.tile([[-0.25, 0.25]], (W, 1))
    li, _, _ = m.correlate(iq, integrate=K, lag_bounds=lb, band=band)
    assert np.array_equal(li[:, 0], np.arange(G) * K - 1000 * np.arange(G))
    with pytest.raises(ValueError):
        m.correlate(iq, integrate=3)
    with pytest.raises(ValueError):
        m.correlate(iq, integrate=K, lag_bounds=np.zeros((W, 3, 2), np.int32))
    li, _, _ = m.correlate(iq)                    # integrate = 1: today's call, one row per window
    assert li.shape == (W, 3)
    m.close()


# -- the seam ----------------------------------------------------------------------------------------------------------
FS = 2.048e6
FC = 121.0e6


def _buoys():
    return {"A": tp.BuoyPosition("A", 37.0, -122.0, 0.0, 100), "B": tp.BuoyPosition("B", 37.0, -121.9, 0.0, 200),
            "C": tp.BuoyPosition("C", 37.2, -122.0, 0.0, 50)}


def _dets(n=4096, f_mhz=121.5, bw=None, fc=None, ts=(0, 0, 0), ids="ABC", u8=False):
    out = []
    for k, (b, t) in enumerate(zip(ids, ts)):
        if u8:
            s = (np.arange(2 * n) % 251).astype(np.uint8) + k
        else:
            s = (np.arange(n) + 100000 * k).astype(np.complex64)
        out.append(tp.SignalDetection(b, f_mhz, -60.0, "t", t, 0, 0, 0.9, iq_samples=s, sample_rate_hz=FS, center_freq_hz=fc,
                                      bandwidth_hz=bw))
    return out


def _fake(seen):
    def fake(iq, pairs=None, lag_bounds=None, band=None, whiten=False, integrate=1):
        iq = np.asarray(iq)
        seen.append({"iq": iq.copy(), "band": None if band is None else np.asarray(band).copy(), "whiten": whiten,
                     "lag_bounds": None if lag_bounds is None else np.asarray(lag_bounds).copy(), "integrate": integrate})
        G = iq.shape[0] // integrate
        return np.full((G, 3), 2, np.int32), np.zeros((G, 3), np.float32), np.ones((G, 3), np.float32)
    return fake


def test_default_is_off_and_sends_no_integrate(monkeypatch):
    calc = tp.TDoACalculator()
    assert calc.integrate == 1 and tp.TDoAProcessor().tdoa_calculator.integrate == 1
    assert tp.TDoAProcessor(integrate=8).tdoa_calculator.integrate == 8
    calls = []

    def fake(iq, pairs=None):          # the plain signature: an integrate argument would raise TypeError
        calls.append(1)
        return np.zeros((1, 3), np.int32), np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)
    monkeypatch.setattr(calc, "measure_lags", fake)
    assert len(calc.calculate_tdoa_measurements(_dets(), _buoys())) == 3 and calls


@pytest.mark.parametrize("u8", [False, True])
def test_segments_are_consecutive_cuts_of_each_window(monkeypatch, u8):
    K, n = 16, 4096
    calc = tp.TDoACalculator(integrate=K)
    seen = []
    monkeypatch.setattr(calc, "measure_lags", _fake(seen))
    dets = _dets(n, u8=u8)
    meas = calc.calculate_tdoa_measurements(dets, _buoys())
    assert len(meas) == 3 and len(seen) == 1                     # one lag per pair, as without integration
    assert all(m.time_difference_ns == round(2 / FS * 1e9) for m in meas)
    s = seen[0]
    per = 2 if u8 else 1
    assert s["integrate"] == K and s["iq"].shape == (K, 3, per * n // K)
    for w in range(K):
        for b in range(3):
            want = np.asarray(dets[b].iq_samples)[w * per * n // K:(w + 1) * per * n // K]
            assert np.array_equal(s["iq"][w, b], want)


def test_bounds_and_band_are_derived_for_the_segment_length(monkeypatch):
    K, n = 4, 4096
    ref = tp.TDoACalculator(bound_lags=True, band_limit=True)
    want_lb, _ = ref.lag_bounds(_dets(n, fc=FC, bw=25e3, ts=(0, 3000, -2000)), _buoys(), n // K, FS)
    want_band, why = ref.band(_dets(n, fc=FC, bw=25e3), n // K, FS)
    assert why is None
    calc = tp.TDoACalculator(bound_lags=True, band_limit=True, integrate=K)
    seen = []
    monkeypatch.setattr(calc, "measure_lags", _fake(seen))
    calc.calculate_tdoa_measurements(_dets(n, fc=FC, bw=25e3, ts=(0, 3000, -2000)), _buoys())
    s = seen[0]
    assert s["lag_bounds"].shape == (1, 3, 2) and np.array_equal(s["lag_bounds"][0], want_lb)      # per GROUP
    assert np.all(np.abs(s["lag_bounds"]) <= n // K - 1)
    assert s["band"].shape == (K, 2) and np.allclose(s["band"], want_band)                         # per WINDOW


@pytest.mark.parametrize("K,n,text", [(3, 4096, "not a power of two"), (32, 4096 - 16, None), (64, 4096, "below 128"),
                                      (8192, 4096, "does not divide")])
def test_refusals_are_logged_and_yield_nothing(monkeypatch, caplog, K, n, text):
    calc = tp.TDoACalculator(integrate=K)
    seen = []
    monkeypatch.setattr(calc, "measure_lags", _fake(seen))
    if text is None:
        # windows of 4080 samples are cut to 2048 first (they are not a power of two); 2048 / 32 = 64 < 128
        dets = _dets(n)
        dets[0].iq_samples = np.zeros(4096, np.complex64)
        text = "below 128"
    else:
        dets = _dets(n)
    with caplog.at_level("ERROR"):
        assert calc.calculate_tdoa_measurements(dets, _buoys()) == []
    assert "Cannot integrate" in caplog.text and text in caplog.text and not seen   # never a silent K = 1


def test_segment_length_rule():
    calc = tp.TDoACalculator(integrate=16)
    assert calc.segment_length(16384) == (1024, None)
    assert calc.segment_length(2048) == (128, None)
    assert calc.segment_length(1024)[0] is None
    calc.min_cut_samples = 0
    assert calc.segment_length(256) == (16, None) and calc.segment_length(128)[0] is None   # the engine's shortest window


def test_processor_integrates_every_group_of_a_batch(monkeypatch, caplog):
    K, n = 8, 4096
    p = tp.TDoAProcessor(integrate=K)
    for b in _buoys().values():
        p.register_buoy(b)
    seen = []
    monkeypatch.setattr(p.tdoa_calculator, "measure_lags", _fake(seen))
    got = []
    monkeypatch.setattr(p.hyperbolic_positioner, "triangulate_position", lambda m, pos: got.append(m))
    p.process_signal_detections(_dets(n, f_mhz=121.5) + _dets(n, f_mhz=121.2))
    assert len(seen) == 1 and seen[0]["integrate"] == K and seen[0]["iq"].shape == (2 * K, 3, n // K)
    assert len(got) == 2 and all(len(m) == 3 for m in got)
    # a batch whose segments cannot be formed: logged per group, no measurements, no call
    seen.clear()
    got.clear()
    p.tdoa_calculator.integrate = 64
    with caplog.at_level("ERROR"):
        p.process_signal_detections(_dets(n, f_mhz=121.5) + _dets(n, f_mhz=121.2))
    assert not seen and not got and caplog.text.count("Cannot integrate") == 2


def test_measure_lags_passes_integrate_and_reshapes_a_channel_axis(monkeypatch):
    calc = tp.TDoACalculator()
    got = {}

    class Eng:
        def correlate(self, iq, pairs=None, lag_bounds=None, band=None, whiten=False, integrate=1):
            got.update(lb=lag_bounds, band=band, W=iq.shape[0], K=integrate)
            G = iq.shape[0] // integrate
            return np.zeros((G, 3), np.int32), np.zeros((G, 3), np.float32), np.zeros((G, 3), np.float32)
    monkeypatch.setattr(calc, "_engine", lambda b, n, w=1: Eng())
    li, _, _ = calc.measure_lags(np.zeros((8, 3, 16), np.complex64), integrate=4)
    assert li.shape == (2, 3) and got["K"] == 4 and got["W"] == 8
    lb = np.zeros((2, 2, 3, 2), np.int32)
    band = np.zeros((2, 8, 2))
    li, _, _ = calc.measure_lags(np.zeros((2, 8, 3, 16), np.complex64), integrate=4, lag_bounds=lb, band=band)
    assert li.shape == (2, 2, 3) and got["lb"].shape == (4, 3, 2) and got["band"].shape == (16, 2) and got["W"] == 16
    with pytest.raises(ValueError):
        calc.measure_lags(np.zeros((8, 3, 16), np.complex64), integrate=3)
