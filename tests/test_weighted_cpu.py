"""rmx_xcorr_batch_weighted without a GPU: the float32 reference of the weighted correlation (tests/weighted_ref.py) against
a float64 restatement and the oracle, its bin rule, the two scenarios the weighting exists for, the export and argument
checks of the C entry and of the Python binding, the per-block slicing of MultiXcorrEngine, and the band / PHAT settings
of TDoACalculator and TDoAProcessor."""
import ctypes as C
import os

import numpy as np
import pytest

import weighted_ref as wr
from conftest import ROOT
from oracle import xcorr_ref as orc
from radio_mapper_amd import multi
from radio_mapper_amd import tdoa_processor as tp
from radio_mapper_amd import xcorr


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return xcorr.load_library()


# -- the reference ---------------------------------------------------------------------------------------------------
def _f64_full(x_i, x_j, band, phat):
    N = x_i.shape[0]
    L = 2 * N
    s = np.fft.fftfreq(L, 1.0 / L)
    keep = np.ones(L, bool) if band is None else (s / L >= band[0]) & (s / L <= band[1])

    def y(x):
        X = np.fft.fft(x.astype(np.complex128), L)
        if phat:
            a = np.abs(X)
            X = np.where(a > 0, X / np.where(a > 0, a, 1.0), 0)
        return np.where(keep, X, 0)
    r = np.fft.ifft(y(x_j) * np.conj(y(x_i)))
    return np.abs(np.concatenate([r[L - (N - 1):], r[:N]]))


@pytest.mark.parametrize("N", [16, 256, 4096])
@pytest.mark.parametrize("band,phat", [(None, True), ((-0.1, 0.3), False), ((0.0, 0.25), True)])
def test_helper_matches_a_float64_restatement(N, band, phat):
    import radio_mapper_amd as rm
    iq, _ = rm.synth.make_windows(1, 2, N, 10e6, seed=N)
    m32 = wr.weighted_full(iq[0, 0], iq[0, 1], band, phat)
    m64 = _f64_full(iq[0, 0], iq[0, 1], band, phat)
    assert np.allclose(m32, m64, rtol=1e-4, atol=1e-5 * m64.max())


def test_helper_full_band_none_is_the_oracle():
    import radio_mapper_amd as rm
    for N in (16, 256, 4096):
        iq, _ = rm.synth.make_windows(2, 3, N, 10e6, seed=N)
        ri, rf, rp = orc.xcorr_batch_literal(iq)
        li, lf, pk, mg, fm = wr.weighted_batch(iq)
        ok = mg > 1e-5
        assert np.array_equal(li[ok], ri[ok])
        assert np.all(np.abs(li + lf - (ri + rf)) <= 1e-5 * np.maximum(np.abs(ri + rf), 1.0))
        assert np.allclose(pk, rp, rtol=1e-5, atol=1e-6 * fm.max())


@pytest.mark.parametrize("N", [16, 4096])
def test_bin_rule_at_its_edges(N):
    L = 2 * N
    assert wr.mask(-0.5, 0.5, N).sum() == L
    m = wr.mask(0.0, 0.0, N)
    assert m.sum() == 1 and m[0]
    m = wr.mask(1.0 / L, 1.0 / L, N)
    assert m.sum() == 1 and m[1]
    assert wr.mask(0.5, 0.5, N).sum() == 0
    assert wr.kept_bins(0.5, 0.5, N) == (N, N - 1)
    assert wr.kept_bins(-0.5, -0.5, N) == (-N, -N)


def test_dc_offset_scenario_on_the_helper():
    iq, d = wr.dc_offset_scene()
    t = wr.true_lags(d)
    li, lf, _, _, _ = wr.weighted_batch(iq)
    assert np.all(np.abs(li[0]) < 20), li                      # plain correlation: the DC triangle at lag 0
    for kw in ({"band": (0.02, 0.5)}, {"phat": True}):
        li, lf, _, _, _ = wr.weighted_batch(iq, **kw)
        assert np.all(np.abs(li[0] + lf[0] - t) < 0.5), (kw, li[0] + lf[0], t)


def test_two_emitter_scenario_on_the_helper():
    iq, ds, dw = wr.two_emitter_scene()
    ts, tw = wr.true_lags(ds), wr.true_lags(dw)
    li, lf, _, _, _ = wr.weighted_batch(iq)
    assert np.all(np.abs(li[0] + lf[0] - ts) < 0.5)            # plain: the strong emitter's lags, for both
    li, lf, _, _, _ = wr.weighted_batch(iq, band=wr.STRONG_BAND)
    assert np.all(np.abs(li[0] + lf[0] - ts) < 0.5)
    li, lf, _, _, _ = wr.weighted_batch(iq, band=wr.WEAK_BAND)
    assert np.all(np.abs(li[0] + lf[0] - tw) < 0.5)


# -- C entry and binding -----------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_weighted_entry(lib):
    hdr = open(os.path.join(ROOT, "include", "rmx.h")).read()
    assert "int rmx_xcorr_batch_weighted(" in hdr and "RMX_WEIGHT_PHAT = 1" in hdr
    assert "rmx_xcorr_batch_weighted" in xcorr.EXPORTS
    assert hasattr(lib, "rmx_xcorr_batch_weighted")


def test_null_ctx_is_rejected(lib):
    band = (C.c_double * 2)(-0.1, 0.1)
    li, lf, pk = C.c_int32(), C.c_float(), C.c_float()
    rc = lib.rmx_xcorr_batch_weighted(None, C.byref(li), 1, None, 0, band, 0, 1, None, 0, C.byref(li), C.byref(lf),
                                      C.byref(pk), 0)
    assert rc == -1   # RMX_E_INVAL


@pytest.mark.parametrize("bad", [np.zeros(3), np.zeros((4, 2)), np.zeros((5, 3)), np.zeros((5, 2, 1)),
                                 np.array([np.nan, 0.1]), np.array([-0.1, np.inf]), np.array([-0.6, 0.1]),
                                 np.array([-0.1, 0.51]), np.array([0.2, 0.1]), np.array(["a", "b"])])
def test_check_band_rejects_bad_bands_before_any_call(bad):
    with pytest.raises(ValueError):
        xcorr.check_band(bad, 5)

    class NoCall(xcorr.XcorrEngine):
        def __init__(self):   # no library, no ctx: a C call would fail with AttributeError, not ValueError
            self.n_buoys, self.n_samples = 3, 16

        def _check_iq(self, iq):
            return iq, 0

        def __del__(self):
            pass
    with pytest.raises(ValueError):
        NoCall().correlate(np.zeros((5, 3, 16), np.complex64), band=bad)


def test_check_band_accepts_both_forms():
    a, pw = xcorr.check_band([-0.5, 0.5], 5)
    assert a.dtype == np.float64 and a.shape == (2,) and not pw
    a, pw = xcorr.check_band(np.zeros((5, 2), np.float32), 5)
    assert a.shape == (5, 2) and a.flags.c_contiguous and pw
    assert xcorr.check_band(None, 5) == (None, False)


class _Stub:
    def __init__(self, b, n, w, device=0):
        self.calls = []

    def correlate(self, iq, pairs=None, lag_bounds=None, band=None, whiten=False):
        self.calls.append((band, whiten))
        W = iq.shape[0]
        # lag_int = band lo * 1000 (per window), peak = whiten
        lo = np.zeros(W) if band is None else np.broadcast_to(np.asarray(band)[..., 0], (W,))
        return (np.broadcast_to((lo * 1000).astype(np.int32)[:, None], (W, 3)), np.zeros((W, 3), np.float32),
                np.full((W, 3), float(whiten), np.float32))

    def close(self):
        pass


def test_multi_engine_slices_per_window_bands():
    m = multi.MultiXcorrEngine(3, 16, 10, devices=[0, 1, 2], engine_factory=_Stub)
    iq = np.zeros((10, 3, 16), np.complex64)
    band = np.zeros((10, 2))
    band[:, 0] = -np.arange(10) / 1000.0
    band[:, 1] = 0.5
    li, _, pk = m.correlate(iq, band=band, whiten=True)
    assert np.array_equal(li, np.broadcast_to(-np.arange(10)[:, None], (10, 3)))
    assert np.all(pk == 1.0)
    li, _, pk = m.correlate(iq, band=[-0.003, 0.1])
    assert np.all(li == -3) and np.all(pk == 0.0)
    with pytest.raises(ValueError):
        m.correlate(iq, band=np.zeros((9, 2)))
    li, _, _ = m.correlate(iq)                       # neither: the plain call on every block
    assert all(e.calls[-1] == (None, False) for e in m._engines)
    m.close()


# -- the seam ----------------------------------------------------------------------------------------------------------
FS = 2.048e6
FC = 121.0e6


def _buoys():
    return {"A": tp.BuoyPosition("A", 37.0, -122.0, 0.0, 100), "B": tp.BuoyPosition("B", 37.0, -121.9, 0.0, 200),
            "C": tp.BuoyPosition("C", 37.2, -122.0, 0.0, 50)}


def _dets(f_mhz=121.5, fc=FC, bw=None, n=4096, ts=(0, 0, 0), ids="ABC"):
    fcs = fc if isinstance(fc, (list, tuple)) else [fc] * len(ids)
    return [tp.SignalDetection(b, f_mhz, -60.0, "t", t, 0, 0, 0.9, iq_samples=np.zeros(n, np.complex64),
                               sample_rate_hz=FS, center_freq_hz=c, bandwidth_hz=bw)
            for b, t, c in zip(ids, ts, fcs)]


def _fake(seen):
    def fake(iq, pairs=None, lag_bounds=None, band=None, whiten=False):
        seen.append({"band": None if band is None else np.asarray(band).copy(), "whiten": whiten,
                     "lag_bounds": lag_bounds})
        W = np.asarray(iq).shape[0]
        return np.zeros((W, 3), np.int32), np.zeros((W, 3), np.float32), np.ones((W, 3), np.float32)
    return fake


def test_signal_detection_fields_default_to_none():
    d = tp.SignalDetection("A", 121.5, -60.0, "t", 0, 0, 0, 0.9, "unknown", None, FS)
    assert d.center_freq_hz is None and d.bandwidth_hz is None and d.sample_rate_hz == FS
    d = tp.SignalDetection("A", 121.5, -60.0, "t", 0, 0, 0, 0.9, "unknown", None, FS, FC, 25e3)
    assert d.center_freq_hz == FC and d.bandwidth_hz == 25e3


def test_default_sends_no_band_and_no_weighting(monkeypatch):
    calc = tp.TDoACalculator()
    assert calc.band_limit is False and calc.whiten is False
    calls = []

    def fake(iq, pairs=None):          # the plain signature: a band or whiten argument would raise TypeError
        calls.append(1)
        return np.zeros((1, 3), np.int32), np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)
    monkeypatch.setattr(calc, "measure_lags", fake)
    assert len(calc.calculate_tdoa_measurements(_dets(bw=25e3), _buoys())) == 3 and calls
    p = tp.TDoAProcessor()
    assert p.tdoa_calculator.band_limit is False and p.tdoa_calculator.whiten is False


def test_band_from_centre_frequency_and_bandwidth(monkeypatch):
    calc = tp.TDoACalculator(band_limit=True)
    seen = []
    monkeypatch.setattr(calc, "measure_lags", _fake(seen))
    assert len(calc.calculate_tdoa_measurements(_dets(f_mhz=121.5, bw=25e3), _buoys())) == 3
    band = seen[0]["band"]
    assert band.shape == (1, 2) and seen[0]["whiten"] is False
    assert np.allclose(band[0], [(121.5e6 - 12.5e3 - FC) / FS, (121.5e6 + 12.5e3 - FC) / FS])
    seen.clear()
    calc.calculate_tdoa_measurements(_dets(f_mhz=120.7), _buoys())           # no bandwidth: the 10 kHz default
    assert np.allclose(seen[0]["band"][0], [(120.7e6 - 5e3 - FC) / FS, (120.7e6 + 5e3 - FC) / FS])
    seen.clear()
    calc.calculate_tdoa_measurements(_dets(f_mhz=121.5, fc=None), _buoys())  # no centre frequency: today's full band
    assert seen[0]["band"] is None
    seen.clear()
    calc.calculate_tdoa_measurements(_dets(f_mhz=122.0, bw=200e3), _buoys())  # clipped to +0.5
    assert np.isclose(seen[0]["band"][0, 1], 0.5)


@pytest.mark.parametrize("case,kw,text", [
    ("centres disagree", {"fc": [FC, FC, FC + 1e5]}, "disagree"),
    ("only some centres", {"fc": [FC, None, FC]}, "only some"),
    ("band misses the capture", {"f_mhz": 125.0}, "misses the capture"),
])
def test_refusals_are_logged_and_yield_nothing(monkeypatch, caplog, case, kw, text):
    calc = tp.TDoACalculator(band_limit=True)
    seen = []
    monkeypatch.setattr(calc, "measure_lags", _fake(seen))
    with caplog.at_level("ERROR"):
        assert calc.calculate_tdoa_measurements(_dets(**kw), _buoys()) == []
    assert text in caplog.text and not seen


def test_refusal_of_a_band_that_keeps_no_bin(monkeypatch, caplog):
    calc = tp.TDoACalculator(band_limit=True)
    # the band ends exactly at +fs/2: [0.5, 0.5] after clipping keeps no bin
    b, why = calc.band(_dets(f_mhz=(FC + FS / 2 + 5e3) / 1e6), 4096, FS)
    assert b is None and "keeps no bin" in why
    seen = []
    monkeypatch.setattr(calc, "measure_lags", _fake(seen))
    with caplog.at_level("ERROR"):
        assert calc.calculate_tdoa_measurements(_dets(f_mhz=(FC + FS / 2 + 5e3) / 1e6), _buoys()) == []
    assert "keeps no bin" in caplog.text and not seen


def test_whiten_sends_phat(monkeypatch):
    calc = tp.TDoACalculator(whiten=True)
    seen = []
    monkeypatch.setattr(calc, "measure_lags", _fake(seen))
    assert len(calc.calculate_tdoa_measurements(_dets(), _buoys())) == 3
    assert seen[0]["whiten"] is True and seen[0]["band"] is None


def test_processor_sends_one_band_per_batch(monkeypatch, caplog):
    p = tp.TDoAProcessor(band_limit=True, whiten=True)
    for b in _buoys().values():
        p.register_buoy(b)
    seen = []
    monkeypatch.setattr(p.tdoa_calculator, "measure_lags", _fake(seen))
    monkeypatch.setattr(p.hyperbolic_positioner, "triangulate_position", lambda m, pos: None)
    g1 = _dets(f_mhz=121.5, bw=20e3)
    g2 = _dets(f_mhz=121.2)
    g3 = _dets(f_mhz=121.8, fc=[FC, None, FC])        # refused: logged, not in the batch
    with caplog.at_level("ERROR"):
        p.process_signal_detections(g1 + g2 + g3)
    assert len(seen) == 1 and seen[0]["band"].shape == (2, 2) and seen[0]["whiten"] is True
    assert np.allclose(seen[0]["band"][0], [(121.5e6 - 10e3 - FC) / FS, (121.5e6 + 10e3 - FC) / FS])
    assert np.allclose(seen[0]["band"][1], [(121.2e6 - 5e3 - FC) / FS, (121.2e6 + 5e3 - FC) / FS])
    assert "only some" in caplog.text


def test_measure_lags_accepts_a_channel_axis_band(monkeypatch):
    calc = tp.TDoACalculator()
    got = {}

    class Eng:
        def correlate(self, iq, pairs=None, lag_bounds=None, band=None, whiten=False):
            got.update(band=band, whiten=whiten, W=iq.shape[0])
            W = iq.shape[0]
            return np.zeros((W, 3), np.int32), np.zeros((W, 3), np.float32), np.zeros((W, 3), np.float32)
    monkeypatch.setattr(calc, "_engine", lambda b, n, w=1: Eng())
    band = np.zeros((2, 3, 2))
    band[..., 1] = 0.25
    li, _, _ = calc.measure_lags(np.zeros((2, 3, 3, 16), np.complex64), band=band, whiten=True)
    assert li.shape == (2, 3, 3) and got["band"].shape == (6, 2) and got["W"] == 6 and got["whiten"] is True
