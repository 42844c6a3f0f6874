"""rmx_xcorr_batch_bounded without a GPU: the export, argument checks of the C entry and of the Python binding, the
interval arithmetic of TDoACalculator(bound_lags=True), the per-block slicing of MultiXcorrEngine, and the sliced
reference of the GPU tests."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROOT
from lag_bounds_ref import bounded_batch, full_magnitude, peak_in_slice
from oracle import xcorr_ref as orc
from radio_mapper_amd import multi
from radio_mapper_amd import tdoa_processor as tp
from radio_mapper_amd import xcorr


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return xcorr.load_library()


def test_header_declares_and_library_exports_the_bounded_entry(lib):
    hdr = open(os.path.join(ROOT, "include", "rmx.h")).read()
    assert "int rmx_xcorr_batch_bounded(" in hdr
    assert "rmx_xcorr_batch_bounded" in xcorr.EXPORTS
    assert hasattr(lib, "rmx_xcorr_batch_bounded")


def test_null_ctx_is_rejected(lib):
    b = (C.c_int32 * 2)(0, 0)
    li, lf, pk = C.c_int32(), C.c_float(), C.c_float()
    rc = lib.rmx_xcorr_batch_bounded(None, C.byref(li), 1, None, 0, b, 0, C.byref(li), C.byref(lf), C.byref(pk), 0)
    assert rc == -1   # RMX_E_INVAL


@pytest.mark.parametrize("bad", [np.zeros((2, 2), np.int32), np.zeros((3, 3), np.int32), np.zeros((4, 3, 2), np.int32),
                                 np.zeros((3, 2), np.float32), np.zeros((6,), np.int32)])
def test_binding_rejects_bad_bounds_before_any_call(bad):
    with pytest.raises(ValueError):
        xcorr.check_lag_bounds(bad, 5, 3)

    class NoCall(xcorr.XcorrEngine):
        def __init__(self):   # no library, no ctx: a C call would fail with AttributeError, not ValueError
            self.n_buoys, self.n_samples = 3, 16

        def _check_iq(self, iq):
            return iq, 0

        def __del__(self):
            pass
    with pytest.raises(ValueError):
        NoCall().correlate(np.zeros((5, 3, 16), np.complex64), lag_bounds=bad)


def test_binding_accepts_both_forms():
    a, pw = xcorr.check_lag_bounds(np.zeros((3, 2), np.int64), 5, 3)
    assert a.dtype == np.int32 and a.flags.c_contiguous and not pw
    a, pw = xcorr.check_lag_bounds(np.zeros((5, 3, 2), np.int16), 5, 3)
    assert a.shape == (5, 3, 2) and pw
    assert xcorr.check_lag_bounds(None, 5, 3) == (None, False)


def _buoys():
    return {"A": tp.BuoyPosition("A", 37.0, -122.0, 0.0, 100), "B": tp.BuoyPosition("B", 37.0, -121.9, 0.0, 200),
            "C": tp.BuoyPosition("C", 37.2, -122.0, 0.0, 50)}


def _dets(ts, n=4096, fs=10e6, ids="ABC"):
    return [tp.SignalDetection(b, 121.5, -60.0, "t", t, 0, 0, 0.9, iq_samples=np.zeros(n, np.complex64), sample_rate_hz=fs)
            for b, t in zip(ids, ts)]


def _expected(p1, p2, ds_ns, fs, n, g=2):
    a = tp.GeodeticCalculator.lat_lng_to_xyz(p1.lat, p1.lng, p1.altitude)
    b = tp.GeodeticCalculator.lat_lng_to_xyz(p2.lat, p2.lng, p2.altitude)
    reach = math.dist(a, b) / 299792458.0 + math.hypot(p1.timing_accuracy_ns, p2.timing_accuracy_ns) * 1e-9
    lo = math.ceil(fs * (-reach - ds_ns * 1e-9)) - g
    hi = math.floor(fs * (reach - ds_ns * 1e-9)) + g
    return max(lo, -(n - 1)), min(hi, n - 1)


def test_seam_bounds_reach_the_engine(monkeypatch):
    calc = tp.TDoACalculator(bound_lags=True)
    seen = []

    def fake(iq, pairs=None, lag_bounds=None):
        seen.append(None if lag_bounds is None else np.asarray(lag_bounds).copy())
        W, B = np.asarray(iq).shape[:2]
        P = B * (B - 1) // 2
        return np.zeros((W, P), np.int32), np.zeros((W, P), np.float32), np.ones((W, P), np.float32)

    monkeypatch.setattr(calc, "measure_lags", fake)
    pos = _buoys()
    t0 = 10 ** 18
    ts = [t0, t0 + 3000, t0 - 1500]                # non-zero window-start differences
    meas = calc.calculate_tdoa_measurements(_dets(ts), pos)
    assert len(meas) == 3 and len(seen) == 1 and seen[0].shape == (1, 3, 2)
    ids = "ABC"
    q = 0
    for i in range(3):
        for j in range(i + 1, 3):
            assert tuple(seen[0][0, q]) == _expected(pos[ids[i]], pos[ids[j]], ts[j] - ts[i], 10e6, 4096)
            q += 1
    # A-B: 8.9 km -> about 297 samples of reach, shifted by the 3 us start difference (30 samples)
    lo, hi = seen[0][0, 0]
    assert -340 < lo < -300 and 240 < hi < 280


def test_seam_skips_a_pair_with_an_empty_interval(monkeypatch, caplog):
    calc = tp.TDoACalculator(bound_lags=True)
    monkeypatch.setattr(calc, "measure_lags", lambda iq, pairs=None, lag_bounds=None: (
        np.zeros((1, 3), np.int32), np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)))
    t0 = 10 ** 18
    # C starts 1 ms after A and B: 10000 samples, more than any lag of a 4096-sample window can undo
    with caplog.at_level("WARNING"):
        meas = calc.calculate_tdoa_measurements(_dets([t0, t0, t0 + 1_000_000]), _buoys())
    assert [(m.buoy1_id, m.buoy2_id) for m in meas] == [("A", "B")]
    assert "no lag of the window is physical" in caplog.text


def test_unknown_position_gets_the_full_interval():
    calc = tp.TDoACalculator(bound_lags=True)
    pos = _buoys()
    pos.pop("C")
    b, empty = calc.lag_bounds(_dets([0, 0, 0]), pos, 4096, 10e6)
    assert tuple(b[1]) == (-4095, 4095) and tuple(b[2]) == (-4095, 4095) and not empty.any()


def test_default_sends_no_bounds(monkeypatch):
    calc = tp.TDoACalculator()
    assert calc.bound_lags is False
    calls = []

    def fake(iq, pairs=None):          # the unbounded signature: a bounds argument would raise TypeError
        calls.append(1)
        return np.zeros((1, 3), np.int32), np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)

    monkeypatch.setattr(calc, "measure_lags", fake)
    assert len(calc.calculate_tdoa_measurements(_dets([0, 0, 0]), _buoys())) == 3 and calls


def test_processor_passes_per_window_bounds(monkeypatch):
    p = tp.TDoAProcessor()
    for b in _buoys().values():
        p.register_buoy(b)
    p.tdoa_calculator.bound_lags = True
    seen = []

    def fake(iq, pairs=None, lag_bounds=None):
        seen.append(np.asarray(lag_bounds).copy())
        W = np.asarray(iq).shape[0]
        return np.zeros((W, 3), np.int32), np.zeros((W, 3), np.float32), np.ones((W, 3), np.float32)

    monkeypatch.setattr(p.tdoa_calculator, "measure_lags", fake)
    t0 = 10 ** 18
    d1 = _dets([t0, t0, t0])
    d2 = [tp.SignalDetection(d.buoy_id, 156.8, d.signal_strength_dbm, "t", d.gps_timestamp_ns + k * 700, 0, 0, 0.9,
                             iq_samples=d.iq_samples, sample_rate_hz=d.sample_rate_hz) for k, d in enumerate(d1)]
    monkeypatch.setattr(p.hyperbolic_positioner, "triangulate_position", lambda m, pos: None)
    p.process_signal_detections(d1 + d2)
    assert len(seen) == 1 and seen[0].shape == (2, 3, 2)
    assert not np.array_equal(seen[0][0], seen[0][1])      # each group its own window starts


class _Stub:
    def __init__(self, b, n, w, device=0):
        self.calls = []

    def correlate(self, iq, pairs=None, lag_bounds=None):
        self.calls.append(None if lag_bounds is None else np.asarray(lag_bounds).copy())
        W = iq.shape[0]
        lb = np.zeros((W, 3), np.int32) if lag_bounds is None else np.broadcast_to(np.asarray(lag_bounds)[..., 0], (W, 3))
        return lb.astype(np.int32), np.zeros((W, 3), np.float32), np.zeros((W, 3), np.float32)

    def close(self):
        pass


def test_multi_engine_slices_per_window_bounds():
    m = multi.MultiXcorrEngine(3, 16, 10, devices=[0, 1, 2], engine_factory=_Stub)
    iq = np.zeros((10, 3, 16), np.complex64)
    lb = np.zeros((10, 3, 2), np.int32)
    lb[..., 0] = np.arange(10)[:, None]
    lb[..., 1] = 15
    li, _, _ = m.correlate(iq, lag_bounds=lb)
    assert np.array_equal(li, np.broadcast_to(np.arange(10)[:, None], (10, 3)))
    shared = np.array([[-3, 3]] * 3, np.int32)
    li, _, _ = m.correlate(iq, lag_bounds=shared)
    assert np.all(li == -3)
    with pytest.raises(ValueError):
        m.correlate(iq, lag_bounds=np.zeros((9, 3, 2), np.int32))
    m.close()


def test_sliced_reference_with_the_full_interval_is_the_oracle():
    import radio_mapper_amd as rm
    for N in (16, 256, 4096):
        iq, _ = rm.synth.make_windows(2, 3, N, 10e6, seed=N)
        ri, rf, rp = orc.xcorr_batch_literal(iq)
        li, lf, pk, _, _ = bounded_batch(iq, np.array([[-(N - 1), N - 1]] * 3))
        assert np.array_equal(li, ri) and np.array_equal(lf, rf) and np.allclose(pk, rp, rtol=0, atol=0)


def test_sliced_reference_edges():
    m = np.array([0, 1, 5, 2, 9, 3, 0], np.float32)          # N = 4: lags -3 .. 3, max 9 at lag 1
    assert peak_in_slice(m, 4, -3, 0)[:3] == (-1, orc.parabolic_offset(1, 5, 2), 5.0)
    assert peak_in_slice(m, 4, 2, 3)[:3] == (2, 0.0, 3.0)    # edge of the slice: frac 0
    assert peak_in_slice(m, 4, -3, -3)[:3] == (-3, 0.0, 0.0)
