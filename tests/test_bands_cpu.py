"""rmx_xcorr_batch_bands without a GPU: the reference helper (tests/bands_ref.py) against a direct masked-FFT restatement,
the checks of the Python binding, the export and NULL-ctx check of the C entry, the argument errors of
measure_lags(bands=...), and the share_captures merge of TDoAProcessor with a stub engine."""
import ctypes as C
import os

import numpy as np
import pytest

import bands_ref as br
from conftest import ROOT
from radio_mapper_amd import multi
from radio_mapper_amd import synth
from radio_mapper_amd import tdoa_processor as tp
from radio_mapper_amd import xcorr


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return xcorr.load_library()


# -- the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("phat", [False, True])
def test_helper_matches_a_masked_fft_restatement(N, phat):
    W, B, M, L = 3, 3, 4, 2 * N
    iq, _ = synth.make_windows(W, B, N, 10e6, seed=N)
    rng = np.random.default_rng(N + phat)
    a = rng.uniform(-0.5, 0.5 - 4.0 / L, size=(W, M))
    bands = np.stack([a, np.minimum(a + rng.uniform(2.0 / L, 0.5, size=(W, M)), 0.5)], -1)
    shared = bands[0]
    s = np.fft.fftfreq(L, 1.0 / L)                       # the signed bin of every natural bin
    for form in (bands, shared):
        li, lf, pk, mg, fm = br.bands_batch(iq, form, phat)
        assert li.shape == pk.shape == mg.shape == (W, M, 3)
        pw = br.per_window(form, W)
        for w in range(W):
            X = np.fft.fft(iq[w].astype(np.complex128), L, axis=-1)
            if phat:
                X = X / np.abs(X)
            for m in range(M):
                keep = (s / L >= pw[w, m, 0]) & (s / L <= pw[w, m, 1])
                for q, (i, j) in enumerate([(0, 1), (0, 2), (1, 2)]):
                    r = np.fft.ifft(np.where(keep, X[j] * np.conj(X[i]), 0))
                    full = np.abs(np.concatenate([r[L - (N - 1):], r[:N]]))
                    assert np.isclose(pk[w, m, q], full.max(), rtol=1e-4)
                    if mg[w, m, q] > 1e-4:
                        assert li[w, m, q] == int(np.argmax(full)) - (N - 1)


def test_helper_applies_the_bounds_per_window_and_pair():
    N, W, M = 16, 2, 2
    iq, _ = synth.make_windows(W, 3, N, 10e6, seed=3)
    lb = np.array([[[-3, 2], [0, 0], [-15, 15]], [[4, 9], [-2, -1], [1, 1]]], np.int32)
    li, _, _, _, _ = br.bands_batch(iq, [[-0.5, 0.5], [0.0, 0.25]], False, lb)
    for m in range(M):
        assert np.all(li[:, m] >= lb[..., 0]) and np.all(li[:, m] <= lb[..., 1])


# -- the binding -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [None, np.zeros(2), np.zeros((4, 3)), np.zeros((4, 2, 2)), np.zeros((5, 0, 2)), np.zeros((65, 2)),
                                 np.zeros((5, 65, 2)), np.array([[np.nan, 0.1]]), np.array([[-0.1, np.inf]]),
                                 np.array([[-0.6, 0.1]]), np.array([[-0.1, 0.51]]), np.array([[0.2, 0.1]]),
                                 np.array([["a", "b"]])])
def test_check_bands_rejects_bad_band_sets_before_any_call(bad):
    with pytest.raises(ValueError):
        xcorr.check_bands(bad, 5)

    class NoCall(xcorr.XcorrEngine):
        def __init__(self):   # no library, no ctx: a C call would fail with AttributeError, not ValueError
            self.n_buoys, self.n_samples = 3, 16

        def _check_iq(self, iq):
            return iq, 0

        def __del__(self):
            pass
    with pytest.raises(ValueError):
        NoCall().correlate_bands(np.zeros((5, 3, 16), np.complex64), bad)


def test_check_bands_accepts_both_forms():
    a, pw = xcorr.check_bands([[-0.5, 0.5], [0.1, 0.2]], 5)
    assert a.dtype == np.float64 and a.shape == (2, 2) and not pw
    a, pw = xcorr.check_bands(np.zeros((5, 64, 2), np.float32), 5)
    assert a.shape == (5, 64, 2) and a.flags.c_contiguous and pw
    a, pw = xcorr.check_bands(np.zeros((2, 2)), 2)       # [M][2] with M == 2, never [W][2]: shared
    assert not pw


def test_header_declares_and_library_exports_the_bands_entry(lib):
    hdr = open(os.path.join(ROOT, "include", "rmx.h")).read()
    assert "int rmx_xcorr_batch_bands(" in hdr and "int n_bands, int bands_per_window" in hdr
    assert "rmx_xcorr_batch_bands" in xcorr.EXPORTS
    assert hasattr(lib, "rmx_xcorr_batch_bands")


def test_null_ctx_is_rejected(lib):
    band = (C.c_double * 4)(-0.1, 0.1, 0.2, 0.3)
    li, lf, pk = C.c_int32(), C.c_float(), C.c_float()
    rc = lib.rmx_xcorr_batch_bands(None, C.byref(li), 1, None, 0, band, 2, 0, 1, None, 0, C.byref(li), C.byref(lf), C.byref(pk), 0)
    assert rc == -1   # RMX_E_INVAL


class _Stub:
    def __init__(self, b, n, w, device=0):
        self.calls = []

    def correlate_bands(self, iq, bands, pairs=None, lag_bounds=None, whiten=False):
        self.calls.append((np.asarray(bands).shape, None if lag_bounds is None else np.asarray(lag_bounds).shape, whiten))
        W = iq.shape[0]
        b = br.per_window(bands, W)
        li = np.broadcast_to(np.rint(b[..., 0] * 1000).astype(np.int32)[..., None], b.shape[:2] + (3,))   # band lo * 1000
        return li, np.zeros(li.shape, np.float32), np.full(li.shape, float(whiten), np.float32)

    def close(self):
        pass


def test_multi_engine_shards_windows_and_slices_per_window_band_sets():
    m = multi.MultiXcorrEngine(3, 16, 10, devices=[0, 1, 2], engine_factory=_Stub)
    iq = np.zeros((10, 3, 16), np.complex64)
    bands = np.zeros((10, 2, 2))
    bands[:, 0, 0] = -np.arange(10) / 1000.0
    bands[:, 1, 0] = -np.arange(10) / 1000.0 - 0.1
    bands[..., 1] = 0.5
    lb = np.zeros((10, 3, 2), np.int32)
    li, lf, pk = m.correlate_bands(iq, bands, lag_bounds=lb, whiten=True)
    assert li.shape == lf.shape == pk.shape == (10, 2, 3) and li.dtype == np.int32
    assert np.array_equal(li[:, 0], np.broadcast_to(-np.arange(10)[:, None], (10, 3)))
    assert np.array_equal(li[:, 1], np.broadcast_to(-np.arange(10)[:, None] - 100, (10, 3)))
    assert np.all(pk == 1.0)
    assert [e.calls[-1] for e in m._engines] == [((4, 2, 2), (4, 3, 2), True), ((3, 2, 2), (3, 3, 2), True), ((3, 2, 2), (3, 3, 2), True)]
    li, _, _ = m.correlate_bands(iq, [[-0.003, 0.1]])
    assert li.shape == (10, 1, 3) and np.all(li == -3)
    assert all(e.calls[-1] == ((1, 2), None, False) for e in m._engines)
    with pytest.raises(ValueError):
        m.correlate_bands(iq, np.zeros((9, 2, 2)))
    m.close()


# -- measure_lags ------------------------------------------------------------------------------------------------------
def test_measure_lags_bands_argument_errors_and_shapes(monkeypatch):
    calc = tp.TDoACalculator()
    eng = _Stub(3, 16, 8)
    monkeypatch.setattr(calc, "_engine", lambda b, n, w=1: eng)
    iq = np.zeros((4, 3, 16), np.complex64)
    bands = np.zeros((4, 2, 2))
    bands[..., 1] = 0.25
    for kw in ({"band": [-0.1, 0.1]}, {"integrate": 2}, {"refine": 4}, {"quality": True}, {"doppler_cps": [0.0, 1e-4]}):
        with pytest.raises(ValueError, match="bands and " + next(iter(kw))):
            calc.measure_lags(iq, bands=bands, **kw)
    for bad in (np.zeros((2, 2)), np.zeros((3, 2, 2)), np.zeros((4, 2, 3))):
        with pytest.raises(ValueError):
            calc.measure_lags(iq, bands=bad)
    assert not eng.calls
    li, lf, pk = calc.measure_lags(iq, bands=bands, whiten=True)
    assert li.shape == (4, 2, 3) and eng.calls[-1] == ((4, 2, 2), None, True)
    chan = np.zeros((2, 2, 3, 16), np.complex64)             # [C][W][B][N] with [C][W][M][2] and [C][W][P][2]
    li, lf, pk = calc.measure_lags(chan, bands=bands.reshape(2, 2, 2, 2), lag_bounds=np.zeros((2, 2, 3, 2), np.int32))
    assert li.shape == (2, 2, 2, 3) and eng.calls[-1] == ((4, 2, 2), (4, 3, 2), False)


# -- the seam: share_captures ------------------------------------------------------------------------------------------
FS = 2.048e6
FC = 121.0e6


def _processor(**kw):
    p = tp.TDoAProcessor(band_limit=True, **kw)
    for b in (tp.BuoyPosition("A", 37.0, -122.0, 0.0, 100), tp.BuoyPosition("B", 37.0, -121.9, 0.0, 200),
              tp.BuoyPosition("C", 37.2, -122.0, 0.0, 50)):
        p.register_buoy(b)
    return p


def _dets(f_mhz, capture, bw=20e3):
    return [tp.SignalDetection(b, f_mhz, -60.0, "t", 0, 0, 0, 0.9, iq_samples=capture[k], sample_rate_hz=FS, center_freq_hz=FC,
                               bandwidth_hz=bw) for k, b in enumerate("ABC")]


def _run(p, dets):
    """the processor over `dets` with a recording engine: (the engine's calls, {frequency: [lag per measurement]})"""
    calls, groups = [], {}

    class Eng:
        def correlate(self, iq, pairs=None, lag_bounds=None, band=None, whiten=False):
            calls.append(("correlate", iq.shape, None if band is None else np.asarray(band).copy()))
            lo = np.rint(np.asarray(band)[:, 0] * 1000).astype(np.int32)
            return np.broadcast_to(lo[:, None], (iq.shape[0], 3)).copy(), np.zeros((iq.shape[0], 3), np.float32), None

        def correlate_bands(self, iq, bands, pairs=None, lag_bounds=None, whiten=False):
            calls.append(("correlate_bands", iq.shape, np.asarray(bands).copy(),
                          None if lag_bounds is None else np.asarray(lag_bounds).copy()))
            lo = np.rint(np.asarray(bands)[..., 0] * 1000).astype(np.int32)
            li = np.broadcast_to(lo[..., None], lo.shape + (3,)).copy()
            return li, np.zeros(li.shape, np.float32), None
    p.tdoa_calculator._engine = lambda b, n, w=1: Eng()
    p.hyperbolic_positioner.triangulate_position = lambda meas, pos: groups.__setitem__(
        meas[0].frequency_mhz, [m.time_difference_ns for m in meas])
    p.process_signal_detections(dets)
    return calls, groups


def test_share_captures_is_off_by_default():
    assert tp.TDoACalculator().share_captures is False and tp.TDoAProcessor().tdoa_calculator.share_captures is False
    assert tp.TDoAProcessor(share_captures=True).tdoa_calculator.share_captures is True


def test_share_captures_merges_groups_over_one_capture_into_one_banded_window():
    rng = np.random.default_rng(1)
    cap = (rng.standard_normal((3, 256)) + 1j * rng.standard_normal((3, 256))).astype(np.complex64)
    dets = _dets(121.5, cap) + _dets(121.2, cap)
    calls, merged = _run(_processor(share_captures=True), dets)
    assert len(calls) == 1 and calls[0][0] == "correlate_bands"
    assert calls[0][1] == (1, 3, 256) and calls[0][2].shape == (1, 2, 2) and calls[0][3] is None      # W = 1, M = 2
    assert np.allclose(calls[0][2][0], [[(121.5e6 - 10e3 - FC) / FS, (121.5e6 + 10e3 - FC) / FS],
                                        [(121.2e6 - 10e3 - FC) / FS, (121.2e6 + 10e3 - FC) / FS]])
    old_calls, separate = _run(_processor(), dets)
    assert len(old_calls) == 1 and old_calls[0][0] == "correlate" and old_calls[0][1] == (2, 3, 256)
    assert merged == separate and set(merged) == {121.5, 121.2}
    # with bound_lags the bounds ride along once per capture, [W][P][2]
    p = _processor(share_captures=True)
    p.tdoa_calculator.bound_lags = True
    calls, bounded = _run(p, dets)
    assert len(calls) == 1 and calls[0][3].shape == (1, 3, 2)


def test_share_captures_leaves_groups_over_different_captures_to_the_old_call():
    rng = np.random.default_rng(2)
    cap = (rng.standard_normal((2, 3, 256)) + 1j * rng.standard_normal((2, 3, 256))).astype(np.complex64)
    dets = _dets(121.5, cap[0]) + _dets(121.2, cap[1])
    calls, groups = _run(_processor(share_captures=True), dets)
    assert len(calls) == 1 and calls[0][0] == "correlate" and calls[0][1] == (2, 3, 256) and calls[0][2].shape == (2, 2)
    assert set(groups) == {121.5, 121.2}


def test_share_captures_pads_the_narrower_row_and_keeps_the_rest():
    rng = np.random.default_rng(3)
    cap = (rng.standard_normal((3, 3, 256)) + 1j * rng.standard_normal((3, 3, 256))).astype(np.complex64)
    dets = (_dets(121.5, cap[0]) + _dets(121.2, cap[0]) + _dets(121.8, cap[0])      # three emitters in capture 0
            + _dets(121.4, cap[1]) + _dets(121.6, cap[1])                           # two in capture 1
            + _dets(121.0, cap[2], bw=10e3))                                        # one alone in capture 2
    calls, merged = _run(_processor(share_captures=True), dets)
    kinds = sorted(c[0] for c in calls)
    assert kinds == ["correlate", "correlate_bands"]
    banded = next(c for c in calls if c[0] == "correlate_bands")
    assert banded[1] == (2, 3, 256) and banded[2].shape == (2, 3, 2)
    assert np.array_equal(banded[2][1, 2], banded[2][1, 1])                         # the padding repeats a band
    plain = next(c for c in calls if c[0] == "correlate")
    assert plain[1] == (1, 3, 256)
    _, separate = _run(_processor(), dets)
    assert merged == separate and len(merged) == 6


@pytest.mark.parametrize("kw", [{"integrate": 2}, {"refine": 4}, {"min_psr": 3.0}, {"doppler_search_hz": (200.0, 100.0)}])
def test_share_captures_stands_back_for_what_the_banded_call_does_not_do(kw):
    cap = np.ones((3, 256), np.complex64)
    seen = []
    p = _processor(share_captures=True, **kw)
    p.tdoa_calculator.measure_lags = lambda *a, **k: seen.append(k) or (_ for _ in ()).throw(ImportError("stub"))
    p.hyperbolic_positioner.triangulate_position = lambda meas, pos: None
    p.process_signal_detections(_dets(121.5, cap) + _dets(121.2, cap))
    assert seen and all("bands" not in k for k in seen)
