"""rmx_xcorr_batch_bands_quality without a GPU: the reference helper (tests/bands_quality_ref.py) against the definition
and against a direct float64 restatement, the fine grid at the edges of a lag interval, the checks and the calls of the
Python binding against a stub library, the export and NULL-ctx check of the C entry, measure_band_lags, the multi-device
pass-through and the share_qualified merge of TDoAProcessor with a recording engine."""
import ctypes as C
import os

import numpy as np
import pytest

import bands_quality_ref as bq
import bands_ref as br
import quality_ref as qr
import refined_ref as rr
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


def _bands(rng, shape, N):
    L = 2 * N
    a = rng.uniform(-0.5, 0.5 - 6.0 / L, size=shape)
    return np.stack([a, np.minimum(a + rng.uniform(4.0 / L, 0.6, size=shape), 0.5)], -1)


# -- the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", [0, 2, 8])
@pytest.mark.parametrize("phat", [False, True])
def test_slot_w_m_is_the_single_band_reference_with_band_w_m(U, phat):
    N, W, B, M = 32, 3, 3, 3
    iq, _ = synth.make_windows(W, B, N, 10e6, seed=U + 1)
    rng = np.random.default_rng(10 + U + phat)
    bands = _bands(rng, (W, M), N)
    lb = np.array([[-20, 20], [-31, 31], [-5, 30]], np.int32)
    pairs = [(1, 0), (0, 2), (2, 2)]
    for form in (bands, bands[1]):
        got = bq.bands_quality_batch(iq, form, U, phat, lb, pairs)
        pw = br.per_window(form, W)
        assert got[0].shape == (W, M, 3) and got[6].shape == (W, M, 3, 4)
        for m in range(M):
            if U:
                one = rr.refined_batch(iq, U, 1, pw[:, m], phat, lb, pairs)
            else:
                one = bq.wr.weighted_batch(iq, pw[:, m], phat, lb, pairs, with_bound=True)
            for k in range(6):
                assert np.array_equal(got[k][:, m], one[k]), (m, k)
            assert np.array_equal(got[6][:, m], qr.quality_batch(iq, 1, pw[:, m], phat, lb, pairs))
    # one band collapses onto the single-band call
    one = bq.bands_quality_batch(iq, bands[:, :1], U, phat, lb, pairs)
    many = bq.bands_quality_batch(iq, bands, U, phat, lb, pairs)
    assert one[0].shape == (W, 1, 3) and all(np.array_equal(one[k][:, 0], many[k][:, 0]) for k in range(7))
    assert bq.bands_quality_batch(iq, bands, U, phat, lb, pairs, quality=False)[6] is None


@pytest.mark.parametrize("phat", [False, True])
def test_reference_against_a_direct_float64_restatement(phat):
    """the fine taps as a direct sum over the kept bins, the figures from the masked spectra: nothing of the helpers"""
    N, W, B, M, U, L = 32, 2, 3, 3, 4, 64
    iq, _ = synth.make_windows(W, B, N, 10e6, seed=5, snr_db=15, bandwidth=0.8, max_delay=4)
    rng = np.random.default_rng(3)
    bands = _bands(rng, (W, M), N)
    li, lf, pk, mg, fm, fb, qual = bq.bands_quality_batch(iq, bands, U, phat)
    s = np.fft.fftfreq(L, 1.0 / L)
    for w in range(W):
        X = np.fft.fft(iq[w].astype(np.complex128), L, axis=-1)
        if phat:
            X = X / np.abs(X)
        for m in range(M):
            keep = (s / L >= bands[w, m, 0]) & (s / L <= bands[w, m, 1])
            for q, (i, j) in enumerate([(0, 1), (0, 2), (1, 2)]):
                p = np.where(keep, X[j] * np.conj(X[i]), 0)
                r = np.fft.ifft(p)
                full = np.abs(np.concatenate([r[L - (N - 1):], r[:N]]))
                if mg[w, m, q] <= 1e-4:
                    continue
                lag0 = int(np.argmax(full)) - (N - 1)
                t = lag0 + np.arange(-U, U + 1) / U
                if lag0 == -(N - 1):
                    t = t[U:]
                if lag0 == N - 1:
                    t = t[:U + 1]
                f = np.abs((p[None, :] * np.exp(2j * np.pi * s[None, :] * t[:, None] / L)).sum(axis=1)) / L
                assert np.isclose(pk[w, m, q], f.max(), rtol=1e-4)
                assert abs(li[w, m, q] + lf[w, m, q] - t[np.argmax(f)]) <= 1.0 / U
                ai, aj = np.abs(np.where(keep, X[i], 0)), np.abs(np.where(keep, X[j], 0))
                d = ai * aj
                want = (min(full.max() / np.sqrt((ai ** 2).sum() / L * (aj ** 2).sum() / L), 1.0),
                        np.sqrt(((s / L) ** 2 * d).sum() / d.sum()), d.sum() ** 2 / (d ** 2).sum())
                assert np.allclose(qual[w, m, q, [qr.COHERENCE, qr.RMS_BW, qr.NEFF]], want, rtol=1e-4)
                et = (d ** 2).sum() / L
                assert np.isclose(qr.et_over_p2(qual[w, m, q], N), et / full.max() ** 2, rtol=1e-4)


def test_a_lag_on_lo_or_hi_admits_one_side_of_the_fine_grid():
    N, W, M, U = 32, 2, 2, 8
    iq, _ = synth.make_windows(W, 3, N, 10e6, seed=9, snr_db=15, bandwidth=0.8, max_delay=4)
    bands = np.array([[-0.4, 0.4], [-0.1, 0.3]])
    free = bq.bands_quality_batch(iq, bands, 0, quality=False)
    assert np.all(free[3] > 1e-5)
    lag0 = free[0]                                      # [W][M][P]: per band, so bound per band through separate calls
    for m in range(M):
        for side in (0, 1):
            lb = np.stack([lag0[:, m] - (0 if side == 0 else 6), lag0[:, m] + (6 if side == 0 else 0)], -1).astype(np.int32)
            li, lf, pk, _, _, _, _ = bq.bands_quality_batch(iq, bands, U, lag_bounds=lb, quality=False)
            lag = li[:, m] + lf[:, m]
            assert np.all(lag >= lb[..., 0]) and np.all(lag <= lb[..., 1])
            # the coarse peak sits on the edge: only u >= 0 (side 0) or u <= 0 (side 1) was admitted
            assert np.all((lag - lag0[:, m]) * (1 if side == 0 else -1) >= 0)
            assert np.all(np.abs(lag - lag0[:, m]) <= 1.0)


# -- the binding -------------------------------------------------------------------------------------------------------
class _Lib:
    """the two banded entries, recording their arguments and filling the outputs with the call's U"""
    def __init__(self):
        self.calls = []

    def _fill(self, name, args, shape, refine, ptrs):
        self.calls.append((name, args))
        for p, t in zip(ptrs[:3], (np.int32, np.float32, np.float32)):
            np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(t))), shape)[:] = refine + 1
        if len(ptrs) > 3 and ptrs[3] is not None:
            np.ctypeslib.as_array(C.cast(ptrs[3], C.POINTER(C.c_float)), shape + (4,))[:] = 0.5
        return 0

    def rmx_xcorr_batch_bands(self, ctx, iq, W, pp, P, bd, M, pw, wt, lb, lb_pw, li, lf, pk, flags):
        return self._fill("bands", (W, P, M, pw, wt, lb is not None, lb_pw, flags), (W, M, P), 0, (li, lf, pk))

    def rmx_xcorr_batch_bands_quality(self, ctx, iq, W, pp, P, bd, M, pw, wt, lb, lb_pw, U, li, lf, pk, ql, flags):
        return self._fill("bands_quality", (W, P, M, pw, wt, lb is not None, lb_pw, U, ql is not None, flags), (W, M, P), U,
                          (li, lf, pk, ql))


class _Engine(xcorr.XcorrEngine):
    def __init__(self, lib):
        self.n_buoys, self.n_samples, self._lib, self._ctx = 3, 16, lib, None

    def _check(self, rc):
        assert rc == 0

    def __del__(self):
        pass


def test_binding_makes_todays_call_by_default_and_the_new_one_on_request():
    lib = _Lib()
    eng = _Engine(lib)
    iq = np.zeros((5, 3, 16), np.complex64)
    bands = np.zeros((5, 2, 2))
    bands[..., 1] = 0.25
    out = eng.correlate_bands(iq, bands, whiten=True)
    assert len(out) == 3 and out[0].shape == (5, 2, 3) and lib.calls[-1] == ("bands", (5, 3, 2, 1, 1, False, 0, 0))
    out = eng.correlate_bands(iq, bands[0], refine=4, lag_bounds=np.zeros((3, 2), np.int32))
    assert len(out) == 3 and np.all(out[0] == 5) and lib.calls[-1] == ("bands_quality", (5, 3, 2, 0, 0, True, 0, 4, False, 0))
    out = eng.correlate_bands(iq, bands, pairs=[(1, 0), (2, 2)], quality=True)
    assert len(out) == 4 and out[3].shape == (5, 2, 2, 4) and out[3].dtype == np.float32 and np.all(out[3] == 0.5)
    assert lib.calls[-1] == ("bands_quality", (5, 2, 2, 1, 0, False, 0, 0, True, 0))
    out = eng.correlate_bands(iq, bands, refine=16, quality=True, lag_bounds=np.zeros((5, 3, 2), np.int32))
    assert lib.calls[-1] == ("bands_quality", (5, 3, 2, 1, 0, True, 1, 16, True, 0)) and np.all(out[1] == 17)
    n = len(lib.calls)
    for bad in (3, -2, 32, 1.5, "4"):
        with pytest.raises(ValueError):
            eng.correlate_bands(iq, bands, refine=bad)
        with pytest.raises(ValueError):
            eng.correlate_bands_device(1, 5, bands, 2, 3, 4, refine=bad)
    with pytest.raises(ValueError):
        eng.correlate_bands(iq, np.zeros((4, 2, 2)), refine=4)
    assert len(lib.calls) == n
    # an empty batch makes no call and still has the four shapes
    out = eng.correlate_bands(iq[:0], bands[0], refine=2, quality=True)
    assert [o.shape for o in out] == [(0, 2, 3)] * 3 + [(0, 2, 3, 4)] and len(lib.calls) == n


def test_device_binding_passes_the_quality_pointer():
    lib = _Lib()
    lib._fill = lambda name, args, *a: lib.calls.append((name, args)) or 0
    eng = _Engine(lib)
    bands = [[-0.1, 0.1], [0.2, 0.3]]
    dev = xcorr.RMX_IN_DEVICE | xcorr.RMX_OUT_DEVICE
    eng.correlate_bands_device(64, 7, bands, 128, 256, 512)
    assert lib.calls[-1] == ("bands", (7, 3, 2, 0, 0, False, 0, dev))
    eng.correlate_bands_device(64, 7, bands, 128, 256, 512, u8=True, whiten=True, refine=8)
    assert lib.calls[-1] == ("bands_quality", (7, 3, 2, 0, 1, False, 0, 8, False, dev | xcorr.RMX_IN_U8))
    eng.correlate_bands_device(64, 7, bands, 128, 256, 512, quality_ptr=1024)
    assert lib.calls[-1] == ("bands_quality", (7, 3, 2, 0, 0, False, 0, 0, True, dev))


def test_header_declares_and_library_exports_the_entry(lib):
    hdr = open(os.path.join(ROOT, "include", "rmx.h")).read()
    assert "int rmx_xcorr_batch_bands_quality(" in hdr
    assert "rmx_xcorr_batch_bands_quality" in xcorr.EXPORTS
    assert hasattr(lib, "rmx_xcorr_batch_bands_quality")
    assert len(lib.rmx_xcorr_batch_bands_quality.argtypes) == 17


def test_null_ctx_is_rejected(lib):
    band = (C.c_double * 4)(-0.1, 0.1, 0.2, 0.3)
    li, lf, pk = C.c_int32(), C.c_float(), C.c_float()
    q = (C.c_float * 4)()
    for refine, qp in ((4, None), (0, q), (0, None)):
        rc = lib.rmx_xcorr_batch_bands_quality(None, C.byref(li), 1, None, 0, band, 2, 0, 1, None, 0, refine, C.byref(li), C.byref(lf),
                                               C.byref(pk), qp, 0)
        assert rc == -1   # RMX_E_INVAL


# -- multi-device, measure_band_lags ---------------------------------------------------------------------------------------
class _Stub:
    """today's correlate_bands, and the new arguments only where they are asked for"""
    def __init__(self, b=3, n=16, w=8, device=0):
        self.calls = []

    def correlate_bands(self, iq, bands, pairs=None, lag_bounds=None, whiten=False, **more):
        assert set(more) <= {"refine", "quality"}
        self.calls.append((np.asarray(bands).shape, None if lag_bounds is None else np.asarray(lag_bounds).shape, whiten, more))
        b = br.per_window(bands, iq.shape[0])
        li = np.broadcast_to(np.rint(b[..., 0] * 1000).astype(np.int32)[..., None], b.shape[:2] + (3,)) + more.get("refine", 0)
        out = (li, np.zeros(li.shape, np.float32), np.ones(li.shape, np.float32))
        return out + (np.full(li.shape + (4,), 0.25, np.float32),) if more.get("quality") else out

    def close(self):
        pass


def test_multi_engine_passes_refine_and_quality_through():
    m = multi.MultiXcorrEngine(3, 16, 10, devices=[0, 1, 2], engine_factory=_Stub)
    iq = np.zeros((10, 3, 16), np.complex64)
    bands = np.zeros((10, 2, 2))
    bands[:, 0, 0] = -np.arange(10) / 1000.0
    bands[..., 1] = 0.5
    out = m.correlate_bands(iq, bands)
    assert len(out) == 3 and all(e.calls[-1][3] == {} for e in m._engines)
    out = m.correlate_bands(iq, bands, refine=4)
    assert len(out) == 3 and np.array_equal(out[0][:, 0, 0], 4 - np.arange(10))
    assert all(e.calls[-1][3] == {"refine": 4} for e in m._engines)
    out = m.correlate_bands(iq, bands, quality=True, lag_bounds=np.zeros((10, 3, 2), np.int32))
    assert len(out) == 4 and out[3].shape == (10, 2, 3, 4) and np.all(out[3] == 0.25)
    assert [e.calls[-1][:2] for e in m._engines] == [((4, 2, 2), (4, 3, 2)), ((3, 2, 2), (3, 3, 2)), ((3, 2, 2), (3, 3, 2))]
    assert all(e.calls[-1][3] == {"refine": 0, "quality": True} for e in m._engines)
    with pytest.raises(ValueError):
        m.correlate_bands(iq, bands, refine=3)
    m.close()


def test_measure_band_lags_shapes_with_and_without_the_channel_axis(monkeypatch):
    calc = tp.TDoACalculator()
    eng = _Stub()
    monkeypatch.setattr(calc, "_engine", lambda b, n, w=1: eng)
    iq = np.zeros((4, 3, 16), np.complex64)
    bands = np.zeros((4, 2, 2))
    bands[..., 1] = 0.25
    for bad in (np.zeros((2, 2)), np.zeros((3, 2, 2)), np.zeros((4, 2, 3))):
        with pytest.raises(ValueError):
            calc.measure_band_lags(iq, bad, refine=4)
    with pytest.raises(ValueError):
        calc.measure_band_lags(iq, bands, refine=5)
    assert not eng.calls
    out = calc.measure_band_lags(iq, bands, whiten=True)
    assert len(out) == 3 and out[0].shape == (4, 2, 3) and eng.calls[-1] == ((4, 2, 2), None, True, {})
    out = calc.measure_band_lags(iq, bands, refine=8, quality=True)
    assert len(out) == 4 and out[3].shape == (4, 2, 3, 4) and eng.calls[-1][3] == {"refine": 8, "quality": True}
    out = calc.measure_band_lags(iq, bands, quality=True)
    assert len(out) == 4 and eng.calls[-1][3] == {"quality": True}
    chan = np.zeros((2, 2, 3, 16), np.complex64)             # [C][W][B][N] with [C][W][M][2] and [C][W][P][2]
    out = calc.measure_band_lags(chan, bands.reshape(2, 2, 2, 2), lag_bounds=np.zeros((2, 2, 3, 2), np.int32), refine=2, quality=True)
    assert [o.shape for o in out] == [(2, 2, 2, 3)] * 3 + [(2, 2, 2, 3, 4)]
    assert eng.calls[-1] == ((4, 2, 2), (4, 3, 2), False, {"refine": 2, "quality": True})
    # measure_lags(bands=...) keeps its refusals
    for kw in ({"refine": 4}, {"quality": True}):
        with pytest.raises(ValueError, match="bands and "):
            calc.measure_lags(iq, bands=bands, **kw)


# -- the seam: share_qualified -----------------------------------------------------------------------------------------
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


def _figures(lo):
    """quality [..][3][4] of a stub call from the bands' lower edges (in 1 / 1000 cycles per sample): psr = |lo| / 10 + pair,
    coherence = 0.5 + 0.1 pair"""
    q = np.zeros(lo.shape + (3, 4), np.float32)
    q[..., 0] = 0.5 + 0.1 * np.arange(3)
    q[..., 1] = np.abs(lo)[..., None] / 10.0 + np.arange(3)
    return q


def _run(p, dets, strict=False):
    """the processor over `dets` with a recording engine: (the engine's calls, {frequency: [(buoys, dt, confidence)]}).
    strict: the engine knows only today's correlate_bands(iq, bands, pairs, lag_bounds, whiten)"""
    calls, groups = [], {}

    class Eng:
        def correlate(self, iq, pairs=None, lag_bounds=None, band=None, whiten=False, **more):
            assert set(more) <= {"refine", "quality"}
            calls.append(("correlate", iq.shape, np.asarray(band).copy(), None if lag_bounds is None else np.asarray(lag_bounds).copy(),
                          more))
            lo = np.rint(np.asarray(band)[:, 0] * 1000).astype(np.int32)
            li = np.broadcast_to(lo[:, None], (iq.shape[0], 3)) + more.get("refine", 0)
            out = (li.copy(), np.zeros(li.shape, np.float32), None)
            return out + (_figures(lo),) if more.get("quality") else out

        def correlate_bands(self, iq, bands, pairs=None, lag_bounds=None, whiten=False, **more):
            assert set(more) <= {"refine", "quality"}
            calls.append(("correlate_bands", iq.shape, np.asarray(bands).copy(),
                          None if lag_bounds is None else np.asarray(lag_bounds).copy(), more))
            lo = np.rint(np.asarray(bands)[..., 0] * 1000).astype(np.int32)
            li = np.broadcast_to(lo[..., None], lo.shape + (3,)) + more.get("refine", 0)
            out = (li.copy(), np.zeros(li.shape, np.float32), None)
            return out + (_figures(lo),) if more.get("quality") else out

    class Strict(Eng):
        def correlate_bands(self, iq, bands, pairs=None, lag_bounds=None, whiten=False):
            return Eng.correlate_bands(self, iq, bands, pairs, lag_bounds, whiten)
    p.tdoa_calculator._engine = lambda b, n, w=1: (Strict() if strict else Eng())
    p.hyperbolic_positioner.triangulate_position = lambda meas, pos: groups.__setitem__(
        meas[0].frequency_mhz, [(m.buoy1_id, m.buoy2_id, m.time_difference_ns, m.confidence) for m in meas])
    p.process_signal_detections(dets)
    return calls, groups


def _capture(seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((3, 256)) + 1j * rng.standard_normal((3, 256))).astype(np.complex64)


def test_share_qualified_is_off_by_default():
    assert tp.TDoACalculator().share_qualified is False and tp.TDoAProcessor().tdoa_calculator.share_qualified is False
    assert tp.TDoAProcessor(share_qualified=True).tdoa_calculator.share_qualified is True


@pytest.mark.parametrize("kw, more", [({"refine": 4}, {"refine": 4}), ({"min_psr": 10.0}, {"quality": True}),
                                      ({"correlation_confidence": True}, {"quality": True}),
                                      ({"refine": 4, "min_psr": 10.0, "correlation_confidence": True}, {"refine": 4, "quality": True})])
@pytest.mark.parametrize("bound_lags", [False, True])
def test_share_qualified_sends_one_banded_call_and_gives_the_measurements_of_the_separate_calls(kw, more, bound_lags):
    cap = _capture(1)
    dets = _dets(121.5, cap) + _dets(121.2, cap)

    def run(**flags):
        p = _processor(**flags, **kw)
        p.tdoa_calculator.bound_lags = bound_lags
        return _run(p, dets)
    calls, merged = run(share_captures=True, share_qualified=True)
    assert len(calls) == 1 and calls[0][0] == "correlate_bands" and calls[0][1] == (1, 3, 256) and calls[0][2].shape == (1, 2, 2)
    assert calls[0][4] == more
    assert (calls[0][3] is None) == (not bound_lags) and (calls[0][3] is None or calls[0][3].shape == (1, 3, 2))
    old_calls, separate = run(share_captures=False)
    assert len(old_calls) == 1 and old_calls[0][0] == "correlate" and old_calls[0][1] == (2, 3, 256) and old_calls[0][4] == more
    assert merged == separate and list(merged) == list(separate) and set(merged) == {121.5, 121.2}
    if "min_psr" in kw:      # psr 9.3 of the first pair at 121.2 MHz lies below 10: dropped on both sides
        assert len(merged[121.2]) == 2 and len(merged[121.5]) == 3
    # the flag off: share_captures stands back exactly as before, call for call
    off_calls, off = run(share_captures=True)
    assert off == separate and len(off_calls) == len(old_calls)
    for a, b in zip(off_calls, old_calls):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[4] == b[4]
        assert (a[3] is None and b[3] is None) or np.array_equal(a[3], b[3])


def test_share_qualified_pads_rows_and_keeps_single_captures():
    cap = [_capture(k) for k in (3, 4, 5)]
    dets = (_dets(121.5, cap[0]) + _dets(121.2, cap[0]) + _dets(121.8, cap[0]) + _dets(121.4, cap[1]) + _dets(121.6, cap[1])
            + _dets(121.0, cap[2], bw=10e3))
    calls, merged = _run(_processor(share_captures=True, share_qualified=True, refine=8, min_psr=12.0), dets)
    assert sorted(c[0] for c in calls) == ["correlate", "correlate_bands"]
    banded = next(c for c in calls if c[0] == "correlate_bands")
    assert banded[1] == (2, 3, 256) and banded[2].shape == (2, 3, 2) and banded[4] == {"refine": 8, "quality": True}
    plain = next(c for c in calls if c[0] == "correlate")
    assert plain[1] == (1, 3, 256) and plain[4] == {"refine": 8, "quality": True}
    _, separate = _run(_processor(refine=8, min_psr=12.0), dets)
    assert merged == separate and list(merged) == list(separate)


def test_share_qualified_with_nothing_requested_makes_todays_banded_call():
    cap = _capture(6)
    dets = _dets(121.5, cap) + _dets(121.2, cap)
    calls, merged = _run(_processor(share_captures=True, share_qualified=True), dets, strict=True)
    ref_calls, ref = _run(_processor(share_captures=True), dets, strict=True)
    assert len(calls) == 1 and calls[0][0] == "correlate_bands" and calls[0][4] == {} and merged == ref
    assert np.array_equal(calls[0][2], ref_calls[0][2])


@pytest.mark.parametrize("kw", [{"integrate": 2}, {"doppler_search_hz": (200.0, 100.0)}, {"integrate": 2, "refine": 4}])
def test_share_qualified_still_stands_back_for_integration_and_the_doppler_search(kw):
    cap = np.ones((3, 256), np.complex64)
    seen = []
    p = _processor(share_captures=True, share_qualified=True, **kw)
    p.tdoa_calculator.measure_lags = lambda *a, **k: seen.append(k) or (_ for _ in ()).throw(ImportError("stub"))
    p.tdoa_calculator.measure_band_lags = lambda *a, **k: seen.append({"bands": 1}) or (_ for _ in ()).throw(ImportError("stub"))
    p.hyperbolic_positioner.triangulate_position = lambda meas, pos: None
    p.process_signal_detections(_dets(121.5, cap) + _dets(121.2, cap))
    assert seen and all("bands" not in k for k in seen)
