"""rmx_xcorr_batch_bands_integrated without a GPU: the reference helper (tests/bands_integrated_ref.py) against the
definition, the export and the argument types of the C entry, the calls of the Python binding against a stub library,
every refusal of the binding and of measure_band_lags, the multi-device sharding of whole groups, the share_integrated
merge of TDoAProcessor with a recording engine against the separate calls, the default-off behaviour, and the scenario the
combination is for -- two emitters in disjoint bands heard by receivers with free-running oscillators -- on the float32
reference alone."""
import ctypes as C
import os

import numpy as np
import pytest

import bands_integrated_ref as bi
import bands_quality_ref as bq
import bands_ref as br
import integrated_ref as ir
import quality_ref as qr
import refined_ref as rr
import test_bands_quality_cpu as tq
import weighted_ref as wr
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
@pytest.mark.parametrize("U", [0, 2, 8])
@pytest.mark.parametrize("phat", [False, True])
def test_slot_g_m_is_the_single_band_integrated_reference_with_band_m(U, phat):
    N, W, K, B, M = 32, 6, 3, 3, 3
    iq, _ = synth.make_windows(W, B, N, 10e6, seed=U + 1)
    rng = np.random.default_rng(20 + U + phat)
    bands = tq._bands(rng, (W, M), N)                    # per window: they differ inside every group
    lb = np.array([[[-20, 20], [-31, 31], [-5, 30]], [[-3, 3], [0, 31], [-31, 0]]], np.int32)   # per group
    pairs = [(1, 0), (0, 2), (2, 2)]
    for form, bounds in ((bands, lb), (bands[1], lb[0]), (bands, None)):
        got = bi.bands_integrated_batch(iq, form, K, U, phat, bounds, pairs)
        pw = br.per_window(form, W)
        assert got[0].shape == (W // K, M, 3) and got[6].shape == (W // K, M, 3, 4)
        for m in range(M):
            if U:
                one = rr.refined_batch(iq, U, K, pw[:, m], phat, bounds, pairs)
            else:
                one = ir.integrated_batch(iq, K, pw[:, m], phat, bounds, pairs, with_bound=True)
            for k in range(6):
                assert np.array_equal(got[k][:, m], one[k]), (m, k)
            assert np.array_equal(got[6][:, m], qr.quality_batch(iq, K, pw[:, m], phat, bounds, pairs))
    # integrate = 1 collapses onto the banded quality reference, one band onto the single-band call
    a, b = bi.bands_integrated_batch(iq, bands, 1, U, phat, None, pairs), bq.bands_quality_batch(iq, bands, U, phat, None, pairs)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    one = bi.bands_integrated_batch(iq, bands[:, :1], K, U, phat, lb, pairs)
    many = bi.bands_integrated_batch(iq, bands, K, U, phat, lb, pairs)
    assert one[0].shape == (W // K, 1, 3) and all(np.array_equal(one[k][:, 0], many[k][:, 0]) for k in range(7))
    assert bi.bands_integrated_batch(iq, bands, K, U, phat, lb, pairs, quality=False)[6] is None


# -- the entry ---------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry(lib):
    hdr = open(os.path.join(ROOT, "include", "rmx.h")).read()
    assert "int rmx_xcorr_batch_bands_integrated(" in hdr
    decl = hdr[hdr.index("int rmx_xcorr_batch_bands_integrated("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") == 17                         # 18 arguments
    assert "rmx_xcorr_batch_bands_integrated" in xcorr.EXPORTS
    assert hasattr(lib, "rmx_xcorr_batch_bands_integrated")
    assert len(lib.rmx_xcorr_batch_bands_integrated.argtypes) == 18
    assert lib.rmx_xcorr_batch_bands_integrated.argtypes == (
        lib.rmx_xcorr_batch_bands_quality.argtypes[:5] + [C.c_int] + lib.rmx_xcorr_batch_bands_quality.argtypes[5:])


def test_null_ctx_is_rejected(lib):
    band = (C.c_double * 4)(-0.1, 0.1, 0.2, 0.3)
    li, lf, pk = C.c_int32(), C.c_float(), C.c_float()
    q = (C.c_float * 4)()
    for K, refine, qp in ((2, 4, None), (1, 0, q), (2, 0, None)):
        rc = lib.rmx_xcorr_batch_bands_integrated(None, C.byref(li), 2, None, 0, K, band, 2, 0, 1, None, 0, refine, C.byref(li),
                                                  C.byref(lf), C.byref(pk), qp, 0)
        assert rc == -1   # RMX_E_INVAL


# -- the binding -------------------------------------------------------------------------------------------------------
class _Lib(tq._Lib):
    """the three banded entries, recording their arguments"""
    def rmx_xcorr_batch_bands_integrated(self, ctx, iq, W, pp, P, K, bd, M, pw, wt, lb, lb_pg, U, li, lf, pk, ql, flags):
        return self._fill("bands_integrated", (W, P, K, M, pw, wt, lb is not None, lb_pg, U, ql is not None, flags), (W // K, M, P), U,
                          (li, lf, pk, ql))


def test_binding_makes_todays_calls_with_integrate_1_and_the_new_one_above():
    lib = _Lib()
    eng = tq._Engine(lib)
    iq = np.zeros((6, 3, 16), np.complex64)
    bands = np.zeros((6, 2, 2))
    bands[..., 1] = 0.25
    out = eng.correlate_bands(iq, bands, whiten=True, integrate=1)
    assert len(out) == 3 and out[0].shape == (6, 2, 3) and lib.calls[-1] == ("bands", (6, 3, 2, 1, 1, False, 0, 0))
    out = eng.correlate_bands(iq, bands[0], refine=4, lag_bounds=np.zeros((3, 2), np.int32), integrate=1)
    assert lib.calls[-1] == ("bands_quality", (6, 3, 2, 0, 0, True, 0, 4, False, 0))
    out = eng.correlate_bands(iq, bands, quality=True, integrate=1)
    assert len(out) == 4 and lib.calls[-1] == ("bands_quality", (6, 3, 2, 1, 0, False, 0, 0, True, 0))
    # integrate > 1: the new entry, results per group, bounds per group, bands per window
    out = eng.correlate_bands(iq, bands, integrate=3)
    assert len(out) == 3 and out[0].shape == (2, 2, 3) and out[0].dtype == np.int32
    assert lib.calls[-1] == ("bands_integrated", (6, 3, 3, 2, 1, 0, False, 0, 0, False, 0))
    out = eng.correlate_bands(iq, bands[0], pairs=[(1, 0), (2, 2)], whiten=True, refine=8, quality=True, integrate=2,
                              lag_bounds=np.zeros((3, 2, 2), np.int32))
    assert [o.shape for o in out] == [(3, 2, 2)] * 3 + [(3, 2, 2, 4)] and np.all(out[0] == 9) and np.all(out[3] == 0.5)
    assert lib.calls[-1] == ("bands_integrated", (6, 2, 2, 2, 0, 1, True, 1, 8, True, 0))
    out = eng.correlate_bands(iq, bands, integrate=6, lag_bounds=np.zeros((3, 2), np.int32))
    assert out[0].shape == (1, 2, 3) and lib.calls[-1] == ("bands_integrated", (6, 3, 6, 2, 1, 0, True, 0, 0, False, 0))
    # every refusal of the binding, before any call into the library
    n = len(lib.calls)
    for bad in (0, -1, 4, 5, 1.5, "2", True):
        with pytest.raises(ValueError):
            eng.correlate_bands(iq, bands, integrate=bad)
        with pytest.raises(ValueError):
            eng.correlate_bands_device(1, 6, bands, 2, 3, 4, integrate=bad)
    with pytest.raises(ValueError):                                       # per-WINDOW bounds under integration
        eng.correlate_bands(iq, bands, integrate=2, lag_bounds=np.zeros((6, 3, 2), np.int32))
    with pytest.raises(ValueError):                                       # per-GROUP bands
        eng.correlate_bands(iq, np.zeros((3, 2, 2)), integrate=2)
    with pytest.raises(ValueError):
        eng.correlate_bands(iq, bands, integrate=2, refine=3)
    with pytest.raises(ValueError):
        eng.correlate_bands(iq, np.zeros((6, 65, 2)), integrate=2)
    assert len(lib.calls) == n
    out = eng.correlate_bands(iq[:0], bands[0], refine=2, quality=True, integrate=1)
    assert [o.shape for o in out] == [(0, 2, 3)] * 3 + [(0, 2, 3, 4)] and len(lib.calls) == n


def test_device_binding_passes_integrate():
    lib = _Lib()
    lib._fill = lambda name, args, *a: lib.calls.append((name, args)) or 0
    eng = tq._Engine(lib)
    bands = [[-0.1, 0.1], [0.2, 0.3]]
    dev = xcorr.RMX_IN_DEVICE | xcorr.RMX_OUT_DEVICE
    eng.correlate_bands_device(64, 8, bands, 128, 256, 512, integrate=1)
    assert lib.calls[-1] == ("bands", (8, 3, 2, 0, 0, False, 0, dev))
    eng.correlate_bands_device(64, 8, bands, 128, 256, 512, u8=True, whiten=True, refine=8, integrate=4,
                               lag_bounds=np.zeros((2, 3, 2), np.int32))
    assert lib.calls[-1] == ("bands_integrated", (8, 3, 4, 2, 0, 1, True, 1, 8, False, dev | xcorr.RMX_IN_U8))
    eng.correlate_bands_device(64, 8, bands, 128, 256, 512, quality_ptr=1024, integrate=2)
    assert lib.calls[-1] == ("bands_integrated", (8, 3, 2, 2, 0, 0, False, 0, 0, True, dev))


# -- multi-device, measure_band_lags ---------------------------------------------------------------------------------------
class _Stub:
    """correlate_bands with integrate: lag_int = 1000 * the lower edge of the band of each group's FIRST window"""
    def __init__(self, b=3, n=16, w=8, device=0):
        self.calls = []
        self.max_windows = w

    def correlate_bands(self, iq, bands, pairs=None, lag_bounds=None, whiten=False, **more):
        assert set(more) <= {"refine", "quality", "integrate"}
        K = more.get("integrate", 1)
        assert iq.shape[0] % K == 0 and iq.shape[0] <= self.max_windows
        self.calls.append((iq.shape[0], np.asarray(bands).shape, None if lag_bounds is None else np.asarray(lag_bounds).shape, whiten,
                           more))
        b = br.per_window(bands, iq.shape[0])[::K]
        li = np.broadcast_to(np.rint(b[..., 0] * 1000).astype(np.int32)[..., None], b.shape[:2] + (3,)) + more.get("refine", 0)
        out = (li, np.zeros(li.shape, np.float32), np.ones(li.shape, np.float32))
        return out + (np.full(li.shape + (4,), 0.25, np.float32),) if more.get("quality") else out

    def close(self):
        pass


def test_multi_engine_shards_whole_groups():
    m = multi.MultiXcorrEngine(3, 16, 12, devices=[0, 1, 2], engine_factory=_Stub)
    iq = np.zeros((12, 3, 16), np.complex64)
    bands = np.zeros((12, 2, 2))
    bands[:, 0, 0] = -np.arange(12) / 1000.0
    bands[..., 1] = 0.5
    out = m.correlate_bands(iq, bands, integrate=1)
    assert len(out) == 3 and out[0].shape == (12, 2, 3) and all(e.calls[-1][4] == {} for e in m._engines)
    out = m.correlate_bands(iq, bands, integrate=2, refine=4, quality=True, lag_bounds=np.zeros((6, 3, 2), np.int32))
    assert len(out) == 4 and out[0].shape == (6, 2, 3) and out[3].shape == (6, 2, 3, 4)
    assert np.array_equal(out[0][:, 0, 0], 4 - 2 * np.arange(6))          # group g starts at window 2 g
    assert [e.calls[-1][:3] for e in m._engines] == [(4, (4, 2, 2), (2, 3, 2))] * 3
    assert all(e.calls[-1][4] == {"refine": 4, "quality": True, "integrate": 2} for e in m._engines)
    out = m.correlate_bands(iq, bands[0], integrate=4)                    # three groups, one per device; shared bands whole
    assert out[0].shape == (3, 2, 3) and [e.calls[-1][:2] for e in m._engines] == [(4, (2, 2))] * 3
    with pytest.raises(ValueError):
        m.correlate_bands(iq, bands, integrate=5)
    with pytest.raises(ValueError, match="more than one device's engine holds"):
        m.correlate_bands(iq, bands, integrate=6)                         # an engine holds 12 / 3 = 4 windows
    m.close()


def test_measure_band_lags_takes_integrate_and_measure_lags_keeps_its_refusals(monkeypatch):
    calc = tp.TDoACalculator()
    eng = _Stub(w=64)
    monkeypatch.setattr(calc, "_engine", lambda b, n, w=1: eng)
    iq = np.zeros((4, 3, 16), np.complex64)
    bands = np.zeros((4, 2, 2))
    bands[..., 1] = 0.25
    for bad in (0, 3, -2, 1.5, "2"):
        with pytest.raises(ValueError):
            calc.measure_band_lags(iq, bands, integrate=bad)
    with pytest.raises(ValueError):
        calc.measure_band_lags(iq, np.zeros((2, 2, 2)), integrate=2)      # bands stay per window
    assert not eng.calls
    out = calc.measure_band_lags(iq, bands, whiten=True, integrate=1)
    assert len(out) == 3 and out[0].shape == (4, 2, 3) and eng.calls[-1][4] == {}
    out = calc.measure_band_lags(iq, bands, refine=8, quality=True, integrate=2, lag_bounds=np.zeros((2, 3, 2), np.int32))
    assert [o.shape for o in out] == [(2, 2, 3)] * 3 + [(2, 2, 3, 4)]
    assert eng.calls[-1] == (4, (4, 2, 2), (2, 3, 2), False, {"refine": 8, "quality": True, "integrate": 2})
    chan = np.zeros((2, 4, 3, 16), np.complex64)          # [C][W][B][N]: groups never straddle two channels
    out = calc.measure_band_lags(chan, np.tile(bands, (2, 1, 1, 1)), integrate=2, lag_bounds=np.zeros((2, 2, 3, 2), np.int32))
    assert [o.shape for o in out] == [(2, 2, 2, 3)] * 3 and eng.calls[-1][:3] == (8, (8, 2, 2), (4, 3, 2))
    with pytest.raises(ValueError):
        calc.measure_band_lags(np.zeros((2, 3, 3, 16), np.complex64), np.zeros((2, 3, 2, 2)), integrate=2)
    for kw in ({"integrate": 2}, {"refine": 4}, {"quality": True}):
        with pytest.raises(ValueError, match="bands and "):
            calc.measure_lags(iq, bands=bands, **kw)


# -- the seam: share_integrated ------------------------------------------------------------------------------------------
def _run(p, dets):
    """the processor over `dets` with a recording engine that takes integrate: (calls, {frequency: measurements}).  A lag is
    1000 * the lower edge of the band of the group's first segment (+ refine); psr and coherence as tq._figures."""
    calls, groups = [], {}

    class Eng:
        def correlate(self, iq, pairs=None, lag_bounds=None, band=None, whiten=False, **more):
            assert set(more) <= {"refine", "quality", "integrate"}
            K = more.get("integrate", 1)
            calls.append(("correlate", iq.copy(), np.asarray(band).copy(), None if lag_bounds is None else np.asarray(lag_bounds).copy(),
                          more))
            lo = np.rint(np.asarray(band)[::K, 0] * 1000).astype(np.int32)
            li = np.broadcast_to(lo[:, None], (iq.shape[0] // K, 3)) + more.get("refine", 0)
            out = (li.copy(), np.zeros(li.shape, np.float32), None)
            return out + (tq._figures(lo),) if more.get("quality") else out

        def correlate_bands(self, iq, bands, pairs=None, lag_bounds=None, whiten=False, **more):
            assert set(more) <= {"refine", "quality", "integrate"}
            K = more.get("integrate", 1)
            calls.append(("correlate_bands", iq.copy(), np.asarray(bands).copy(),
                          None if lag_bounds is None else np.asarray(lag_bounds).copy(), more))
            lo = np.rint(np.asarray(bands)[::K, :, 0] * 1000).astype(np.int32)
            li = np.broadcast_to(lo[..., None], lo.shape + (3,)) + more.get("refine", 0)
            out = (li.copy(), np.zeros(li.shape, np.float32), None)
            return out + (tq._figures(lo),) if more.get("quality") else out
    p.tdoa_calculator._engine = lambda b, n, w=1: Eng()
    p.hyperbolic_positioner.triangulate_position = lambda meas, pos: groups.__setitem__(
        meas[0].frequency_mhz, [(m.buoy1_id, m.buoy2_id, m.time_difference_ns, m.confidence) for m in meas])
    p.process_signal_detections(dets)
    return calls, groups


def test_share_integrated_is_off_by_default():
    assert tp.TDoACalculator().share_integrated is False and tp.TDoAProcessor().tdoa_calculator.share_integrated is False
    assert tp.TDoAProcessor(share_integrated=True).tdoa_calculator.share_integrated is True


@pytest.mark.parametrize("kw, more", [({}, {}), ({"refine": 4}, {"refine": 4}), ({"min_psr": 10.0}, {"quality": True}),
                                      ({"refine": 4, "min_psr": 10.0, "correlation_confidence": True}, {"refine": 4, "quality": True})])
@pytest.mark.parametrize("bound_lags", [False, True])
def test_share_integrated_sends_one_banded_call_and_gives_the_measurements_of_the_separate_calls(kw, more, bound_lags):
    K = 2
    cap = tq._capture(1)
    dets = tq._dets(121.5, cap) + tq._dets(121.2, cap)

    def run(**flags):
        p = tq._processor(integrate=K, **flags, **kw)
        p.tdoa_calculator.bound_lags = bound_lags
        p.tdoa_calculator.min_cut_samples = 16
        return _run(p, dets)
    calls, merged = run(share_captures=True, share_qualified=True, share_integrated=True)
    old_calls, separate = run(share_captures=False)
    assert len(calls) == 1 and calls[0][0] == "correlate_bands" and calls[0][4] == dict(more, integrate=K)
    assert len(old_calls) == 1 and old_calls[0][0] == "correlate" and old_calls[0][4] == dict(more, integrate=K)
    # the capture is cut ONCE, exactly as the separate calls cut it: K segments of 128 samples; the separate call holds
    # the same segments once per emitter
    assert calls[0][1].shape == (K, 3, 128) and old_calls[0][1].shape == (2 * K, 3, 128)
    assert np.array_equal(calls[0][1], old_calls[0][1][:K]) and np.array_equal(calls[0][1], old_calls[0][1][K:])
    # each member's band repeated over its K segments: bands[s][m] is the separate call's band of (member m, segment s)
    assert calls[0][2].shape == (K, 2, 2)
    for m in range(2):
        assert np.array_equal(calls[0][2][:, m], old_calls[0][2][m * K:(m + 1) * K])
    # lag bounds per group, as today
    assert (calls[0][3] is None) == (not bound_lags)
    if bound_lags:
        assert calls[0][3].shape == (1, 3, 2) and old_calls[0][3].shape == (2, 3, 2) and np.array_equal(calls[0][3][0], old_calls[0][3][0])
    assert merged == separate and list(merged) == list(separate) and set(merged) == {121.5, 121.2}
    if "min_psr" in kw:
        assert len(merged[121.2]) == 2 and len(merged[121.5]) == 3
    # without share_integrated the sharing flags stand back for integration exactly as before, call for call
    for flags in ({"share_captures": True}, {"share_captures": True, "share_qualified": True}):
        off_calls, off = run(**flags)
        assert off == separate and len(off_calls) == len(old_calls)
        for a, b in zip(off_calls, old_calls):
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[4] == b[4]
    # with refine or quality it needs share_qualified
    if more:
        off_calls, off = run(share_captures=True, share_integrated=True)
        assert off == separate and [c[0] for c in off_calls] == ["correlate"]


def test_share_integrated_keeps_the_segment_length_checks_and_leaves_the_doppler_search_out():
    cap = tq._capture(2)
    dets = tq._dets(121.5, cap) + tq._dets(121.2, cap)
    p = tq._processor(integrate=4, share_captures=True, share_integrated=True)      # 256 / 4 = 64 < min_cut_samples = 128
    calls, groups = _run(p, dets)
    assert calls == [] and groups == {}
    with pytest.raises(ValueError, match="doppler_search_hz and integrate"):
        tq._processor(integrate=2, share_captures=True, share_integrated=True, doppler_search_hz=(200.0, 100.0))
    seen = []
    p = tq._processor(share_captures=True, share_integrated=True, doppler_search_hz=(200.0, 100.0))
    p.tdoa_calculator.measure_lags = lambda *a, **k: seen.append(k) or (_ for _ in ()).throw(ImportError("stub"))
    p.tdoa_calculator.measure_band_lags = lambda *a, **k: seen.append({"bands": 1}) or (_ for _ in ()).throw(ImportError("stub"))
    p.hyperbolic_positioner.triangulate_position = lambda meas, pos: None
    p.process_signal_detections(dets)
    assert seen and all("bands" not in k for k in seen)


# -- the scenario, on the float32 reference alone ------------------------------------------------------------------------
SCENE = dict(n=4096, K=16, seed=4, snr_db=-9.0, delays=((0, 9, -14), (0, -21, 6)), cycles=((0, 3, 8), (0, -5, 4)),
             bands=((-0.45, -0.05), (0.05, 0.45)))


def two_emitter_offset_scene(n, K, seed, snr_db, delays, cycles, bands):
    """three buoys, two emitters in disjoint bands, each with its own per-receiver frequency offset (cycles over the n
    samples) and its own delays, in unit-variance noise: [B][n] complex64"""
    rng = np.random.default_rng(seed)
    pad = 64
    t = np.arange(n)
    out = (rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))) / np.sqrt(2.0)
    for e in range(2):
        s = wr.band_signal(rng, n + 2 * pad, *bands[e])
        for b in range(3):
            d = delays[e][b]
            out[b] += 10 ** (snr_db / 20) * s[pad - d: pad - d + n] * np.exp(2j * np.pi * cycles[e][b] / n * t)
    return out.astype(np.complex64)


def test_two_emitters_with_frequency_offsets_need_bands_and_integration():
    """The single-window banded reference misses at least half of the (band, pair) integer lags; the integrated reference
    with K segments finds all of them with top-two margin > 1e-5.  The counts are printed."""
    s = SCENE
    x = two_emitter_offset_scene(**s)
    bands = np.array(s["bands"])
    true = np.array([[d[j] - d[i] for i in range(3) for j in range(i + 1, 3)] for d in s["delays"]])     # [M][P]
    one = bq.bands_quality_batch(x[None], bands, 0, quality=False)
    seg = ir.segments(x, s["K"])
    many = bi.bands_integrated_batch(seg, bands, s["K"], 0, quality=False)
    hit_one, hit_many = int((one[0][0] == true).sum()), int((many[0][0] == true).sum())
    print("single window: %d of 6 integer lags; %d integrated segments: %d of 6, smallest top-two margin %.3e"
          % (hit_one, s["K"], hit_many, float(many[3].min())))
    assert hit_one <= 3
    assert hit_many == 6 and np.all(many[3] > 1e-5)
