"""rmx_caf_batch_bands without a GPU: tests/caf_bands_ref.py pinned against the helper it stacks; the two-emitter facts the
entry exists for, on the reference alone; the conditions on the inputs of every case tests/test_gpu_caf_bands.py holds to
the parity rule (no slot excused, and winners that differ between the bands of a window and between the slots of a call);
the binding's own side on a fake library (the entry name, the argument order, the output shapes, the ValueErrors);
MultiXcorrEngine.caf_bands and TDoAProcessor's share_doppler on stub engines; the export and the header text."""
import os

import numpy as np
import pytest

import caf_bands_ref as br
import caf_ref as cr
import caf_request_ref as rr
import weighted_ref as wr
from radio_mapper_amd import multi, xcorr
from radio_mapper_amd import tdoa_processor as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement against the helper it stacks ---------------------------------------------------------------------------------
def test_the_reference_stacks_the_single_band_reference_per_band():
    W, B, N, D = 3, 3, 64, 5
    iq, _, grid, lags, _ = br.scene(W, B, N, D, seed=11)
    bands = br.band_set(3, W)
    lb = br.bounds_holding(lags, N)
    ref = br.reference(iq, grid, bands, None, True, lb)
    assert ref["dop"].shape == (W, 3, 3) and ref["bin_peak"].shape == (W, 3, 3, D)
    for m in range(3):
        one = rr.reference(iq, grid, None, band=bands[:, m], phat=True, lag_bounds=lb)
        for k in br.OUT_KEYS + ("bin_peak",):
            assert np.array_equal(ref[k][:, m], one[k]), (k, m)
    shared = br.reference(iq, grid, br.band_set(2), cr.custom_pairs(B))
    assert shared["dop"].shape == (W, 2, 4)
    assert np.array_equal(shared["lag_int"][:, 1], rr.reference(iq, grid, cr.custom_pairs(B), band=np.array(br.EMITTER_BANDS[1]))["lag_int"])


# ---- 2. what the entry is for: two emitters in one capture, free-running receivers -----------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 2), (4096, 1)], ids=["N=256 W=2", "N=4096 W=1"])
def test_two_emitters_each_band_finds_its_own_emitter(shape):
    """caf_request_ref.two_emitter_scene: offsets (0, 1, 2) and (2, 0, 1) grid steps per buoy, D = 5.  Without a band the
    search returns the strong emitter's hypotheses [3, 4, 3] and lags for all three pairs; under each emitter's own band,
    with and without PHAT, it returns that emitter's: [3, 4, 3] and [0, 1, 3], hypothesis margins at least 0.20 and lag
    margins at least 5e-3."""
    N, W = shape
    iq, grid, la, ha, lw, hb = rr.two_emitter_scene(N, W=W)
    assert ha.tolist() == [3, 4, 3] and hb.tolist() == [0, 1, 3]
    plain = rr.reference(iq, grid)
    assert np.array_equal(plain["dop"], np.broadcast_to(ha, (W, 3))) and np.array_equal(plain["lag_int"], la)
    bands = np.array([wr.STRONG_BAND, wr.WEAK_BAND])
    for phat in (False, True):
        ref = br.reference(iq, grid, bands, None, phat)
        assert np.array_equal(ref["dop"][:, 0], np.broadcast_to(ha, (W, 3))) and np.array_equal(ref["lag_int"][:, 0], la)
        assert np.array_equal(ref["dop"][:, 1], np.broadcast_to(hb, (W, 3))) and np.array_equal(ref["lag_int"][:, 1], lw)
        print("phat %s: hypothesis margin %.3f, lag margin %.2e" % (phat, ref["hyp_margin"].min(), ref["lag_margin"].min()))
        assert ref["hyp_margin"].min() >= 0.20 and ref["lag_margin"].min() >= 5e-3


def test_transform_count_of_the_reference_fleet():
    """3 buoys, D = 21, M = 4: (1 + D) B + M D P = 318 transforms serve what M ((1 + D) B + D P) = 516 do now"""
    B, D, M = 3, 21, 4
    P = B * (B - 1) // 2
    assert (1 + D) * B + M * D * P == 318 and M * ((1 + D) * B + D * P) == 516


# ---- 3. the conditions on the inputs of the GPU cases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", br.REFERENCE_CASES + [c for c in br.ANCHOR_CASES if c not in br.REFERENCE_CASES])
def test_every_gpu_case_needs_no_excuse_and_its_winners_differ(name):
    """every slot's hypothesis margin and lag margin exceed 1e-5 on the reference alone, so dop_idx and lag_int are demanded
    exactly everywhere; and the winners differ between the bands of a window and between the slots of a call"""
    ref = br.case_reference(name)
    print("hypothesis margin %.3e, lag margin %.3e" % (ref["hyp_margin"].min(), ref["lag_margin"].min()))
    assert int((ref["hyp_margin"] <= br.LAG_MARGIN_BAR).sum() + (ref["lag_margin"] <= br.LAG_MARGIN_BAR).sum()) == 0
    dop, li = ref["dop"], ref["lag_int"]
    assert np.any(dop != dop[:, :1]) and np.any(li != li[:, :1])             # between the bands of a window
    assert len(set(dop.ravel().tolist())) > 1 and len(set(li.ravel().tolist())) > 1
    sc, pl, M, form, rid = name.split("/")
    if form == "perwin":
        _, _, _, _, bands, _ = br.case(name)
        for m in range(int(M)):
            assert len({tuple(r) for r in bands[:, m].tolist()}) == bands.shape[0]      # column m differs in every window


@pytest.mark.parametrize("shape", [(4096, 3), (256, 5), (8192, 5)], ids=lambda s: "N=%d W=%d" % s)
def test_own_window_case_needs_no_excuse(shape):
    N, W = shape
    iq, _, grid, bands, lb = br.differing_case(N, W, 3)
    ref = br.reference(iq, grid, bands, None, True, lb)
    assert ref["hyp_margin"].min() > br.LAG_MARGIN_BAR and ref["lag_margin"].min() > br.LAG_MARGIN_BAR
    for w in range(1, W):
        assert np.all((lb[w, :, 0] > lb[w - 1, :, 1]) | (lb[w, :, 1] < lb[w - 1, :, 0]))
    thin = br.one_bin_bands(N, W, 3)
    for w in range(W):
        for m in range(3):
            s0, s1 = wr.kept_bins(thin[w, m, 0], thin[w, m, 1], N)
            assert s0 == s1 and abs(s0) <= 0.4 * 2 * N, (w, m, s0, s1)           # one bin, inside the generator's band
    assert len({tuple(r) for r in thin.reshape(-1, 2).tolist()}) == W * 3


# ---- 4. the binding ----------------------------------------------------------------------------------------------------------------------
def test_export_and_header():
    assert "rmx_caf_batch_bands" in xcorr.EXPORTS
    header = open(os.path.join(ROOT, "include", "rmx.h")).read()
    assert "int rmx_caf_batch_bands(rmx_ctx* ctx" in header
    doc = header[header.index("The Doppler search under several bands per window"):header.index("int rmx_caf_batch_bands(")]
    for said in ("n_bands == 1 IS rmx_caf_batch_request", "[n_windows][n_bands][n_pairs]", "never NULL", "d-major first maximum",
                 "v = (d * n_windows + w) * n_bands + m", "g_rows_anchor", "n_bands outside 1 .. 64", "never split silently",
                 "There is no integration here", "n_windows == 0 or n_pairs == 0 returns RMX_OK"):
        assert said in doc, said
    integ = header[header.index("The Doppler search integrated noncoherently"):header.index("int rmx_caf_batch_integrated(")]
    assert "Several bands under the search: rmx_caf_batch_bands" in integ
    src = open(os.path.join(ROOT, "radio-mapper_amd", "csrc", "rmx_hip.hip")).read()
    body = src[src.index("int rmx_caf_batch_bands("):src.index("int rmx_solve_batch(")]
    assert "return caf_request(c, a, flags);" in body and "rmx_caf_batch_request(" not in body     # through no other entry


class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def _engine(n_buoys, n_samples):
    eng = object.__new__(xcorr.XcorrEngine)
    eng._lib, eng._ctx = _FakeLib(), None
    eng.n_buoys, eng.n_samples, eng.max_windows, eng.device = n_buoys, n_samples, 64, 0
    return eng


def test_caf_bands_goes_through_its_entry_with_the_arguments_in_order():
    eng = _engine(3, 16)
    W, M, P = 4, 2, 3
    iq = np.zeros((W, 3, 16), np.complex64)
    bands = np.tile([[-0.2, 0.1], [0.2, 0.3]], (W, 1, 1))
    lb = np.zeros((W, P, 2), np.int32)
    out = eng.caf_bands(iq, [0.0, 0.01, 0.02], bands, lag_bounds=lb, whiten=True, fine=True)
    name, a = eng._lib.calls[-1]
    assert name == "rmx_caf_batch_bands" and len(a) == 19
    # ctx, iq, n_windows, pairs, n_pairs, grid, n_dopplers, band_cps, n_bands, bands_per_window, weighting, lag_bounds,
    # bounds_per_window, dop_idx, dop_frac, lag_int, lag_frac, peak, flags
    assert a[2] == W and a[3] is None and a[4] == P and a[6] == 3 and a[8] == M and a[9] == 1 and a[10] == xcorr.RMX_WEIGHT_PHAT
    assert a[12] == 1 and a[14] is not None and a[18] == 0
    assert [o.shape for o in out] == [(W, M, P)] * 5
    assert [o.dtype for o in out] == [np.int32, np.float32, np.int32, np.float32, np.float32]
    out = eng.caf_bands(iq, [0.0], bands[0], pairs=[(2, 0), (0, 1)])
    name, a = eng._lib.calls[-1]
    assert name == "rmx_caf_batch_bands" and a[4] == 2 and a[3] is not None and a[9] == 0 and a[10] == 0 and a[11] is None and a[14] is None
    assert [o.shape for o in out] == [(W, M, 2)] * 4
    out = eng.caf_bands(iq, [0.0], bands[0, :1])                                # one band still goes through the banded entry
    assert eng._lib.calls[-1][0] == "rmx_caf_batch_bands" and eng._lib.calls[-1][1][8] == 1 and out[0].shape == (W, 1, P)
    raw = np.zeros((W, 3, 32), np.uint8)
    eng.caf_bands(raw, [0.0], bands)
    assert eng._lib.calls[-1][1][18] == xcorr.RMX_IN_U8
    n = len(eng._lib.calls)
    assert [o.shape for o in eng.caf_bands(iq[:0], [0.0], bands[:0])] == [(0, M, P)] * 4 and len(eng._lib.calls) == n   # empty: no call
    eng.caf_bands_device(1 << 20, W, [0.0, 0.1], bands, 2 << 20, 3 << 20, 4 << 20, 5 << 20, lag_bounds=lb[0], dop_frac_ptr=6 << 20, u8=True)
    name, a = eng._lib.calls[-1]
    assert name == "rmx_caf_batch_bands" and a[1].value == 1 << 20 and a[13].value == 2 << 20 and a[14].value == 6 << 20
    assert a[15].value == 3 << 20 and a[12] == 0 and a[18] == xcorr.RMX_IN_DEVICE | xcorr.RMX_OUT_DEVICE | xcorr.RMX_IN_U8
    eng.caf_bands_device(1 << 20, W, [0.0], bands, 2 << 20, 3 << 20, 4 << 20, 5 << 20)
    assert eng._lib.calls[-1][1][14] is None
    # the other families are as they were
    eng.caf(iq, [0.0], band=bands[:, 0])
    assert eng._lib.calls[-1][0] == "rmx_caf_batch_request"
    eng.correlate_bands(iq, bands)
    assert eng._lib.calls[-1][0] == "rmx_xcorr_batch_bands"


def test_lag_request_checks_and_refusals():
    W, B = 4, 3
    ok = np.array([[-0.2, 0.1], [0.2, 0.3]])
    req = xcorr.lag_request("caf_bands", B, W, None, None, ok, doppler_cps=[0.0, 0.1], fine=True)
    assert req.family == "caf_bands" and req.M == 2 and req.K == 1 and req.U == 0 and req.grid.shape == (2,) and not req.quality
    assert xcorr.entry_name(req) == "rmx_caf_batch_bands" and xcorr._ENTRY_ARGS["rmx_caf_batch_bands"] == "WBF"
    assert [(n, s) for n, _, s in req.outputs()] == [(n, (W, 2, 3)) for n in ("dop_idx", "dop_frac", "lag_int", "lag_frac", "peak")]
    assert [n for n, _, _ in req._replace(fine=False).outputs()] == ["dop_idx", "lag_int", "lag_frac", "peak"]
    for kw, word in ((dict(integrate=2), "no integration"), (dict(refine=4), "no refinement"), (dict(quality=True), "no quality")):
        with pytest.raises(ValueError, match=word):
            xcorr.lag_request("caf_bands", B, W, None, None, ok, doppler_cps=[0.0], **kw)
    # the order: grid, bands, lag_bounds
    with pytest.raises(ValueError, match="could not convert|float"):
        xcorr.lag_request("caf_bands", B, W, None, "bad bounds", None, doppler_cps=["x"])
    with pytest.raises(ValueError, match="bands"):
        xcorr.lag_request("caf_bands", B, W, None, np.zeros((5, 5)), None, doppler_cps=[0.0])
    with pytest.raises(ValueError, match="bands must hold 1..64"):
        xcorr.lag_request("caf_bands", B, W, None, np.zeros((5, 5)), np.zeros((65, 2)), doppler_cps=[0.0])
    with pytest.raises(ValueError, match="lag_bounds"):
        xcorr.lag_request("caf_bands", B, W, None, np.zeros((5, 5), np.int32), ok, doppler_cps=[0.0])
    per = xcorr.lag_request("caf_bands", B, W, None, np.zeros((W, 3, 2), np.int32), np.tile(ok, (W, 1, 1)), doppler_cps=[0.0])
    lb, bd = per.cut(1, 3)
    assert lb.shape == (2, 3, 2) and bd.shape == (2, 2, 2)


# ---- 5. MultiXcorrEngine.caf_bands on stub engines ----------------------------------------------------------------------------------------
class _StubBands:
    instances = []

    def __init__(self, n_buoys, n_samples, max_windows, device):
        self.n_buoys, self.max_windows, self.calls = n_buoys, max_windows, []
        _StubBands.instances.append(self)

    def caf_bands(self, iq, doppler_cps, bands, pairs=None, **kw):
        self.calls.append(dict(kw, windows=iq.shape[0], bands=np.asarray(bands), grid=doppler_cps))
        W, M = iq.shape[0], np.asarray(bands).shape[-2]
        P = self.n_buoys * (self.n_buoys - 1) // 2
        tag = np.asarray(iq)[:, 0, 0].real.astype(np.int32)[:, None, None] + 1000 * np.arange(M, dtype=np.int32)[None, :, None] \
            + np.zeros((1, 1, P), np.int32)
        lb = kw.get("lag_bounds")
        lo = tag if lb is None or np.asarray(lb).ndim == 2 else np.broadcast_to(np.asarray(lb)[:, None, :, 0], (W, M, P)).astype(np.int32)
        out = (tag, lo, tag.astype(np.float32), tag.astype(np.float32) + 0.5)
        if kw.get("fine"):
            out = (out[0], tag.astype(np.float32) / 100) + out[1:]
        return out

    def close(self):
        pass


def test_multi_engine_caf_bands_shards_windows():
    _StubBands.instances.clear()
    W, B, N, M = 11, 3, 16, 2
    iq = np.zeros((W, B, N), np.complex64)
    iq[:, 0, 0] = np.arange(W)
    lb = np.zeros((W, 3, 2), np.int32)
    lb[:, :, 0] = 100 + np.arange(W)[:, None]
    bands = np.tile([[-0.2, 0.1], [0.2, 0.3]], (W, 1, 1)) + 0.001 * np.arange(W)[:, None, None]
    grid = [0.0, 0.01]
    with multi.MultiXcorrEngine(B, N, W, devices=[0, 1, 2], engine_factory=_StubBands) as eng:
        out = eng.caf_bands(iq, grid, bands, lag_bounds=lb, whiten=True, fine=True)
        assert len(out) == 5 and all(a.shape == (W, M, 3) for a in out)
        assert np.array_equal(out[0][:, 0, 0], np.arange(W)) and np.array_equal(out[0][:, 1, 0], 1000 + np.arange(W))
        assert np.array_equal(out[2][:, 0, 0], 100 + np.arange(W))             # every window under its own bounds
        calls = [c for e in _StubBands.instances for c in e.calls]
        assert len(calls) == 3 and sum(c["windows"] for c in calls) == W
        assert all(c["fine"] is True and c["whiten"] is True and c["grid"] is grid for c in calls)
        assert all(c["bands"].shape == (c["windows"], M, 2) and c["lag_bounds"].shape == (c["windows"], 3, 2) for c in calls)
        w0 = 0
        for c in calls:
            assert np.array_equal(c["bands"], bands[w0:w0 + c["windows"]])       # its own windows' band sets
            w0 += c["windows"]
        out = eng.caf_bands(iq, grid, bands[0])                                  # shared: whole to every block
        assert len(out) == 4 and all(c["bands"].shape == (M, 2) for e in _StubBands.instances for c in e.calls[-1:])
        with pytest.raises(ValueError, match="bands"):
            eng.caf_bands(iq, grid, np.zeros((3, 2, 2)))
    _StubBands.instances.clear()


# ---- 6. the seam: share_doppler on a stub engine ------------------------------------------------------------------------------------------
class _StubEngine:
    """records caf / caf_bands; a slot's lag encodes its band's lower edge, its offset the band's upper edge"""
    max_windows = 64

    def __init__(self):
        self.calls = []

    @staticmethod
    def _of(band, shape):
        lo = np.broadcast_to(np.asarray(band)[..., 0, None], shape)
        hi = np.broadcast_to(np.asarray(band)[..., 1, None], shape)
        li = np.rint(lo * 1000).astype(np.int32)
        return (np.clip(np.rint(hi * 5).astype(np.int32) + 2, 0, 4), np.zeros(shape, np.float32), li, np.zeros(shape, np.float32), np.ones(shape, np.float32))

    def caf(self, iq, doppler_cps, pairs=None, lag_bounds=None, band=None, whiten=False, fine=False):
        self.calls.append(("caf", iq.shape[0], None if lag_bounds is None else np.asarray(lag_bounds).copy()))
        W = iq.shape[0]
        return self._of(np.asarray(band).reshape(W, 2), (W, 3))

    def caf_bands(self, iq, doppler_cps, bands, pairs=None, lag_bounds=None, whiten=False, fine=False):
        self.calls.append(("caf_bands", iq.shape[0], None if lag_bounds is None else np.asarray(lag_bounds).copy()))
        W, M = iq.shape[0], np.asarray(bands).shape[1]
        return self._of(np.asarray(bands), (W, M, 3))

    def close(self):
        pass


def _seam(bound_lags=False, captures=1, first=3, **flags):
    """`captures` captures; capture c is cut into first - c frequency groups"""
    fs, fc, N = 2.048e6, 121.0e6, 256
    p = tp.TDoAProcessor(band_limit=True, doppler_search_hz=(8000.0, 4000.0), **flags)
    p.tdoa_calculator.bound_lags = bound_lags
    stub = _StubEngine()
    p.tdoa_calculator._engine = lambda *a, **k: stub
    buoys = [("B0", 37.0, -122.0), ("B1", 37.3, -122.0), ("B2", 37.0, -121.6)]
    for bid, lat, lng in buoys:
        p.register_buoy(tp.BuoyPosition(bid, lat, lng, 0.0, timing_accuracy_ns=20))
    groups = []
    p.hyperbolic_positioner.triangulate_position = lambda meas, pos: groups.append(list(meas))
    rng = np.random.default_rng(5)
    dets = []
    for c in range(captures):
        cap = (rng.standard_normal((3, N)) + 1j * rng.standard_normal((3, N))).astype(np.complex64)
        for f in (fc + 0.10 * fs + c * 0.02 * fs, fc - 0.25 * fs + c * 0.02 * fs, fc + 0.30 * fs + c * 0.02 * fs)[:first - c]:
            dets += [tp.SignalDetection(bid, f / 1e6, -60.0, "t", 1_700_000_000_000_000_000, lat, lng, 0.9, iq_samples=cap[b],
                                        sample_rate_hz=fs, center_freq_hz=fc, bandwidth_hz=0.05 * fs) for b, (bid, lat, lng) in enumerate(buoys)]
    p.process_signal_detections(dets)
    meas = [[(m.buoy1_id, m.buoy2_id, m.frequency_mhz, m.time_difference_ns, m.confidence, m.frequency_offset_hz) for m in g] for g in groups]
    return [(n, w) for n, w, _ in stub.calls], meas, stub.calls


@pytest.mark.parametrize("bound_lags", [False, True])
def test_share_doppler_sends_shared_captures_through_one_caf_bands_call(bound_lags):
    """two captures, three and two frequency groups cut from them: with share_doppler ONE caf_bands call of two windows
    (the narrower row padded, the padded output dropped); the measurements, frequency_offset_hz included, are those of the
    separate searches, in the same order.  Off by default, and only together with share_captures."""
    calls_on, meas_on, raw_on = _seam(bound_lags, captures=2, share_captures=True, share_doppler=True)
    calls_off, meas_off, _ = _seam(bound_lags, captures=2, share_captures=True)
    assert calls_on == [("caf_bands", 2)] and calls_off == [("caf", 5)], (calls_on, calls_off)
    assert len(meas_on) == 5 and meas_on == meas_off
    assert all(m[5] is not None for g in meas_on for m in g) and len({m[5] for g in meas_on for m in g}) > 1
    assert (raw_on[0][2] is not None) == bound_lags
    for flags in ({}, {"share_doppler": True}, {"share_captures": True}):
        assert _seam(bound_lags, captures=2, **flags)[0] == calls_off
    assert tp.TDoACalculator().share_doppler is False
    # one capture cut into three groups: one window under three bands
    assert _seam(bound_lags, captures=1, share_captures=True, share_doppler=True)[0] == [("caf_bands", 1)]
    # a capture with a single group has nothing to share: the usual search, as with the flag off
    alone = _seam(bound_lags, captures=1, first=1, share_captures=True, share_doppler=True)
    assert alone[0] == [("caf", 1)] and alone[1] == _seam(bound_lags, captures=1, first=1)[1]
    # a shared capture beside a lone one: the shared one through caf_bands, the other the usual way
    mixed = _seam(bound_lags, captures=3, share_captures=True, share_doppler=True)
    assert sorted(mixed[0]) == [("caf", 1), ("caf_bands", 2)] and mixed[1] == _seam(bound_lags, captures=3)[1]


def test_measure_band_lags_with_a_grid():
    calc = tp.TDoACalculator()
    stub = _StubEngine()
    calc._engine = lambda *a, **k: stub
    iq = np.zeros((2, 3, 64), np.complex64)
    bands = np.tile([[-0.2, 0.1], [0.2, 0.3]], (2, 1, 1))
    grid = np.array([-0.02, -0.01, 0.0, 0.01, 0.02])
    li, lf, pk, dop, nu = calc.measure_band_lags(iq, bands, doppler_cps=grid)
    assert stub.calls[-1][:2] == ("caf_bands", 2) and li.shape == dop.shape == nu.shape == (2, 2, 3)
    assert np.array_equal(nu, xcorr.doppler_estimate(grid, dop, np.zeros(dop.shape)))
    out = calc.measure_band_lags(iq[None], bands[None], doppler_cps=grid)
    assert out[0].shape == (1, 2, 2, 3)
    for kw in (dict(integrate=2), dict(refine=4), dict(quality=True)):
        with pytest.raises(ValueError, match="no integration, refinement or quality"):
            calc.measure_band_lags(iq, bands, doppler_cps=grid, **kw)
