"""rmx_caf_batch_request without a GPU: the conditions on the inputs of every case tests/test_gpu_caf_request.py holds
to the parity rule, what the request is for (a common DC offset, two emitters, an echo) on the float32 restatement
(tests/caf_request_ref.py), the sub-grid Doppler estimate measured on the reference, the rules of dop_frac, and the
binding's own checks -- doppler_estimate, the shapes caf() refuses before it calls the library, the shards of
MultiXcorrEngine.caf, TDoACalculator's routing -- with stub engines."""
import numpy as np
import pytest

import caf_ref as cr
import caf_request_ref as rr
import radio_mapper_amd as rm
from radio_mapper_amd import multi, xcorr
from radio_mapper_amd.tdoa_processor import TDoACalculator, TDoAMeasurement, TDoAProcessor


# ---- 1. the conditions on the inputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_every_gpu_case_is_far_from_a_tie_on_the_reference(name):
    """dop_idx exact and lag_int exact, with no lag excused, are fair demands only where the reference's best hypothesis
    stands more than caf_ref.MARGIN_BAR above its second best and the winner's two largest magnitudes more than 1e-5
    apart: both hold for every pair-window of every case, on the reference alone."""
    ref = rr.case_reference(name)
    print("hypothesis margin %.3e, lag margin %.3e" % (ref["hyp_margin"].min(), ref["lag_margin"].min()))
    assert ref["hyp_margin"].min() > cr.MARGIN_BAR
    assert ref["lag_margin"].min() > rr.LAG_MARGIN_BAR


# ---- 2. what the request is for ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [256, 4096])
def test_dc_offset_plain_finds_zero_and_phat_finds_the_emitter(N):
    _, grid, lags, hyp = rr.dc_scene(N)
    plain, phat = rr.case_reference("dc%d/plain" % N), rr.case_reference("dc%d/phat" % N)
    assert np.all(plain["dop"] == len(grid) // 2)                 # nu = 0 for every pair: the DC offset's hypothesis
    assert np.all(np.abs(plain["lag_int"]) <= 4) and not np.any(plain["lag_int"][0] == lags)
    assert np.array_equal(phat["dop"][0], hyp) and np.array_equal(phat["lag_int"][0], lags)


def test_dc_offset_a_band_without_dc_repairs_it_too():
    iq, grid, lags, hyp = rr.dc_scene(1024)
    ref = rr.reference(iq, grid, band=(0.02, 0.5))
    assert np.array_equal(ref["dop"][0], hyp) and np.array_equal(ref["lag_int"][0], lags)


@pytest.mark.parametrize("N", [256, 4096])
def test_two_emitters_each_band_returns_its_own_lags_and_hypotheses(N):
    import weighted_ref as wr
    iq, grid, la, ha, lw, hw = rr.two_emitter_scene(N, W=2)
    assert not np.array_equal(ha, hw) and not np.array_equal(la, lw)
    strong, weak = rr.reference(iq, grid, band=wr.STRONG_BAND), rr.reference(iq, grid, band=wr.WEAK_BAND)
    assert np.array_equal(strong["lag_int"], la) and np.all(strong["dop"] == ha)
    assert np.array_equal(weak["lag_int"], lw) and np.all(weak["dop"] == hw)
    assert np.array_equal(rr.reference(iq, grid)["lag_int"], la)      # without a band the strong one hides the other


@pytest.mark.parametrize("N", [256, 4096])
def test_echo_bounds_return_the_direct_path(N):
    iq, grid, lags, hyp, lb = rr.echo_scene(N, W=2)
    free, bounded = rr.reference(iq, grid), rr.reference(iq, grid, lag_bounds=lb)
    assert np.array_equal(bounded["lag_int"], lags) and np.all(bounded["dop"] == hyp)
    assert np.all(free["lag_int"][:, :2] == lags[:, :2] + N // 4)     # pairs (0, 1), (0, 2): the echo wins without bounds
    assert np.all(free["peak"][:, :2] > bounded["peak"][:, :2])


# ---- 3. the sub-grid Doppler estimate on the reference ---------------------------------------------------------------------
@pytest.mark.parametrize("N", [256, 1024])
def test_subgrid_doppler_estimate_on_the_reference(N):
    """200 seeded trials, step 0.5 / N, 20 dB, offsets uniform within +-2.5 steps, D = 9: the rms error of
    doppler_estimate is below a quarter of the rms error of the index alone (0.29 steps: uniform within half a step)."""
    rng = np.random.default_rng(20 + N)
    t = np.array([rr.subgrid_trial(N, rng) for _ in range(200)])
    idx_rms = float(np.sqrt(np.mean((t[:, 1] - t[:, 0]) ** 2)))
    fine_rms = float(np.sqrt(np.mean((t[:, 2] - t[:, 0]) ** 2)))
    print("N = %d: index only %.4f steps rms, with dop_frac %.4f steps rms" % (N, idx_rms, fine_rms))
    assert 0.25 < idx_rms < 0.33
    assert fine_rms < 0.25 * idx_rms


# ---- 4. the rules of dop_frac -----------------------------------------------------------------------------------------------
def test_dop_frac_range_edges_and_zero_windows():
    rng = np.random.default_rng(5)
    peaks = rng.uniform(0.0, 1.0, size=(40, 6, 7)).astype(np.float32)
    peaks[3, 2] = peaks[3, 2, 0]                       # all equal: hypothesis 0
    peaks[4, 1, 3] = peaks[4, 1, 4] = 2.0              # a tie with the right neighbour: the lowest wins, dop_frac = +0.5
    dop = cr.first_max(peaks)
    frac = rr.dop_parabola(peaks, dop)
    assert frac.dtype == np.float32
    assert np.all(frac > -0.5) and np.all(frac <= 0.5)
    assert frac[4, 1] == np.float32(0.5) and dop[4, 1] == 3
    assert np.all(frac[(dop == 0) | (dop == 6)] == 0) and dop[3, 2] == 0
    assert np.any(frac != 0)
    # all-zero windows: every hypothesis' peak is 0, hypothesis 0 wins, dop_frac = 0 (through the restatement itself)
    ref = rr.reference(np.zeros((2, 3, 16), np.complex64), (np.arange(5) - 2) / 32.0, phat=True)
    assert not ref["dop"].any() and not ref["dop_frac"].any() and not ref["peak"].any()
    # a single hypothesis has no neighbours
    assert not rr.dop_parabola(peaks[..., :1], np.zeros((40, 6), np.int32)).any()


# ---- 5. the binding ------------------------------------------------------------------------------------------------------------
def test_doppler_estimate_values_and_refusals():
    grid = (np.arange(5) - 2) * 0.25e-3
    dop = np.array([[0, 2], [4, 3]], np.int32)
    frac = np.array([[0.0, 0.25], [0.0, -0.5]], np.float32)
    est = xcorr.doppler_estimate(grid, dop, frac)
    assert est.dtype == np.float64 and est.shape == (2, 2)
    assert np.allclose(est, grid[dop] + frac.astype(np.float64) * 0.25e-3, rtol=0, atol=1e-18)
    assert np.array_equal(xcorr.doppler_estimate([0.001], np.zeros(3, np.int32), np.zeros(3, np.float32)), np.full(3, 0.001))
    with pytest.raises(ValueError, match="uniformly"):
        xcorr.doppler_estimate([0.0, 0.001, 0.003], dop[:1, :1], frac[:1, :1])
    with pytest.raises(ValueError, match="uniformly"):
        xcorr.doppler_estimate([0.001, 0.001, 0.001], dop[:1, :1], frac[:1, :1])
    with pytest.raises(ValueError, match="fewer than 2"):
        xcorr.doppler_estimate([0.001], np.zeros(1, np.int32), np.array([0.1], np.float32))
    with pytest.raises(ValueError, match="shape"):
        xcorr.doppler_estimate(grid, dop, frac[:1])
    with pytest.raises(ValueError, match="dop_idx"):
        xcorr.doppler_estimate(grid, dop + 3, frac)
    with pytest.raises(ValueError, match="integer"):
        xcorr.doppler_estimate(grid, dop.astype(np.float32), frac)


def test_the_new_symbol_is_exported_and_declared():
    import os
    assert "rmx_caf_batch_request" in xcorr.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.abspath(rm.__file__)), "..", "include", "rmx.h")).read()
    assert "int rmx_caf_batch_request(rmx_ctx* ctx" in header and "dop_frac" in header


class _NoLibrary:
    """stands where the loaded library would: any call into it fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the binding called %s before it checked its arguments" % name)


def _bare_engine(B, N):
    eng = xcorr.XcorrEngine.__new__(xcorr.XcorrEngine)
    eng._lib, eng._ctx, eng.n_buoys, eng.n_samples = _NoLibrary(), None, B, N
    return eng


def test_caf_checks_its_shapes_before_it_calls_the_library():
    B, N, W = 3, 16, 4
    eng = _bare_engine(B, N)
    iq = np.zeros((W, B, N), np.complex64)
    grid = [0.0, 0.01]
    for kw, word in ((dict(lag_bounds=np.zeros((2, 2), np.int32)), "lag_bounds"), (dict(lag_bounds=np.zeros((W, 3, 2))), "integer"),
                     (dict(lag_bounds=np.zeros((W + 1, 3, 2), np.int32)), "lag_bounds"), (dict(band=[0.1, 0.2, 0.3]), "band"),
                     (dict(band=np.zeros((W + 1, 2))), "band"), (dict(band=[0.2, 0.1]), "lo <= hi"), (dict(band=[-0.6, 0.1]), "band")):
        with pytest.raises(ValueError, match=word):
            eng.caf(iq, grid, **kw)
        with pytest.raises(ValueError, match=word):
            eng.caf_device(0, W, grid, 0, 0, 0, 0, **kw)
    with pytest.raises(ValueError, match="iq"):
        eng.caf(iq[:, :2], grid, whiten=True)
    # a custom pair list sets P of the bounds' shape
    with pytest.raises(ValueError, match="lag_bounds"):
        eng.caf(iq, grid, pairs=[(0, 1), (1, 2)], lag_bounds=np.zeros((3, 2), np.int32))
    # an empty batch returns without a call, five arrays with fine=True
    out = eng.caf(iq[:0], grid, whiten=True, fine=True)
    assert [a.shape for a in out] == [(0, 3)] * 5 and out[1].dtype == np.float32
    assert len(eng.caf(iq[:0], grid, band=[-0.1, 0.1])) == 4


class _StubCaf:
    """records what each shard's engine is handed; answers with the window tags so the gather is visible"""
    instances = []

    def __init__(self, n_buoys, n_samples, max_windows, device):
        self.n_buoys, self.max_windows, self.calls = n_buoys, max_windows, []
        _StubCaf.instances.append(self)

    def caf(self, iq, doppler_cps, pairs=None, **kw):
        self.calls.append(kw)
        W, P = iq.shape[0], self.n_buoys * (self.n_buoys - 1) // 2
        tag = np.asarray(iq)[:, 0, 0].real.astype(np.int32)[:, None] + np.zeros((1, P), np.int32)
        out = (tag, tag + 1, tag.astype(np.float32), tag.astype(np.float32) + 0.5)
        return (out[0], tag.astype(np.float32) / 100,) + out[1:] if kw.get("fine") else out

    def close(self):
        pass


def test_multi_engine_caf_slices_bounds_and_bands_per_shard():
    _StubCaf.instances.clear()
    W, B, N = 7, 3, 16
    iq = np.zeros((W, B, N), np.complex64)
    iq[:, 0, 0] = np.arange(W)
    lb = np.arange(W * 3 * 2, dtype=np.int32).reshape(W, 3, 2) % 7
    bd = np.stack([np.full(W, -0.25), 0.01 * np.arange(W)], axis=1)
    with multi.MultiXcorrEngine(B, N, W, devices=[0, 1, 2], engine_factory=_StubCaf) as eng:
        blocks = eng.blocks(W)
        dop, dfrac, li, lf, pk = eng.caf(iq, [0.0, 0.01], lag_bounds=lb, band=bd, whiten=True, fine=True)
        assert np.array_equal(dop[:, 0], np.arange(W)) and np.array_equal(li[:, 2], np.arange(W) + 1)
        assert dfrac.dtype == np.float32 and np.allclose(dfrac[:, 1], np.arange(W) / 100.0)
        for e, (s, c) in zip(_StubCaf.instances, blocks):
            kw = e.calls[-1]
            assert np.array_equal(kw["lag_bounds"], lb[s:s + c]) and np.array_equal(kw["band"], bd[s:s + c])
            assert kw["whiten"] is True and kw["fine"] is True
        out = eng.caf(iq, [0.0, 0.01], lag_bounds=lb[0], band=bd[0])         # the shared forms go to every shard whole
        assert len(out) == 4
        for e in _StubCaf.instances:
            assert np.array_equal(e.calls[-1]["lag_bounds"], lb[0]) and np.array_equal(e.calls[-1]["band"], bd[0])
        assert len(eng.caf(iq, [0.0, 0.01])) == 4 and all(e.calls[-1] == {} for e in _StubCaf.instances)   # the plain call as before
        with pytest.raises(ValueError, match="lag_bounds"):
            eng.caf(iq, [0.0], lag_bounds=lb[:3])


# ---- 6. TDoACalculator ---------------------------------------------------------------------------------------------------------
def test_doppler_search_hz_construction_and_defaults():
    m = TDoAMeasurement("a", "b", 1, 2.0, 0.5, 100.0)
    assert m.frequency_offset_hz is None
    calc = TDoACalculator()
    assert calc.doppler_search_hz is None
    calc = TDoACalculator(doppler_search_hz=(500, 100), bound_lags=True, band_limit=True, whiten=True)
    grid = calc.doppler_grid(2.4e6)
    assert len(grid) == 11 and grid[5] == 0.0 and np.allclose(grid * 2.4e6, np.arange(-500, 501, 100))
    assert TDoAProcessor(doppler_search_hz=(300, 150)).tdoa_calculator.doppler_search_hz == (300.0, 150.0)
    for other in (dict(integrate=2), dict(refine=4), dict(min_psr=10.0), dict(correlation_confidence=True)):
        with pytest.raises(ValueError, match="doppler_search_hz and %s" % list(other)[0]):
            TDoACalculator(doppler_search_hz=(500, 100), **other)
    for bad in ((100, 0), (50, 100), (1e9, 1.0), (100,), "fast"):
        with pytest.raises(ValueError, match="doppler_search_hz"):
            TDoACalculator(doppler_search_hz=bad)


def test_measure_lags_routes_a_doppler_grid_to_caf(monkeypatch):
    seen = {}

    class FakeEngine:
        max_windows = 8

        def caf(self, iq, doppler_cps, pairs=None, **kw):
            seen.update(kw, grid=np.asarray(doppler_cps), shape=iq.shape)
            W, P = iq.shape[0], 3
            dop = np.full((W, P), 3, np.int32)
            return dop, np.full((W, P), 0.25, np.float32), np.full((W, P), 7, np.int32), np.zeros((W, P), np.float32), np.ones((W, P), np.float32)

        def correlate(self, *a, **k):
            raise AssertionError("a Doppler grid must go to caf()")

        def close(self):
            pass

    calc = TDoACalculator()
    monkeypatch.setattr(calc, "_engine", lambda b, n, w=1: FakeEngine())
    grid = (np.arange(5) - 2) * 1e-4
    lb = np.zeros((2, 3, 2), np.int32)
    li, lf, pk, dop, nu = calc.measure_lags(np.zeros((2, 3, 64), np.complex64), lag_bounds=lb, band=[-0.1, 0.2], whiten=True,
                                            doppler_cps=grid)
    assert seen["fine"] is True and seen["whiten"] is True and np.array_equal(seen["lag_bounds"], lb) and list(seen["band"]) == [-0.1, 0.2]
    assert np.all(li == 7) and np.all(dop == 3) and nu.dtype == np.float64 and np.allclose(nu, 1e-4 + 0.25e-4)
    for kw in (dict(integrate=2), dict(refine=2), dict(quality=True)):
        with pytest.raises(ValueError, match="doppler_cps and %s" % list(kw)[0]):
            calc.measure_lags(np.zeros((2, 3, 64), np.complex64), doppler_cps=grid, **kw)
    # _measure_groups: lags and offsets in hertz
    calc = TDoACalculator(doppler_search_hz=(200, 100), whiten=True)
    monkeypatch.setattr(calc, "_engine", lambda b, n, w=1: FakeEngine())
    lag, hz = calc._measure_groups(np.zeros((2, 3, 64), np.complex64), fs=2.0e6)
    assert np.all(lag == 7.0) and np.allclose(hz, 100.0 + 25.0) and len(seen["grid"]) == 5   # hypothesis 3 of -200 .. 200, + 0.25 steps
