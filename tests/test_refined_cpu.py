"""rmx_xcorr_batch_refined without a GPU: the restatement of the fine lag search (tests/refined_ref.py) against the coarse
references it is built on, its bounds and tie rules, the accuracy the feature exists for (pinned on the restatement), and
the export and argument checks of the C entry and of the Python binding."""
import ctypes as C
import os

import numpy as np
import pytest

import radio_mapper_amd as rm
import refined_ref as rr
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


def _true(delays, pairs=None):
    B = delays.shape[1]
    pairs = [(i, j) for i in range(B) for j in range(i + 1, B)] if pairs is None else pairs
    return np.stack([delays[:, j] - delays[:, i] for i, j in pairs], axis=1)


# -- the restatement -------------------------------------------------------------------------------------------------
def test_the_centre_tap_is_the_coarse_peak():
    """f[0] = |r(lag0)| of the interpolant is the existing r[lag0 mod L]: the coarse reference's peak"""
    N = 256
    iq, _ = rm.synth.make_windows(4, 3, N, 10e6, seed=7, max_delay=min(40, N / 8))
    for U in (2, 8):
        *_, det = rr.refined_batch(iq, U, detail=True)
        f0 = det["taps"][:, :, U].astype(np.float64)
        assert np.all(np.abs(f0 - det["coarse_peak"]) <= 1e-6 * det["coarse_peak"])
    *_, det = rr.refined_batch(iq, 4, integrate=2, detail=True)
    assert np.all(np.abs(det["taps"][:, :, 4] - det["coarse_peak"]) <= 1e-6 * det["coarse_peak"])


def test_the_fine_grid_contains_the_integer_lags():
    """u = +-U are lag0 +- 1: the interpolant there is the coarse vector's neighbour taps"""
    N, U = 64, 4
    iq, _ = rm.synth.make_windows(3, 2, N, 10e6, seed=3, max_delay=6)
    *_, det = rr.refined_batch(iq, U, detail=True)
    for w in range(3):
        m = wr.weighted_full(iq[w, 0], iq[w, 1])
        k = int(det["lag0"][w, 0]) + N - 1
        assert np.allclose(det["taps"][w, 0, [0, U, 2 * U]], m[[k - 1, k, k + 1]], rtol=2e-6)


@pytest.mark.parametrize("edge", ["lo", "hi"])
def test_only_admitted_taps_at_a_bound(edge):
    N, U = 256, 8
    iq, _ = rm.synth.make_windows(6, 3, N, 10e6, seed=11, max_delay=30)
    li0, *_ = rr.refined_batch(iq, U)
    *_, det0 = rr.refined_batch(iq, U, detail=True)
    lag0 = det0["lag0"]
    lb = np.stack([lag0, lag0 + 3] if edge == "lo" else [lag0 - 3, lag0], axis=-1)   # [W][P][2]
    li, lf, pk, _, _, _, det = rr.refined_batch(iq, U, lag_bounds=lb, detail=True)
    assert np.array_equal(det["lag0"], lag0)                    # the same integer peak, now on the slice's edge
    lag = li + lf
    assert np.all(li >= lb[..., 0]) and np.all(li <= lb[..., 1])
    assert np.all(lag >= lb[..., 0]) and np.all(lag <= lb[..., 1])
    assert np.all(np.abs(lf) <= 0.5)
    # the free estimate leaves lag0 on either side; the bounded one only into the slice: it is the free one where that
    # has u* on the admitted side (more than half a fine step from lag0), and lag0 itself (u* = 0 without its outer
    # neighbour: no parabola) everywhere else
    off = (li0 + rr.refined_batch(iq, U)[1] - lag0) * (1 if edge == "lo" else -1)
    side, rest = off > 0.5 / U + 1e-6, off < 0.5 / U - 1e-6
    assert side.any() and rest.any()
    assert np.allclose((lag - lag0)[side] * (1 if edge == "lo" else -1), off[side], atol=1e-6)
    assert np.all(lag[rest] == lag0[rest]) and np.all(pk[rest] == det["taps"][..., U][rest])


@pytest.mark.parametrize("sign", [1, -1])
def test_the_ends_of_the_full_interval(sign):
    N, U = 32, 4
    x = np.zeros((1, 2, N), np.complex64)
    x[0, 0, 0 if sign > 0 else N - 1] = 20
    x[0, 1, N - 1 if sign > 0 else 0] = 20 * np.exp(0.3j)
    li, lf, pk, *_ = rr.refined_batch(x, U)
    assert li[0, 0] == sign * (N - 1) and abs(lf[0, 0]) <= 0.5 and pk[0, 0] > 0
    assert abs(li[0, 0] + lf[0, 0]) <= N - 1


def test_an_all_zero_window_gives_lag0_zero_zero():
    N = 64
    iq, _ = rm.synth.make_windows(2, 3, N, 10e6, seed=2, max_delay=6)
    iq[:, 1] = 0
    lb = np.array([[-5, 9], [-(N - 1), N - 1], [2, 2]])
    for kw in ({}, {"phat": True}, {"integrate": 2}):
        li, lf, pk, *_ = rr.refined_batch(iq, 8, lag_bounds=lb, **kw)
        assert np.all(np.isfinite(lf)) and np.all(np.isfinite(pk))
        for q in (0, 2):                                        # pairs (0,1), (1,2): argmax of zeros = the slice's start
            assert np.all(li[:, q] == lb[q, 0]) and np.all(lf[:, q] == 0) and np.all(pk[:, q] == 0)
        assert np.all(pk[:, 1] > 0)


def test_lag_frac_stays_in_half_a_sample_and_the_carry_happens():
    """a true offset of half a sample: delta crosses +-0.5 on some windows, the carry goes into lag_int"""
    N, U, W = 256, 8, 24
    d = np.zeros((W, 2))
    d[:, 1] = 10.5
    iq, _ = rm.synth.make_windows(W, 2, N, 10e6, seed=5, snr_db=25, delays=d)
    li, lf, _, _, _, _, det = rr.refined_batch(iq, U, detail=True)
    assert np.all(np.abs(lf) <= 0.5)
    carried = li != det["lag0"]
    assert carried.any(), "no window crossed half a sample: the case does not test the carry"
    assert np.all(np.abs(li - det["lag0"]) <= 1)
    assert np.all(np.abs(li + lf - 10.5) < 0.1)


def test_resolve_tie_rule():
    f = np.ones(9, np.float32)
    assert rr.resolve(f, 5, -9, 9, 4)[:3] == (5, 0.0, 1.0)                    # all equal: u* = 0
    f = np.array([0, 3, 0, 0, 1, 0, 0, 3, 0], np.float32)
    li, lf, pk, best, *_ = rr.resolve(f, 5, -9, 9, 4)
    assert best == -3 and pk == 3.0                                           # equal |u|: the negative one
    f = np.array([3, 0, 0, 3, 1, 0, 0, 0, 3], np.float32)
    assert rr.resolve(f, 5, -9, 9, 4)[3] == -1                                # the smallest |u|
    assert rr.resolve(f, 5, 5, 9, 4)[3] == 4 and rr.resolve(f, 5, 5, 9, 4)[:2] == (6, 0.0)   # lag0 == lo: u >= 0 only
    assert rr.resolve(f, 5, 5, 5, 4)[:4] == (5, 0.0, 1.0, 0)


# -- the reason for the feature ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    iq, delays = rm.synth.make_windows(16, 3, 1024, 10e6, seed=7, snr_db=10, bandwidth=0.8, max_delay=40)
    out = rr.refined_batch(iq, 8, detail=True)
    return iq, _true(delays), out


def test_the_parabola_is_biased_and_the_fine_search_is_not(scene):
    """measured with this restatement: parabola 0.0575 rms, refined U = 8 0.0080 rms, closure 0.008 against 0.104; the
    bounds leave 1.4 ... 4 x for a different FFT's rounding"""
    iq, true, (li, lf, _, _, _, _, det) = scene
    coarse = det["lag0"] + det["coarse_frac"]
    rms_par = float(np.sqrt(np.mean((coarse - true) ** 2)))
    rms_ref = float(np.sqrt(np.mean((li + lf - true) ** 2)))
    closure = np.abs((li + lf)[:, 0] + (li + lf)[:, 2] - (li + lf)[:, 1])     # (0,1) + (1,2) - (0,2)
    print("parabola rms %.4f, refined rms %.4f, closure max %.4f" % (rms_par, rms_ref, closure.max()))
    assert rms_par >= 0.04
    assert rms_ref <= 0.012
    assert np.all(closure <= 0.03)


def test_the_float32_variant_lands_on_the_float64_one(scene):
    iq, _, (li, lf, pk, *_) = scene
    si, sf, sp, *_ = rr.refined_batch(iq, 8, single=True)
    assert np.all(np.abs((si + sf) - (li + lf)) <= 1e-5)
    assert np.allclose(sp, pk, rtol=1e-5)


# -- C entry and binding -----------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_refined_entry(lib):
    hdr = open(os.path.join(ROOT, "include", "rmx.h")).read()
    assert "int rmx_xcorr_batch_refined(" in hdr and "int refine," in hdr
    assert "rmx_xcorr_batch_refined" in xcorr.EXPORTS
    assert hasattr(lib, "rmx_xcorr_batch_refined")
    import __graft_entry__ as g
    assert "refine.hpp" in g.SOURCES


@pytest.mark.parametrize("U", [0, 3, 8])
def test_null_ctx_is_rejected_whatever_u(lib, U):
    li, lf, pk = C.c_int32(), C.c_float(), C.c_float()
    rc = lib.rmx_xcorr_batch_refined(None, C.byref(li), 4, None, 0, 1, None, 0, 0, None, 0, U, C.byref(li), C.byref(lf),
                                     C.byref(pk), 0)
    assert rc == -1   # RMX_E_INVAL


class _NoCall(xcorr.XcorrEngine):
    def __init__(self):   # no library, no ctx: a C call would fail with AttributeError, not ValueError
        self.n_buoys, self.n_samples = 3, 16

    def _check_iq(self, iq):
        return iq, 0

    def __del__(self):
        pass


@pytest.mark.parametrize("bad", [1, 3, 32, -2, 2.5, True, "8", None])
def test_check_refine_rejects_before_any_call(bad):
    with pytest.raises(ValueError):
        xcorr.check_refine(bad)
    with pytest.raises(ValueError):
        _NoCall().correlate(np.zeros((4, 3, 16), np.complex64), refine=bad)
    with pytest.raises(ValueError):
        _NoCall().correlate_device(0, 4, 0, 0, 0, refine=bad)
    with pytest.raises(ValueError):
        tp.TDoACalculator(refine=bad)


def test_check_refine_accepts():
    assert [xcorr.check_refine(u) for u in (0, 2, 4, 8, 16)] == [0, 2, 4, 8, 16]
    assert xcorr.check_refine(np.int32(8)) == 8


def test_a_refined_call_reaches_the_library():
    """refine = 8 passes the checks and goes to the C entry: without a ctx that is an AttributeError, not a ValueError"""
    with pytest.raises(AttributeError):
        _NoCall().correlate(np.zeros((4, 3, 16), np.complex64), refine=8)


class _Stub:
    def __init__(self, b, n, w, device=0):
        self.max_windows = w
        self.calls = []

    def correlate(self, iq, pairs=None, lag_bounds=None, band=None, whiten=False, integrate=1, refine=0):
        G = iq.shape[0] // integrate
        self.calls.append({"W": iq.shape[0], "K": integrate, "U": refine})
        return np.zeros((G, 3), np.int32), np.zeros((G, 3), np.float32), np.full((G, 3), float(refine), np.float32)

    def close(self):
        pass


@pytest.mark.parametrize("K", [1, 2])
def test_multi_engine_hands_refine_to_every_block(K):
    W = 8
    m = multi.MultiXcorrEngine(3, 16, W, devices=[0, 1], engine_factory=_Stub)
    _, _, pk = m.correlate(np.zeros((W, 3, 16), np.complex64), integrate=K, refine=4)
    calls = [c for e in m._engines for c in e.calls]
    assert len(calls) == 2 and all(c["U"] == 4 and c["K"] == K for c in calls)
    assert pk.shape == (W // K, 3) and np.all(pk == 4.0)
    with pytest.raises(ValueError):
        m.correlate(np.zeros((W, 3, 16), np.complex64), refine=3)
    m.close()


def test_calculator_passes_refine_only_when_set(monkeypatch):
    seen = []

    class Eng:
        max_windows = 8

        def correlate(self, iq, pairs=None, **kw):
            seen.append(kw)
            z = np.zeros((iq.shape[0], 3))
            return z.astype(np.int32), z.astype(np.float32), z.astype(np.float32)
    calc = tp.TDoACalculator(refine=8)
    monkeypatch.setattr(calc, "_engine", lambda b, n, w=1: Eng())
    assert calc._measure_groups(np.zeros((2, 3, 64), np.complex64)) is not None
    calc.measure_lags(np.zeros((2, 3, 64), np.complex64))
    calc.measure_lags(np.zeros((2, 3, 64), np.complex64), refine=2)
    assert seen[0].get("refine") == 8 and "refine" not in seen[1] and seen[2].get("refine") == 2
    assert tp.TDoAProcessor(refine=16).tdoa_calculator.refine == 16 and tp.TDoAProcessor().tdoa_calculator.refine == 0
