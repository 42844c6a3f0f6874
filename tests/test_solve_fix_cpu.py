"""rmx_solve_batch_fix without a GPU: the kernel-order restatement of k_solve_plane and k_solve_fix
(tests/solve_fix_ref.py) against an independent numpy.linalg statement, the statistics that give the outputs their meaning
(a covariance that predicts the scatter, a cost that is a chi-square) by Monte Carlo through the restatement, the finding
that motivates the plane mode, the singular rule, the helpers (lag_weight, error_ellipse, tangent_plane), the binding's
checks before any C call, and the ABI.  tests/test_gpu_solve_fix.py holds the kernels to the restatement bit for bit.

The Monte-Carlo margins are five standard errors from chi-square statistics alone, for T windows and n unknowns:
variance ratios 5 sqrt(2 / (T - 1)), mean normalised error^2 within 5 sqrt(2 n / T) of n, mean cost within
5 sqrt(2 (P - n) / T) of P - n."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import solve_fix_ref as fr
import solve_kernel_ref as kr
from radio_mapper_amd import tdoa_processor as tp
from radio_mapper_amd import xcorr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 2000
MPS = kr.metres_per_sample(fr.FS_SCENE)
VAR_MARGIN = 5.0 * math.sqrt(2.0 / (T - 1))

_MC = {}


def _mc(name, plane_mode):
    """one Monte-Carlo run per (scene, mode), shared read-only by the tests below"""
    if (name, plane_mode) not in _MC:
        _MC[name, plane_mode] = fr.monte_carlo(name, plane_mode, T=T, seed=1)
    return _MC[name, plane_mode]


def _horizontal(m):
    """the east/north errors and the east/north block of cov of a three-unknown run, over the windows whose cov is finite"""
    E = m["plane"].reshape(3, 3)[1:]
    ok = np.isfinite(m["cov"][:, 0, 0])
    return m["err"][ok] @ E.T, E @ m["cov"][ok] @ E.T, ok


# -- 1. the two restatements agree ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,plane_mode,weighted", [("sea5", True, True), ("sea4", True, False), ("sea3", True, True),
                                                      ("heights6", False, True), ("heights6", False, False),
                                                      ("sea5", False, True)])
def test_kernel_order_agrees_with_linalg(name, plane_mode, weighted):
    """info to 1e-12 relative; cov to 1e-9 cond(info) relative: both sides form the same sums, the inversion amplifies a
    perturbation by the condition number, and 1e-9 leaves three decades over float64 rounding"""
    buoys, emitter, plane = fr.scene(name)
    pairs, li, lf, wgt = fr.noisy_lags(buoys, emitter, 200, seed=2)
    wgt = wgt if weighted else None
    pl = plane if plane_mode else None
    pos, cost, it, info, cov, resid = fr.solve_fix_kernel_order(buoys, pairs, li, lf, wgt, MPS, pl)
    linfo, lcov, lresid, cond = fr.fix_linalg(buoys, pairs, li, lf, wgt, MPS, pos, pl)
    assert np.all(np.isfinite(cov)), "the case is meant to be regular"
    big = lambda a: np.abs(a).max(axis=(1, 2))   # noqa: E731
    d_info = big(fr.sym(info) - linfo) / big(linfo)
    d_cov = big(fr.sym(cov) - lcov) / big(lcov)
    print("%s: info %.2e relative, cov %.2e relative at cond %.2e, resid %.2e m" % (
        name, d_info.max(), d_cov.max(), cond.max(), np.abs(resid - lresid).max()))
    assert np.all(d_info <= 1e-12)
    assert np.all(d_cov <= 1e-9 * cond)
    assert np.abs(resid - lresid).max() <= 1e-6      # metres: differences of ranges of 1e4 m formed from 6e6 m coordinates
    d = (li.astype(np.float64) + lf.astype(np.float64)) * MPS
    w64 = np.ones(d.shape) if wgt is None else wgt.astype(np.float64)
    assert np.allclose((w64 * resid * resid).sum(axis=1), cost, rtol=1e-12)      # cost is f at the returned pos


# -- 2. Monte Carlo: the covariance predicts the scatter, the cost is a chi-square ---------------------------------------------------
@pytest.mark.parametrize("name,plane_mode", [("sea3", True), ("sea4", True), ("sea5", True), ("heights6", False)])
def test_covariance_and_chi_square_by_monte_carlo(name, plane_mode):
    m = _mc(name, plane_mode)
    n, P = m["n"], m["P"]
    assert n == (2 if plane_mode else 3)
    print("%s: iters %.2f, bias %s m, variance ratios %s, normalised error^2 %.3f (%d), cost %.3f (%d)" % (
        name, m["iters"], np.round(m["bias"], 3), np.round(m["var_ratio"], 3), m["nees"], n, m["cost"], P - n))
    assert np.all(np.isfinite(m["cov"])) and m["maxed"] == 0.0
    assert np.all(np.abs(m["var_ratio"] - 1.0) <= VAR_MARGIN)
    assert abs(m["nees"] - n) <= 5.0 * math.sqrt(2.0 * n / T)
    assert abs(m["cost"] - (P - n)) <= 5.0 * math.sqrt(2.0 * (P - n) / T)
    if plane_mode:
        assert np.all(np.abs(m["bias"]) < 0.2)


def test_ninety_five_percent_ellipse_holds_its_share():
    """inside the ellipse of error_ellipse(cov, 0.95) <=> e^T info e <= -2 ln 0.05; five binomial standard errors"""
    for name in ("sea3", "sea4", "sea5"):
        m = _mc(name, True)
        inside = np.einsum("wi,wij,wj->w", m["err"], m["info"], m["err"]) <= -2.0 * math.log(0.05)
        print(name, "inside the 95 %% ellipse: %.4f" % inside.mean())
        assert abs(inside.mean() - 0.95) <= 5.0 * math.sqrt(0.95 * 0.05 / T)


# -- 3. the finding that motivates the feature ----------------------------------------------------------------------------------------
def test_plane_mode_walks_less_on_a_sea_level_fleet():
    plane, full = _mc("sea5", True), _mc("sea5", False)
    e, c, ok = _horizontal(full)
    up = np.cross(full["plane"][3:6], full["plane"][6:9])
    alt = full["err"] @ up
    print("five sea-level stations: iters %.1f in the plane, %.1f with three unknowns (%.2f %% on max_iter); altitude off by "
          "%.0f m on average, sd %.0f m" % (plane["iters"], full["iters"], 100 * full["maxed"], alt.mean(), alt.std()))
    assert plane["iters"] < full["iters"]
    assert plane["iters"] < 10 and full["iters"] > 15          # here 7.4 against 20.4


def test_three_unknowns_on_four_sea_level_stations_mispredict_the_scatter():
    full = _mc("sea4", False)
    e, c, ok = _horizontal(full)
    ratio = e.var(axis=0, ddof=1) / np.diagonal(c, axis1=1, axis2=2).mean(axis=0)
    print("four sea-level stations, three unknowns: %d of %d windows singular; of the others, east bias %.1f m, horizontal "
          "variance ratios %s" % ((~ok).sum(), T, e[:, 0].mean(), np.round(ratio, 2)))
    assert np.abs(ratio - 1.0).max() > VAR_MARGIN               # here 0.53 in the east
    # about half of the walks end on the fold of the two mirror solutions, where J^T W J is singular (here 978 of 2000):
    # some do and some do not, and every one of them says so
    assert 0.25 < (~ok).mean() < 0.75
    assert np.all(np.isposinf(full["cov"][~ok][:, [0, 1, 2], [0, 1, 2]]))
    plane = _mc("sea4", True)
    assert np.all(np.abs(plane["var_ratio"] - 1.0) <= VAR_MARGIN)


# -- 4. the singular rule ---------------------------------------------------------------------------------------------------------------
def _singular(cov):
    n = {3: 2, 6: 3}[cov.shape[1]]
    m = fr.sym(cov)
    eye = np.eye(n, dtype=bool)
    return np.all(np.isposinf(m[:, eye]), axis=1) & np.all(m[:, ~eye] == 0.0, axis=1)


def _last_pivot_ratio(info6):
    a = fr.sym(info6[None])[0]
    l00 = math.sqrt(a[0, 0])
    l10, l20 = a[0, 1] / l00, a[0, 2] / l00
    l11 = math.sqrt(a[1, 1] - l10 * l10)
    l21 = (a[1, 2] - l20 * l10) / l11
    return (a[2, 2] - l20 * l20 - l21 * l21) / a[2, 2]


def test_three_sea_level_stations_are_singular_for_three_unknowns_and_five_are_not():
    m3, m5 = _mc("sea3", False), _mc("sea5", False)
    assert np.all(_singular(m3["cov"].reshape(T, 9)[:, [0, 1, 2, 4, 5, 8]]))
    assert np.all(np.isfinite(m5["cov"]))
    for name, lo, hi in (("sea3", -1e-14, 1e-14), ("sea5", 1e-8, 1e-5)):
        buoys, emitter, plane = fr.scene(name)
        pairs, li, lf, wgt = fr.noisy_lags(buoys, emitter, 1, seed=3)
        info, cov, _ = fr.fix_kernel_order(buoys, pairs, li, lf, wgt, MPS, emitter[None, :])
        ratio = _last_pivot_ratio(info[0])
        print(name, "last pivot / its diagonal entry at the emitter: %.1e" % ratio)
        assert lo < ratio < hi and _singular(cov)[0] == (name == "sea3")
    # and the plane mode on the same three stations is regular
    assert np.all(np.isfinite(_mc("sea3", True)["cov"]))


@pytest.mark.parametrize("plane_mode", [False, True])
def test_all_zero_weights_are_singular(plane_mode):
    buoys, emitter, plane = fr.scene("sea5")
    pairs, li, lf, wgt = fr.noisy_lags(buoys, emitter, 5, seed=4)
    out = fr.solve_fix_kernel_order(buoys, pairs, li, lf, np.zeros_like(wgt), MPS, plane if plane_mode else None)
    pos, cost, it, info, cov, resid = out
    assert np.all(it == 25) and np.all(cost == 0.0) and np.all(info == 0.0) and np.all(_singular(cov))
    assert all(not np.any(np.isnan(a)) for a in out) and np.all(np.isfinite(resid))


def collinear_in_plane():
    """four stations on the plane's e1 axis, exactly: every unit vector from a point of the axis is +-e1, so j . e2 = 0"""
    o = kr.DEGENERATE_C
    plane = fr.as_plane(o, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    buoys = np.array([o + np.array([1000.0 * k, 0.0, 0.0]) for k in (-3, -1, 1, 4)])
    pairs = kr.all_pairs(4)
    li, lf = kr.seeded_lags(6, len(pairs), seed=5, span=3)
    return buoys, pairs, li, lf, plane


def test_collinear_stations_are_singular_in_plane_mode():
    buoys, pairs, li, lf, plane = collinear_in_plane()
    out = fr.solve_fix_kernel_order(buoys, pairs, li, lf, None, MPS, plane)
    pos, cost, it, info, cov, resid = out
    assert np.all(info[:, 0] > 0.0) and np.all(info[:, 1:] == 0.0) and np.all(_singular(cov))
    assert np.all(it == 25) and all(np.all(np.isfinite(a)) for a in (pos, cost, info, resid))


def centroid_on_a_buoy(plane_mode):
    buoys = kr.line_of_buoys((1, 0, -1))
    pairs = kr.all_pairs(3)
    li, lf = kr.seeded_lags(4, 3, seed=5)
    plane = fr.as_plane(kr.DEGENERATE_C, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)) if plane_mode else None
    return buoys, pairs, li, lf, plane


@pytest.mark.parametrize("plane_mode", [False, True])
def test_a_centroid_on_a_buoy_gives_zero_information_and_no_nan(plane_mode):
    buoys, pairs, li, lf, plane = centroid_on_a_buoy(plane_mode)
    out = fr.solve_fix_kernel_order(buoys, pairs, li, lf, None, kr.metres_per_sample(10e6), plane)
    pos, cost, it, info, cov, resid = out
    assert np.all(pos == buoys[1]) and np.all(it == 25)
    assert np.all(info == 0.0) and np.all(_singular(cov))
    assert all(not np.any(np.isnan(a)) for a in out) and np.all(np.isfinite(resid)) and np.all(np.isfinite(cost))


# -- 5. the helpers ---------------------------------------------------------------------------------------------------------------------
def test_lag_weight():
    fs, floor = 2.048e6, 0.05
    sig = np.array([[0.0, 0.02, 0.2, np.inf], [1.0, 3.5, 1e-9, 7.0]])
    w = xcorr.lag_weight(sig, fs, floor)
    mps = 299792458.0 / fs
    want = (1.0 / ((sig * sig + floor * floor) * (mps * mps))).astype(np.float32)
    assert w.dtype == np.float32 and w.shape == sig.shape and np.array_equal(w.view(np.uint32), want.view(np.uint32))
    assert w[0, 3] == 0.0 and w[0, 0] == np.float32(1.0 / (floor * floor * mps * mps))
    assert abs(w[0, 2] * (0.2 ** 2 + floor ** 2) * mps ** 2 - 1.0) < 1e-6        # m^-2: 1 / sigma_d^2
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma_floor"):
            xcorr.lag_weight(sig, fs, bad)
    with pytest.raises(ValueError, match="sigma_samples"):
        xcorr.lag_weight([0.1, float("nan")], fs, floor)
    with pytest.raises(ValueError, match="sample_rate_hz"):
        xcorr.lag_weight(sig, 0.0, floor)


def test_error_ellipse():
    k = math.sqrt(-2.0 * math.log(0.05))
    assert abs(k - 2.4477) < 5e-5
    a, b, ang = xcorr.error_ellipse([[9.0, 0.0, 4.0], [4.0, 0.0, 9.0]])
    assert np.allclose(a, 3 * k) and np.allclose(b, 2 * k) and np.allclose(ang, [0.0, math.pi / 2])
    for th in (0.3, -0.7, 1.2, -1.5):                  # axes 5 and 2, major axis at th from e1 towards e2
        c, s = math.cos(th), math.sin(th)
        cov = [25 * c * c + 4 * s * s, (25 - 4) * c * s, 25 * s * s + 4 * c * c]
        a, b, ang = xcorr.error_ellipse(cov, confidence=1.0 - math.exp(-0.5))      # scale 1: the 1-sigma ellipse
        assert abs(a - 5.0) < 1e-12 and abs(b - 2.0) < 1e-12 and abs(ang - th) < 1e-12
    a, b, ang = xcorr.error_ellipse([[np.inf, 0.0, np.inf], [1.0, 0.0, 1.0]])
    assert np.isposinf(a[0]) and np.isposinf(b[0]) and ang[0] == 0.0 and np.allclose([a[1], b[1]], k)
    with pytest.raises(ValueError, match="cov2"):
        xcorr.error_ellipse(np.zeros((4, 6)))
    with pytest.raises(ValueError, match="confidence"):
        xcorr.error_ellipse([1.0, 0.0, 1.0], confidence=1.0)


@pytest.mark.parametrize("lat,lng", [(37.0, -122.0), (-33.9, 18.4), (51.5, 0.1), (-45.0, -170.0)])
def test_tangent_plane(lat, lng):
    G = tp.GeodeticCalculator
    o, e, n = (np.array(v) for v in G.tangent_plane(lat, lng, 250.0))
    assert np.array_equal(o, np.array(G.lat_lng_to_xyz(lat, lng, 250.0)))
    assert abs(e @ e - 1.0) <= 1e-15 and abs(n @ n - 1.0) <= 1e-15 and abs(e @ n) <= 1e-15
    up = o / np.linalg.norm(o)
    assert abs(e @ up) <= 1e-15 and abs(n @ up) <= 1e-15 and np.allclose(np.cross(e, n), up, atol=1e-15)
    h = 1e-6                                            # degrees: a step of 0.1 m
    d_n = np.array(G.lat_lng_to_xyz(lat + h, lng, 250.0)) - o
    d_e = np.array(G.lat_lng_to_xyz(lat, lng + h, 250.0)) - o
    assert d_n @ n > 0.999 * np.linalg.norm(d_n) and d_e @ e > 0.999 * np.linalg.norm(d_e)
    # the sag the docstring quotes: d^2 / 2R below the plane at distance d
    for d, sag in ((3e3, 0.7), (10e3, 7.8), (32e3, 80.0)):
        p = np.array(G.lat_lng_to_xyz(lat + math.degrees(d / (G.EARTH_RADIUS_M + 250.0)), lng, 250.0))
        assert abs(-(p - o) @ up - sag) < 0.05 * sag and abs(d * d / (2 * G.EARTH_RADIUS_M) - sag) < 0.05 * sag
    assert "0.7 m at 3 km, 7.8 m at 10 km, 80 m at" in G.tangent_plane.__doc__


# -- 6. the binding -----------------------------------------------------------------------------------------------------------------------
class _NoCall(xcorr.XcorrEngine):
    def __init__(self):   # no library, no ctx: a C call would fail with AttributeError, not ValueError
        self.n_buoys, self.n_samples = 3, 16

    def __del__(self):
        pass


def _args(W=4, B=4):
    P = B * (B - 1) // 2
    return dict(buoy_xyz=np.arange(3.0 * B).reshape(B, 3), lag_int=np.zeros((W, P), np.int32),
                lag_frac=np.zeros((W, P), np.float32), sample_rate_hz=10e6)


_PLANE = np.array([1.0, 2.0, 3.0, 0.0, 0.6, 0.8, 1.0, 0.0, 0.0])
_BAD = {
    "lag_int 1-D": (dict(lag_int=np.zeros(6, np.int32), lag_frac=np.zeros(6, np.float32)), "lag_int"),
    "lag_frac one row": (dict(lag_frac=np.zeros(6, np.float32)), "lag_frac"),
    "lag_frac fewer windows": (dict(lag_frac=np.zeros((3, 6), np.float32)), "lag_frac"),
    "weight of length W": (dict(weight=np.ones(4, np.float32)), "weight"),
    "weight transposed": (dict(weight=np.ones((6, 4), np.float32)), "weight"),
    "one buoy": (dict(buoy_xyz=np.zeros((1, 3))), "buoy_xyz"),
    "65 buoys": (dict(buoy_xyz=np.zeros((65, 3))), "buoy_xyz"),
    "pairs of another length": (dict(pairs=np.zeros((5, 2), np.int32)), "pairs"),
    "no pairs, P != B(B-1)/2": (dict(lag_int=np.zeros((4, 5), np.int32), lag_frac=np.zeros((4, 5), np.float32)), "pairs"),
    "max_iter 0": (dict(max_iter=0), "max_iter"),
    "fs 0": (dict(sample_rate_hz=0.0), "sample_rate_hz"),
    "fs NaN": (dict(sample_rate_hz=float("nan")), "sample_rate_hz"),
    "plane of 8": (dict(plane=np.zeros(8)), "plane"),
    "plane [3][4]": (dict(plane=np.zeros((3, 4))), "plane"),
    "plane NaN": (dict(plane=np.where(np.arange(9) == 1, np.nan, _PLANE)), "plane"),
    "plane inf": (dict(plane=np.where(np.arange(9) == 4, np.inf, _PLANE)), "plane"),
    "e1 too long": (dict(plane=_PLANE * np.where((np.arange(9) // 3) == 1, 1.0 + 1e-8, 1.0)), "plane"),
    "e2 too short": (dict(plane=_PLANE * np.where((np.arange(9) // 3) == 2, 1.0 - 1e-8, 1.0)), "plane"),
    "e1 . e2": (dict(plane=np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1e-8, 1.0, 0.0])), "plane"),
}


@pytest.mark.parametrize("case", sorted(_BAD))
def test_solve_fix_refuses_before_any_call(case):
    change, name = _BAD[case]
    with pytest.raises(ValueError, match=name):
        _NoCall().solve_fix(**{**_args(), **change})


@pytest.mark.parametrize("change", [{}, dict(plane=_PLANE), dict(plane=_PLANE.reshape(3, 3), residuals=True),
                                    dict(weight=np.ones(6)), dict(pairs=np.zeros((6, 2), np.int32), max_iter=1)],
                         ids=["plain", "plane", "plane [3][3], residuals", "weight [P]", "pairs"])
def test_an_accepted_solve_fix_reaches_the_library(change):
    """the checks pass and the call goes to rmx_solve_batch_fix, once, and to no other entry"""
    eng = _Recording()
    out = eng.solve_fix(**{**_args(), **change})
    assert eng._lib.calls == ["rmx_solve_batch_fix"]
    assert isinstance(out, xcorr.SolveFix) and (out.resid is not None) == bool(change.get("residuals"))


def test_no_windows_is_no_call():
    for plane, n in ((None, 6), (_PLANE, 3)):
        out = _NoCall().solve_fix(np.zeros((4, 3)), np.zeros((0, 6), np.int32), np.zeros((0, 6), np.float32), 10e6,
                                  plane=plane, residuals=True)
        assert out.pos.shape == (0, 3) and out.cost.shape == (0,) and out.iters.shape == (0,)
        assert out.info.shape == (0, n) and out.cov.shape == (0, n) and out.resid.shape == (0, 6)


class _Recorder:
    """stands in for the loaded library: keeps what each entry would have read, and writes recognisable outputs"""

    def __init__(self, cov_row=None):
        self.seen, self.calls, self.cov_row = None, [], cov_row

    @staticmethod
    def _read(p, ctype, n):
        return None if p is None or p.value is None else np.array((ctype * n).from_address(p.value))

    @staticmethod
    def _write(p, values):
        values = np.ascontiguousarray(values, np.float64).reshape(-1)
        (C.c_double * values.size).from_address(p.value)[:] = list(values)

    def rmx_solve_batch(self, ctx, bx, B, pp, P, li, lf, wp, fs, W, max_iter, pos, cost, iters, flags):
        self.calls.append("rmx_solve_batch")
        self.seen = dict(weight=self._read(wp, C.c_float, W * P))
        buoys = self._read(bx, C.c_double, 3 * B).reshape(B, 3)
        self._write(pos, np.tile(buoys[0], (W, 1)) + np.arange(W)[:, None])
        self._write(cost, 6.0 * (1 + np.arange(W)))
        return 0

    def rmx_solve_batch_fix(self, ctx, bx, B, pp, P, li, lf, wp, fs, plane, W, max_iter, pos, cost, iters, info, cov, resid,
                            flags):
        self.calls.append("rmx_solve_batch_fix")
        n = 6 if plane is None or plane.value is None else 3
        self.seen = dict(B=B, P=P, W=W, fs=fs, max_iter=max_iter, flags=flags, weight=self._read(wp, C.c_float, W * P),
                         plane=self._read(plane, C.c_double, 9), pairs=self._read(pp, C.c_int32, 2 * P),
                         has_resid=not (resid is None or resid.value is None), n=n)
        buoys = self._read(bx, C.c_double, 3 * B).reshape(B, 3)
        self._write(pos, np.tile(buoys[0], (W, 1)))
        self._write(cost, 1.5 * (1 + np.arange(W)))
        row = self.cov_row if self.cov_row is not None else ([4.0, 0.0, 1.0] if n == 3 else [1.0, 0.0, 0.0, 1.0, 0.0, 1.0])
        self._write(cov, np.tile(row, (W, 1)))
        return 0


class _Recording(_NoCall):
    def __init__(self, **kw):
        super().__init__()
        self._lib, self._ctx = _Recorder(**kw), None

    def _check(self, rc):
        assert rc == 0


def test_solve_fix_hands_over_plane_weight_and_residual_pointer():
    eng = _Recording()
    row = np.linspace(0.5, 3.0, 6)
    out = eng.solve_fix(**_args(W=5), weight=row, plane=_PLANE.reshape(3, 3), residuals=True)
    seen = eng._lib.seen
    assert seen["W"] == 5 and seen["P"] == 6 and seen["B"] == 4 and seen["flags"] == 0 and seen["has_resid"]
    assert np.array_equal(seen["plane"], _PLANE) and seen["pairs"] is None
    assert np.array_equal(seen["weight"].reshape(5, 6), np.tile(row.astype(np.float32), (5, 1)))
    assert out.info.shape == (5, 3) and out.cov.shape == (5, 3) and out.resid.shape == (5, 6)
    assert isinstance(out, xcorr.SolveFix) and out._fields == ("pos", "cost", "iters", "info", "cov", "resid")
    out = eng.solve_fix(**_args(W=5))
    seen = eng._lib.seen
    assert seen["plane"] is None and seen["weight"] is None and not seen["has_resid"]
    assert out.info.shape == (5, 6) and out.cov.shape == (5, 6) and out.resid is None


def _fleet():
    return [tp.BuoyPosition("b%d" % i, 37.0 + 0.03 * i, -122.0 + 0.05 * (i % 2), 0.0) for i in range(4)]


def test_triangulate_batch_without_the_new_keywords_is_unchanged():
    G = tp.GeodeticCalculator
    buoys = _fleet()
    li, lf = np.zeros((3, 6), np.int32), np.zeros((3, 6), np.float32)
    conf = np.linspace(0.3, 0.9, 6)
    for confidence in (None, conf):
        eng = _Recording()
        out = tp.HyperbolicPositioning().triangulate_batch(eng, buoys, li, lf, 10e6, confidence=confidence)
        assert eng._lib.calls == ["rmx_solve_batch"]
        b0 = np.array(G.lat_lng_to_xyz(buoys[0].lat, buoys[0].lng, buoys[0].altitude))
        want = [G.xyz_to_lat_lng(*(b0 + w)) + (math.sqrt(6.0 * (1 + w) / 6),) for w in range(3)]
        assert out == want and all(len(t) == 4 for t in out)
        if confidence is not None:
            assert np.array_equal(eng._lib.seen["weight"].reshape(3, 6), np.tile((1.0 / (conf + 0.1)).astype(np.float32), (3, 1)))


def test_triangulate_batch_keyword_rules():
    hp, buoys = tp.HyperbolicPositioning(), _fleet()
    li, lf = np.zeros((3, 6), np.int32), np.zeros((3, 6), np.float32)
    sig = np.full((3, 6), 0.1)
    for kw in (dict(lag_sigma=sig), dict(sigma_floor=0.05)):
        with pytest.raises(ValueError, match="lag_sigma and sigma_floor"):
            hp.triangulate_batch(_Recording(), buoys, li, lf, 10e6, **kw)
    with pytest.raises(ValueError, match="confidence"):
        hp.triangulate_batch(_Recording(), buoys, li, lf, 10e6, confidence=np.ones(6), lag_sigma=sig, sigma_floor=0.05)
    with pytest.raises(ValueError, match="sigma_floor"):
        hp.triangulate_batch(_Recording(), buoys, li, lf, 10e6, lag_sigma=sig, sigma_floor=0.0)


def test_triangulate_batch_in_the_plane_reports_ellipse_drms_chi2_and_dof():
    G = tp.GeodeticCalculator
    hp, buoys = tp.HyperbolicPositioning(), _fleet()
    li, lf = np.zeros((3, 6), np.int32), np.zeros((3, 6), np.float32)
    sig = np.full((3, 6), 0.1)
    sig[1, 2] = sig[1, 4] = np.inf                       # two dead pairs in window 1
    eng = _Recording()                                   # cov = (4, 0, 1): 2 m east, 1 m north
    out = hp.triangulate_batch(eng, buoys, li, lf, 10e6, lag_sigma=sig, sigma_floor=0.05, altitude_m=12.0)
    seen = eng._lib.seen
    assert eng._lib.calls == ["rmx_solve_batch_fix"]
    assert np.array_equal(seen["weight"].reshape(3, 6), xcorr.lag_weight(sig, 10e6, 0.05))
    xyz = np.array([G.lat_lng_to_xyz(b.lat, b.lng, b.altitude) for b in buoys])
    lat0, lng0, _ = G.xyz_to_lat_lng(*xyz.mean(axis=0))
    assert np.array_equal(seen["plane"], np.array(G.tangent_plane(lat0, lng0, 12.0)).reshape(-1))
    k = math.sqrt(-2.0 * math.log(0.05))
    for w, t in enumerate(out):
        assert len(t) == 5 and t[:3] == G.xyz_to_lat_lng(*xyz[0])
        extra = t[4]
        assert sorted(extra) == ["chi2", "dof", "drms_m", "ellipse_m"]
        assert t[3] == extra["drms_m"] == math.sqrt(5.0) and extra["chi2"] == 1.5 * (1 + w)
        assert extra["dof"] == (2 if w == 1 else 4)
        assert np.allclose(extra["ellipse_m"], (2 * k, 1 * k, 90.0))      # the major axis points east: 90 degrees from north
    # a major axis towards the north-east reads 45 degrees; a singular covariance reads inf
    out = hp.triangulate_batch(_Recording(cov_row=[2.5, 1.5, 2.5]), buoys, li, lf, 10e6, altitude_m=0.0)
    assert np.allclose(out[0][4]["ellipse_m"], (2 * k, 1 * k, 45.0)) and out[0][4]["dof"] == 4
    out = hp.triangulate_batch(_Recording(cov_row=[np.inf, 0.0, np.inf]), buoys, li, lf, 10e6, altitude_m=0.0)
    assert out[0][3] == math.inf and out[0][4]["ellipse_m"][0] == math.inf


def test_triangulate_batch_with_three_unknowns_takes_the_east_north_block():
    G = tp.GeodeticCalculator
    hp, buoys = tp.HyperbolicPositioning(), _fleet()
    li, lf = np.zeros((2, 6), np.int32), np.zeros((2, 6), np.float32)
    b0 = buoys[0]
    _, e, n = (np.array(v) for v in G.tangent_plane(b0.lat, b0.lng))
    up = np.cross(e, n)
    full = 9.0 * np.outer(e, e) + 4.0 * np.outer(n, n) + 1e4 * np.outer(up, up)      # 3 m east, 2 m north, 100 m up
    row = [full[0, 0], full[0, 1], full[0, 2], full[1, 1], full[1, 2], full[2, 2]]
    eng = _Recording(cov_row=row)
    out = hp.triangulate_batch(eng, buoys, li, lf, 10e6, lag_sigma=np.full(6, 0.1), sigma_floor=0.05)
    assert eng._lib.seen["plane"] is None and eng._lib.seen["n"] == 6
    for t in out:
        assert len(t) == 5 and t[4]["ellipse_m"] is None and t[4]["dof"] == 3
        assert abs(t[3] - math.sqrt(13.0)) < 1e-6 and t[3] == t[4]["drms_m"]
    out = hp.triangulate_batch(_Recording(cov_row=[np.inf, 0, 0, np.inf, 0, np.inf]), buoys, li, lf, 10e6,
                               lag_sigma=np.full(6, 0.1), sigma_floor=0.05)
    assert out[0][3] == math.inf


# -- 7. the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_prototypes_name_the_entry():
    assert "rmx_solve_batch_fix" in xcorr.EXPORTS
    header = open(os.path.join(ROOT, "include", "rmx.h")).read()
    decl = re.search(r"int rmx_solve_batch_fix\(rmx_ctx\* ctx,([^;]*)\);", header)
    assert decl, "the header declares the entry"
    n_args = decl.group(0).count(",") + 1
    doc = header[header.index("rmx_solve_batch with a surface constraint"):decl.start()]
    for said in ("xx xy xz yy yz zz", "11 12 22", "1e-12", "+inf", "cofactor", "dilution of precision", "B - 1 independent",
                 "optimistic", "NULL = three unknowns", "n_windows == 0 returns RMX_OK", "No output is ever NaN"):
        assert said in doc, said
    binding = open(os.path.join(ROOT, "radio-mapper_amd", "xcorr.py")).read()
    proto = re.search(r"lib\.rmx_solve_batch_fix\.argtypes = \[([^\]]*)\]", binding)
    assert proto and proto.group(1).count(",") + 1 == n_args == 19
    assert "lib.rmx_solve_batch_fix.restype = ci" in binding
    src = open(os.path.join(ROOT, "radio-mapper_amd", "csrc", "rmx_hip.hip")).read()
    assert src.index("int rmx_solve_batch_fix(") > src.index("int rmx_solve_batch(")
    kernels = open(os.path.join(ROOT, "radio-mapper_amd", "csrc", "solve_path.hpp")).read()
    for name in ("void k_solve_plane(", "void k_solve_fix("):        # each new kernel's body opens with the pragma
        body = kernels[kernels.index(name):]
        body = body[body.index(") {") + 3:]
        assert body.lstrip().startswith("#pragma clang fp contract(off)"), name
