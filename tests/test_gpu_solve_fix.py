"""k_solve_plane and k_solve_fix through rmx_solve_batch_fix against their kernel-order restatement
(tests/solve_fix_ref.py): pos, cost, iters, info, cov and resid equal bit for bit (np.array_equal) for EVERY window, in both
modes, with and without weights and residuals; pos, cost and iters without a plane equal XcorrEngine.solve's; custom pair
lists, max_iter, the degenerate inputs of tests/test_solve_fix_cpu.py, the pointer flags, the refusals and ctx reuse through
the raw ABI; and the chain correlate -> lag_sigma -> lag_weight -> solve_fix.  The restatement itself is held to
numpy.linalg and to the statistics in tests/test_solve_fix_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import radio_mapper_amd as rm
import solve_fix_ref as fr
import solve_kernel_ref as kr
from radio_mapper_amd.tdoa_processor import GeodeticCalculator as G
from test_solve import scenario
from test_solve_fix_cpu import centroid_on_a_buoy, collinear_in_plane

pytestmark = pytest.mark.gpu

FS = 10e6
MPS = kr.metres_per_sample(FS)
RMX_E_INVAL = -1
NAMES = ("pos", "cost", "iters", "info", "cov", "resid")


@pytest.fixture(scope="module")
def xc():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    assert xcorr.device_count() > 0, "no MI355X visible"
    return xcorr


def _engine(xc):
    # the solve entries use nothing of the ctx but its stream and its solve buffers: any engine will do
    return xc.XcorrEngine(3, 256, 2)


def _weights(shape):
    return (1.0 / (np.random.default_rng(3).uniform(0.2, 1.0, shape) + 0.1)).astype(np.float32)


def _plane_of(buoys, alt=100.0):
    """the tangent plane at the centroid's lat/lng, as triangulate_batch(altitude_m=alt) forms it"""
    lat, lng, _ = G.xyz_to_lat_lng(*buoys.mean(axis=0))
    return fr.as_plane(*G.tangent_plane(lat, lng, alt))


_REF = {}


def _ref(key, buoys, pairs, li, lf, wgt, plane, max_iter=60, mps=MPS):
    """the restatement's six outputs, computed once per case and shared read-only"""
    if key not in _REF:
        out = fr.solve_fix_kernel_order(buoys, pairs, li, lf, wgt, mps, plane, max_iter)
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _assert_exact(got, ref, what):
    """got: a SolveFix or six arrays (resid may be None: then it is not compared)"""
    bad = []
    for name, g, r in zip(NAMES, got, ref):
        if name == "resid" and g is None:
            continue
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        assert not np.any(np.isnan(g)), (what, name, "NaN")
        if not np.array_equal(g, r):
            rows = np.flatnonzero(np.any((g != r).reshape(len(g), -1), axis=1))
            with np.errstate(all="ignore"):
                bad.append("%s: %d of %d windows differ (first %s), max |d| %.3e" % (
                    name, len(rows), len(g), rows[:5], np.nanmax(np.abs(g.astype(np.float64) - r))))
    assert not bad, what + ": " + "; ".join(bad)


# -- 1. every output, both modes, by shape ----------------------------------------------------------------------------------------
# 64 threads a block: one lane; a full block; a block and one lane; three blocks, the last partial; 2016 pairs
SHAPES = [(3, 1), (4, 64), (5, 65), (8, 130), (64, 3)]


def _case(B, W):
    buoys, tx, pairs, li, lf, fs = scenario(B, W, seed=20 + B, noise_m=3.0)
    assert fs == FS
    return buoys, pairs, li, lf


@pytest.mark.parametrize("residuals", [True, False], ids=["resid", "no_resid"])
@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "no_weights"])
@pytest.mark.parametrize("plane_mode", [True, False], ids=["plane", "three_unknowns"])
@pytest.mark.parametrize("B,W", SHAPES)
def test_every_output_bit_for_bit(xc, B, W, plane_mode, weighted, residuals):
    buoys, pairs, li, lf = _case(B, W)
    wgt = _weights(li.shape) if weighted else None
    plane = _plane_of(buoys) if plane_mode else None
    ref = _ref(("case", B, W, plane_mode, weighted), buoys, pairs, li, lf, wgt, plane)
    with _engine(xc) as eng:
        got = eng.solve_fix(buoys, li, lf, FS, weight=wgt, plane=plane, residuals=residuals)
    assert (got.resid is not None) == residuals
    assert np.all(np.isfinite(got.info)) and np.all(np.isfinite(got.pos))
    _assert_exact(got, ref, "B %d W %d" % (B, W))


# -- 2. without a plane the walk is rmx_solve_batch's ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,W", [(4, 64), (8, 130)])
def test_without_a_plane_the_fix_is_solves(xc, B, W):
    buoys, pairs, li, lf = _case(B, W)
    wgt = _weights(li.shape)
    with _engine(xc) as eng:
        for w in (wgt, None):
            pos, cost, it = eng.solve(buoys, li, lf, FS, weight=w)
            got = eng.solve_fix(buoys, li, lf, FS, weight=w)
            assert np.array_equal(got.pos, pos) and np.array_equal(got.cost, cost) and np.array_equal(got.iters, it)


# -- 3. custom pair lists and max_iter ------------------------------------------------------------------------------------------------
CUSTOM5 = np.array([[0, 1], [0, 1], [2, 2], [4, 0], [3, 1], [0, 2], [0, 3], [0, 4]], np.int32)   # a repeat, (i, i), reversed, a star


def _custom():
    buoys, tx, *_ = scenario(5, 65, seed=25, noise_m=3.0)
    dist = np.linalg.norm(tx[:, None, :] - buoys[None, :, :], axis=2)
    dd = dist[:, CUSTOM5[:, 1]] - dist[:, CUSTOM5[:, 0]] + np.random.default_rng(77).normal(0.0, 3.0, (65, len(CUSTOM5)))
    lag = dd / kr.SPEED_OF_LIGHT * FS
    li = np.round(lag).astype(np.int32)
    return buoys, CUSTOM5, li, (lag - li).astype(np.float32), _weights(li.shape)


@pytest.mark.parametrize("plane_mode", [True, False], ids=["plane", "three_unknowns"])
def test_custom_pair_list(xc, plane_mode):
    buoys, pairs, li, lf, wgt = _custom()
    plane = _plane_of(buoys) if plane_mode else None
    ref = _ref(("custom", plane_mode), buoys, pairs, li, lf, wgt, plane)
    with _engine(xc) as eng:
        got = eng.solve_fix(buoys, li, lf, FS, weight=wgt, pairs=pairs, plane=plane, residuals=True)
    _assert_exact(got, ref, "custom list")
    assert np.all(got.resid[:, 2] == -(li[:, 2].astype(np.float64) + lf[:, 2].astype(np.float64)) * MPS)      # the (i, i) pair


@pytest.mark.parametrize("plane_mode", [True, False], ids=["plane", "three_unknowns"])
@pytest.mark.parametrize("k", [1, 2, 200])
def test_max_iter(xc, k, plane_mode):
    buoys, tx, pairs, li, lf, _ = scenario(4, 130, seed=14, noise_m=5.0)
    wgt = _weights(li.shape)
    plane = _plane_of(buoys) if plane_mode else None
    ref = _ref(("max_iter", k, plane_mode), buoys, pairs, li, lf, wgt, plane, max_iter=k)
    with _engine(xc) as eng:
        got = eng.solve_fix(buoys, li, lf, FS, weight=wgt, max_iter=k, plane=plane, residuals=True)
    assert got.iters.max() <= k and (k > 2 or np.all(got.iters == k))
    _assert_exact(got, ref, "max_iter %d" % k)


# -- 4. the degenerate cases -----------------------------------------------------------------------------------------------------------
def _degenerate(name):
    """(buoys, pairs, lag_int, lag_frac, weight or None, plane or None, sample rate, every window singular?)"""
    if name.startswith("zero_weights"):
        buoys, pairs, li, lf = _case(5, 65)
        return buoys, pairs, li, lf, np.zeros(li.shape, np.float32), _plane_of(buoys) if name.endswith("plane") else None, FS, True
    if name.startswith("centroid_on_a_buoy"):
        buoys, pairs, li, lf, plane = centroid_on_a_buoy(name.endswith("plane"))
        return buoys, pairs, li, lf, None, plane, FS, True
    if name == "collinear_plane":
        buoys, pairs, li, lf, plane = collinear_in_plane()
        return buoys, pairs, li, lf, None, plane, fr.FS_SCENE, True
    sea = {"sea3_three_unknowns": "sea3", "sea5_three_unknowns": "sea5"}[name]
    buoys, emitter, plane = fr.scene(sea)
    pairs, li, lf, wgt = fr.noisy_lags(buoys, emitter, 70, seed=6)
    return buoys, pairs, li, lf, wgt, None, fr.FS_SCENE, sea == "sea3"


@pytest.mark.parametrize("name", ["zero_weights", "zero_weights_plane", "centroid_on_a_buoy", "centroid_on_a_buoy_plane",
                                  "collinear_plane", "sea3_three_unknowns", "sea5_three_unknowns"])
def test_degenerate_inputs_have_no_nan_and_are_exact(xc, name):
    buoys, pairs, li, lf, wgt, plane, fs, singular = _degenerate(name)
    ref = _ref(("degenerate", name), buoys, pairs, li, lf, wgt, plane, mps=kr.metres_per_sample(fs))
    with _engine(xc) as eng:
        got = eng.solve_fix(buoys, li, lf, fs, weight=wgt, plane=plane, residuals=True)
    for a in got:
        assert not np.any(np.isnan(a))
    n = got.cov.shape[1]
    diag = [0, 2] if n == 3 else [0, 3, 5]
    off = [k for k in range(n) if k not in diag]
    if singular:
        assert np.all(np.isposinf(got.cov[:, diag])) and np.all(got.cov[:, off] == 0.0)
    else:
        assert np.all(np.isfinite(got.cov))
    if name.startswith(("zero_weights", "centroid")):
        assert np.all(got.info == 0.0)
    _assert_exact(got, ref, name)


# -- 5. the raw ABI -----------------------------------------------------------------------------------------------------------------------
def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _tp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _guarded(W, P, n):
    return [np.full((W, 3), -77.0), np.full(W, -77.0), np.full(W, -77, np.int32), np.full((W, n), -77.0),
            np.full((W, n), -77.0), np.full((W, P), -77.0)]


def _untouched(o):
    return all(np.all(a == -77) for a in o)


@pytest.mark.parametrize("plane_mode", [True, False], ids=["plane", "three_unknowns"])
def test_pointer_flags_through_the_raw_abi(xc, plane_mode):
    import torch
    buoys, tx, pairs, li, lf, _ = scenario(8, 130, seed=18, noise_m=10.0)
    wgt = _weights(li.shape)
    W, P = li.shape
    plane = _plane_of(buoys) if plane_mode else None
    n = 3 if plane_mode else 6
    ref = _ref(("flags", plane_mode), buoys, pairs, li, lf, wgt, plane)
    lib = xc.load_library()
    dev = torch.device("cuda", 0)
    ins_d = [torch.from_numpy(a).to(dev) for a in (li, lf, wgt)]
    got = {}
    with _engine(xc) as eng:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        for flags in (0, xc.RMX_IN_DEVICE, xc.RMX_OUT_DEVICE, xc.RMX_IN_DEVICE | xc.RMX_OUT_DEVICE):
            ins = [_tp(t) for t in ins_d] if flags & xc.RMX_IN_DEVICE else [_vp(li), _vp(lf), _vp(wgt)]
            o = _guarded(W, P, n)
            if flags & xc.RMX_OUT_DEVICE:
                o = [torch.from_numpy(a).to(dev) for a in o]
                outs = [_tp(t) for t in o]
            else:
                outs = [_vp(a) for a in o]
            torch.cuda.synchronize()
            rc = lib.rmx_solve_batch_fix(eng._ctx, _vp(buoys), 8, None, P, *ins, FS, _vp(plane), W, 60, *outs, flags)
            assert rc == 0, (flags, lib.rmx_last_error(eng._ctx))
            assert lib.rmx_synchronize(eng._ctx) == 0
            got[flags] = [t.cpu().numpy() if flags & xc.RMX_OUT_DEVICE else t for t in o]
    for flags in (0, 1, 2, 3):
        _assert_exact(got[flags], ref, "flags %d" % flags)


def _refusals():
    """every refusal of rmx_solve_batch, case by case as tests/test_gpu_solve_exact.py lists them, and the new entry's own on
    top.  A case may bring its own lag arrays; `cols` is then the width of the guarded resid."""
    B, W, P = 5, 3, 10
    bad_lo, bad_hi = kr.all_pairs(B), kr.all_pairs(B)
    bad_lo[4, 1], bad_hi[9, 0] = -1, B
    many = np.zeros((2017, 2), np.int32)
    many[:, 1] = 1
    big = dict(li=np.zeros((W, 2017), np.int32), lf=np.zeros((W, 2017), np.float32), wgt=None, cols=2017)
    ok = fr.as_plane((1.0, 2.0, 3.0), (0.0, 0.6, 0.8), (1.0, 0.0, 0.0))

    def changed(k, v):
        p = ok.copy()
        p[k] = v
        return p
    out = {
        # rmx_solve_batch's
        "n_buoys 1": dict(n_buoys=1, n_pairs=0), "n_buoys 65": dict(n_buoys=65, n_pairs=0),
        "fs 0": dict(fs=0.0), "fs -1": dict(fs=-1.0), "fs NaN": dict(fs=float("nan")),
        "max_iter 0": dict(max_iter=0), "n_windows -1": dict(n_windows=-1),
        "pair index -1": dict(pairs=bad_lo), "pair index n_buoys": dict(pairs=bad_hi),
        "no list, n_pairs 7": dict(n_pairs=7), "no list, n_pairs 11": dict(n_pairs=11),
        "2017 pairs": dict(pairs=many, n_pairs=2017, **big),
        "2017 pairs, three unknowns": dict(pairs=many, n_pairs=2017, plane=None, **big),
        "a list of 0 pairs": dict(pairs=kr.all_pairs(B), n_pairs=0),
        # the new entry's
        "plane NaN": dict(plane=changed(0, np.nan)), "plane inf": dict(plane=changed(5, np.inf)),
        "plane -inf in e2": dict(plane=changed(8, -np.inf)),
        "e1 too long": dict(plane=changed(3, 1e-4)), "e2 too short": dict(plane=changed(6, 1.0 - 1e-8)),
        "e1 . e2": dict(plane=changed(7, 1e-8)),
    }
    for name in ("buoys", "li", "lf", "pos", "cost", "iters", "info", "cov"):
        out["NULL " + name] = {name: None}
    out["NULL info, three unknowns"] = dict(info=None, plane=None)
    out["NULL cov, three unknowns"] = dict(cov=None, plane=None)
    return out, ok


@pytest.mark.parametrize("name", sorted(_refusals()[0]))
def test_refusals_leave_the_outputs_alone_and_the_ctx_usable(xc, name):
    B, W, P = 5, 3, 10
    buoys, tx, pairs, li, lf, _ = scenario(B, W, seed=45, noise_m=3.0)
    wgt = _weights(li.shape)
    cases, plane = _refusals()
    ref = _ref(("refusal", "valid"), buoys, pairs, li, lf, wgt, plane)
    lib = xc.load_library()

    def call(eng, o, **kw):
        a = dict(buoys=buoys, n_buoys=B, pairs=None, n_pairs=P, li=li, lf=lf, wgt=wgt, fs=FS, plane=plane, n_windows=W,
                 max_iter=60, pos=o[0], cost=o[1], iters=o[2], info=o[3], cov=o[4], resid=o[5])
        a.update(kw)
        return lib.rmx_solve_batch_fix(eng._ctx, _vp(a["buoys"]), a["n_buoys"], _vp(a["pairs"]), a["n_pairs"], _vp(a["li"]),
                                       _vp(a["lf"]), _vp(a["wgt"]), a["fs"], _vp(a["plane"]), a["n_windows"], a["max_iter"],
                                       _vp(a["pos"]), _vp(a["cost"]), _vp(a["iters"]), _vp(a["info"]), _vp(a["cov"]),
                                       _vp(a["resid"]), 0)

    case = dict(cases[name])
    cols = case.pop("cols", P)
    with _engine(xc) as eng:
        o = _guarded(W, cols, 6)            # (info and cov guarded at the wider of the two layouts)
        assert call(eng, o, **case) == RMX_E_INVAL
        assert len(lib.rmx_last_error(eng._ctx) or b"") > 0
        assert _untouched(o)
        o = _guarded(W, P, 3)
        assert call(eng, o) == 0
        _assert_exact(o, ref, "the valid call after the refusal: " + name)


def test_no_windows_is_ok_and_writes_nothing(xc):
    buoys, tx, pairs, li, lf, _ = scenario(5, 3, seed=45, noise_m=3.0)
    lib = xc.load_library()
    with _engine(xc) as eng:
        for plane, n in ((None, 6), (_refusals()[1], 3)):
            o = _guarded(3, 10, n)
            rc = lib.rmx_solve_batch_fix(eng._ctx, _vp(buoys), 5, None, 10, _vp(li), _vp(lf), None, FS, _vp(plane), 0, 60,
                                         *map(_vp, o), 0)
            assert rc == 0 and lib.rmx_synchronize(eng._ctx) == 0 and _untouched(o)
        out = eng.solve_fix(buoys, li[:0], lf[:0], FS)
        assert out.pos.shape == (0, 3) and out.cov.shape == (0, 6)


def test_one_ctx_through_growing_and_shrinking_calls_that_alternate_modes(xc):
    """sv_in / sv_out / sv_pairs grow, are reused by smaller calls, by the other mode and by rmx_solve_batch between them:
    every result is the restatement's"""
    steps = []
    for n, (B, W) in enumerate([(5, 3), (16, 130), (3, 1), (8, 70), (16, 130), (4, 2)]):
        buoys, tx, pairs, li, lf, _ = scenario(B, W, seed=40 + B, noise_m=3.0)
        steps.append((B, W, n % 2 == 0, buoys, pairs, li, lf, _weights(li.shape)))
    with _engine(xc) as eng:
        for n, (B, W, plane_mode, buoys, pairs, li, lf, wgt) in enumerate(steps):
            plane = _plane_of(buoys) if plane_mode else None
            got = eng.solve_fix(buoys, li, lf, FS, weight=wgt, plane=plane, residuals=n % 3 != 2)
            _assert_exact(got, _ref(("ctx", B, W, plane_mode), buoys, pairs, li, lf, wgt, plane), "step %d" % n)
            plain = eng.solve(buoys, li, lf, FS, weight=wgt)
            if not plane_mode:
                assert all(np.array_equal(a, b) for a, b in zip(plain, got[:3]))


# -- 6. the chain -------------------------------------------------------------------------------------------------------------------------
def test_correlate_quality_to_weights_to_fix(xc):
    """correlate(refine=8, quality=True) -> lag_sigma -> lag_weight -> solve_fix in both modes: what the restatement gives for
    the same lags and weights"""
    B, W, N = 4, 3, 256
    fs = fr.FS_SCENE
    buoys, emitter, plane = fr.scene("sea4")
    iq, _ = rm.synth.make_windows(W, B, N, fs, seed=3, max_delay=20)
    iq = np.ascontiguousarray(iq, dtype=np.complex64)
    with xc.XcorrEngine(B, N, W) as eng:
        li, lf, pk, q = eng.correlate(iq, refine=8, quality=True)
        sigma = xc.lag_sigma(q)
        wgt = xc.lag_weight(sigma, fs, 0.05)
        assert wgt.shape == li.shape and wgt.dtype == np.float32 and np.all(np.isfinite(wgt)) and np.all(wgt >= 0)
        assert np.any(wgt > 0)
        for pl in (plane, None):
            got = eng.solve_fix(buoys, li, lf, fs, weight=wgt, plane=pl, residuals=True)
            ref = _ref(("chain", pl is None), buoys, kr.all_pairs(B), li, lf, wgt, pl, mps=kr.metres_per_sample(fs))
            _assert_exact(got, ref, "chain, %s" % ("three unknowns" if pl is None else "plane"))
