"""rmx_caf_batch_request, the Doppler search under a band, PHAT and lag bounds with its sub-grid Doppler estimate, on the
GPU: every route of rmx_caf_batch against the float32 restatement (tests/caf_request_ref.py), per-window bounds and bands
under the one-launch path and across chunk seams, the rotation, the weighting and the selection bit for bit against the
engine's own correlate(), the identities with rmx_caf_batch, the DC-offset scene, the pointer flags, the state an engine
keeps between calls, and the refusals.

Parity is the rule of tests/test_gpu_caf.py (its _assert_parity, imported), with no lag excused: tests/test_caf_request_cpu.py
holds every case's winner more than 1e-5 above its runner-up on the reference alone.  dop_frac agrees within 1e-5 or
within what one float32 ulp on each of its three taps moves it.  Every call also reads rmx_last_timing_kind: a request
call launches, family by family, exactly what the plain call launches."""
import ctypes as C

import numpy as np
import pytest

import caf_ref as cr
import caf_request_ref as rr
from test_gpu_caf import _assert_parity, _engine, _expected, _launches

pytestmark = pytest.mark.gpu
NAMES = ("dop_idx", "dop_frac", "lag_int", "lag_frac", "peak")


@pytest.fixture(scope="module")
def xc():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    if xcorr.device_count() < 1:
        pytest.fail("no GPU visible")
    return xcorr


@pytest.fixture
def opts(xc):
    xc.clear_default_options()
    yield xc.set_default_option
    xc.clear_default_options()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _assert_same(a, b, what="", names=None):
    names = names or (NAMES if len(a) == 5 else ("dop_idx", "lag_int", "lag_frac", "peak"))
    assert len(a) == len(b) == len(names), what
    for name, u, v in zip(names, a, b):
        assert u.dtype == v.dtype and u.shape == v.shape, (what, name)
        assert np.array_equal(_bits(u), _bits(v)), "%s %s: %d of %d elements differ" % (what, name, int((_bits(u) != _bits(v)).sum()), u.size)


def _four(fine_out):
    """(dop_idx, lag_int, lag_frac, peak) of a fine=True result"""
    return (fine_out[0],) + tuple(fine_out[2:])


def _assert_request_parity(fine_out, ref):
    """test_gpu_caf's rule on the four arrays, no lag excused, and dop_frac"""
    dop, dfrac, li, lf, pk = fine_out
    assert float(ref["lag_margin"].min()) > rr.LAG_MARGIN_BAR        # (the condition test_caf_request_cpu.py checks)
    _assert_parity((dop, li, lf, pk), ref)
    assert np.array_equal(li, ref["lag_int"]), "%d integer lags differ (none is excused)" % int((li != ref["lag_int"]).sum())
    assert dfrac.dtype == np.float32 and dfrac.shape == dop.shape
    err = np.abs(dfrac.astype(np.float64) - ref["dop_frac"].astype(np.float64))
    print("worst dop_frac error %.3e (three-tap bound there %.3e)" % (err.max(), ref["dop_frac_bound"].ravel()[np.argmax(err)]))
    assert np.all((err <= 1e-5) | (err <= ref["dop_frac_bound"])), "dop_frac outside the rule: %.3e" % err.max()
    D = ref["bin_peak"].shape[-1]
    assert np.all(dfrac > -0.5) and np.all(dfrac <= 0.5) and not np.any(dfrac[(dop == 0) | (dop == D - 1)])


# ---- 1. every route against the restatement -------------------------------------------------------------------------------
# (id, scene, kind, chunks, default options, engine options, row family with the default list / with the custom one)
ROUTES = [
    ("small N=16", "n16", "small", 1, {}, (), None, None),
    ("small N=256", "n256", "small", 1, {}, (), None, None),
    ("small N=4096 generic4096", "g4096", "small", 1, {"generic4096": 1}, (), None, None),
    ("four-step N=8192", "n8192", "four", 1, {}, (), "g_rows_inv", "g_rows_inv"),
    ("four-step N=8192 anchor", "n8192b6", "four", 1, {}, (), "g_rows_anchor", "g_rows_inv"),
    ("one launch DW=40 resident=1", "one8", "one", 1, {}, (("resident", 1),), None, None),
    ("one launch DW=40 resident=0", "one8", "one", 1, {}, (("resident", 0),), None, None),
    ("one launch DW=21 resident=1", "one3", "one", 1, {}, (("resident", 1),), None, None),
    ("one launch DW=21 resident=0", "one3", "one", 1, {}, (("resident", 0),), None, None),
    ("per hypothesis chunks 8+8+4 resident=1", "chunked", "per", 3, {}, (("chunk_windows", 8), ("resident", 1)), None, None),
    ("per hypothesis chunks 8+8+4 resident=0", "chunked", "per", 3, {}, (("chunk_windows", 8), ("resident", 0)), None, None),
]


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_against_the_reference(xc, opts, route):
    """{PHAT, a band, shared bounds, per-window bounds + per-window bands + PHAT} x {default, custom pair list} x {complex64,
    uint8} x {fine off, on}: the plain call's launch counts, uint8 bit-identical to complex64, fine=True's four arrays
    bit-identical to the call without it, parity."""
    _, name, kind, chunks, defaults, eng_opts, rows_def, rows_custom = route
    for k, v in defaults.items():
        opts(k, v)
    with _engine(xc, *[cr.SCENES[name][i] for i in (1, 2, 0)], eng_opts) as eng:
        for custom in (False, True):
            want = _expected(kind, cr.SCENES[name][3], chunks, rows_custom if custom else rows_def)
            for rid in rr.REQUEST_IDS:
                case = "%s/%s/%s" % (name, "custom" if custom else "default", rid)
                iq, raw, grid, pairs, kw = rr.case(case)
                got = eng.caf(iq, grid, pairs, **kw)
                assert _launches(eng) == want, (case, _launches(eng))
                fine = eng.caf(iq, grid, pairs, fine=True, **kw)
                assert _launches(eng) == want, (case, "fine", _launches(eng))
                _assert_same(_four(fine), got, case + ": fine=True against fine=False")
                got8 = eng.caf(raw, grid, pairs, fine=True, **kw)
                assert _launches(eng) == want, (case, "uint8", _launches(eng))
                _assert_same(got8, fine, case + ": uint8 against complex64")
                _assert_same(eng.caf(raw, grid, pairs, **kw), got, case + ": uint8 against complex64, fine=False")
                print(case)
                _assert_request_parity(fine, rr.case_reference(case))


# ---- 2. per-window bounds and bands reach their own window under every hypothesis ----------------------------------------
# (id, N, W, default options of the cut engine, engine options, kind, chunks)
OWN = [
    ("one launch resident=1", 4096, 3, {}, (("resident", 1),), "one", 1),
    ("one launch resident=0", 4096, 3, {}, (("resident", 0),), "one", 1),
    ("small N=256 chunks 2+2+1", 256, 5, {"gen_chunk": 2}, (), "small", 3),
    ("four-step N=8192 chunks 2+2+1", 8192, 5, {"gen_chunk": 2}, (), "four", 3),
]


@pytest.mark.parametrize("what", ["bounds", "bands"])
@pytest.mark.parametrize("case", OWN, ids=[c[0] for c in OWN])
def test_per_window_bounds_and_bands_reach_their_own_window(xc, opts, case, what):
    """Windows whose true lags differ, a narrow interval per window around its own (disjoint between windows): under the
    one-launch path the pair kernels see the virtual window hypothesis x W + window and must read the bounds of the real
    one; across chunk seams a chunk must read its own rows.  The same with one band per window."""
    _, N, W, defaults, eng_opts, kind, chunks = case
    name = "differing%d/%s" % (N, what)
    iq, raw, grid, pairs, kw = rr.case(name)
    ref = rr.case_reference(name)
    assert iq.shape == (W, 3, N)
    if what == "bounds":
        lb = kw["lag_bounds"]
        assert lb.shape == (W, 3, 2)
        for w in range(1, W):   # disjoint between consecutive windows, pair by pair: a neighbour's interval cannot hold this lag
            assert np.all((lb[w, :, 0] > lb[w - 1, :, 1]) | (lb[w, :, 1] < lb[w - 1, :, 0]))
    else:
        assert len({tuple(r) for r in kw["band"].tolist()}) == W
    with _engine(xc, 3, N, W, eng_opts) as whole:
        for k, v in defaults.items():
            opts(k, v)
        with _engine(xc, 3, N, W, eng_opts) as cut:
            for x in (iq, raw):
                got = cut.caf(x, grid, fine=True, **kw)
                assert _launches(cut) == _expected(kind, len(grid), chunks, "g_rows_inv"), _launches(cut)
                one = whole.caf(x, grid, fine=True, **kw)
                assert _launches(whole) == _expected(kind, len(grid), 1, "g_rows_inv"), _launches(whole)
                _assert_same(got, one, "chunked against one chunk")
                _assert_request_parity(got, ref)
                if what == "bounds":
                    assert np.all((got[2] >= lb[..., 0]) & (got[2] <= lb[..., 1]))


# ---- 3. rotation, weighting and selection, bit for bit ----------------------------------------------------------------------
# (id, N, W, engine options, families of the weighted correlate(), kind of the search with D = 3, its chunks)
EXACT = [
    ("N=256", 256, 3, (), {"g_fwd_small", "g_pair_small"}, "small", 1),
    ("N=8192", 8192, 2, (), {"g_cols_fwd", "g_rows_fwd", "g_rows_inv", "g_cols_inv", "g_final"}, "four", 1),
    ("N=4096 one launch", 4096, 3, (), {"k_fwd", "k_win|k_pair"}, "one", 1),
    ("N=4096 chunked", 4096, 12, (("chunk_windows", 8),), {"k_fwd", "k_win|k_pair"}, "per", 2),
]


def _exact_requests(N, P):
    lb = np.array([[-(N // 2), N // 3]] * P, np.int32)
    return [("phat", dict(whiten=True)), ("band + bounds", dict(band=np.array([-0.28, 0.31]), lag_bounds=lb))]


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_rotation_weighting_and_selection_bit_for_bit(xc, case, D):
    """caf(request) IS the d-major first maximum over correlate(host-rotated windows, the same request) -- a weighted
    correlate() runs the per-transform kernels the search runs --, and dop_frac IS the double-precision parabola, cast to
    float32, through the float32 peaks of D single-hypothesis caf(iq, [grid[d]], request) calls on the same engine."""
    _, N, W, eng_opts, corr_families, kind, chunks = case
    iq, raw, grid, _ = cr.scene(W, 4, N, 3, seed=300 + N + W)
    if D == 1:
        grid = grid[2:]
        kind = {"one": "per"}.get(kind, kind)
    pairs = cr.CROSS_PAIRS
    with _engine(xc, 4, N, W, eng_opts) as eng:
        for rid, kw in _exact_requests(N, len(pairs)):
            per_d = []
            for nu in grid:
                x = iq.copy()
                x[:, 2:] = cr.rot_mul(iq[:, 2:], cr.libm_phasor(nu, N))
                per_d.append(eng.correlate(x, pairs, **kw))
                assert set(_launches(eng)) == corr_families, _launches(eng)
            li, lf, pk = (np.stack([r[k] for r in per_d], axis=-1) for k in range(3))
            dop = cr.first_max(pk)
            want = (dop, cr.take(li, dop), cr.take(lf, dop), cr.take(pk, dop))
            singles = np.stack([eng.caf(iq, [nu], pairs, **kw)[3] for nu in grid], axis=-1)
            assert singles.dtype == np.float32
            want_frac = rr.dop_parabola(singles, dop)
            if D == 3:
                assert np.any(dop == 1) and np.any(want_frac != 0)     # an interior winner: the parabola is exercised
            for x in (iq, raw):
                got = eng.caf(x, grid, pairs, fine=True, **kw)
                assert _launches(eng) == _expected(kind, D, chunks), _launches(eng)
                _assert_same(_four(got), want, rid + ": caf against correlate() of the host-rotated windows")
                assert np.array_equal(_bits(got[1]), _bits(want_frac)), rid + ": dop_frac against the parabola of the single-hypothesis peaks"


# ---- 4. identities ------------------------------------------------------------------------------------------------------------
SELECT = [
    ("N=256", "seam256", (), "small", 1),
    ("N=8192", "seam8192", (), "four", 1),
    ("N=4096 one launch", "one3", (), "one", 1),
    ("N=4096 chunked", "chunked", (("chunk_windows", 8),), "per", 3),
]


def _raw_request(xc, eng, x, grid, P, band=None, band_pw=0, weighting=0, lb=None, lb_pw=0, fine=False, flags=0, outs=None,
                 n_dop=None):
    """rmx_caf_batch_request through ctypes with host arrays; -> (rc, [dop, dfrac or None, lag_int, lag_frac, peak]).
    n_dop: n_dopplers where it is not the grid's length"""
    lib = xc.load_library()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    W = x.shape[0]
    gp = np.ascontiguousarray(grid, np.float64)
    if outs is None:
        outs = [np.full((W, P), -77, np.int32), np.full((W, P), -77, np.float32) if fine else None, np.full((W, P), -77, np.int32),
                np.full((W, P), -77, np.float32), np.full((W, P), -77, np.float32)]
    rc = lib.rmx_caf_batch_request(eng._ctx, vp(x), W, None, P, vp(gp), len(gp) if n_dop is None else n_dop, vp(band), band_pw,
                                   weighting, vp(lb), lb_pw, *map(vp, outs), flags | (xc.RMX_IN_U8 if x.dtype == np.uint8 else 0))
    return rc, outs


@pytest.mark.parametrize("case", SELECT, ids=[c[0] for c in SELECT])
def test_a_request_with_nothing_set_is_the_plain_call(xc, case):
    """NULL band, RMX_WEIGHT_NONE, NULL bounds, NULL dop_frac -- and the full band with full-interval bounds -- are
    rmx_caf_batch: the same launches per family, the same bits.  fine=True on the plain call adds dop_frac and changes
    nothing else."""
    _, name, eng_opts, kind, chunks = case
    W, B, N, D, seed = cr.SCENES[name]
    iq, raw, grid, _ = cr.scene(W, B, N, D, seed)
    P = B * (B - 1) // 2
    full_band = np.array([-0.5, 0.5])
    full_lb = np.array([[-(N - 1), N - 1]] * P, np.int32)
    with _engine(xc, B, N, W, eng_opts) as eng:
        for x in (iq, raw):
            plain = eng.caf(x, grid)
            want = _launches(eng)
            assert want == _expected(kind, D, chunks), want
            rc, o = _raw_request(xc, eng, x, grid, P)
            assert rc == 0 and _launches(eng) == want
            _assert_same([o[0]] + o[2:], plain, "nothing set")
            rc, o = _raw_request(xc, eng, x, grid, P, band=full_band, lb=full_lb)
            assert rc == 0 and _launches(eng) == want
            _assert_same([o[0]] + o[2:], plain, "full band, full bounds")
            for kw in ({}, dict(band=np.tile(full_band, (W, 1)), lag_bounds=np.tile(full_lb, (W, 1, 1)))):
                fine = eng.caf(x, grid, fine=True, **kw)
                assert _launches(eng) == want, _launches(eng)
                _assert_same(_four(fine), plain, "fine=True on the plain call")
                assert np.array_equal(_bits(fine[1]), _bits(rr.dop_parabola(_per_hypothesis_peaks(eng, x, grid), fine[0])))


def _per_hypothesis_peaks(eng, x, grid, **kw):
    return np.stack([eng.caf(x, [nu], **kw)[3] for nu in grid], axis=-1)


@pytest.mark.parametrize("case", SELECT, ids=[c[0] for c in SELECT])
def test_ties_between_hypotheses_under_bounds_keep_the_lowest_index(xc, case):
    """[a, b, a, b, a] repeats its peaks exactly: under bounds and PHAT, strict > answers as for [a, b] -- dop_idx 0 or 1,
    the four arrays bit for bit -- in both selection kernels with and without dop_frac.  All-zero windows: hypothesis 0,
    the interval's first lag, peak 0, dop_frac 0."""
    _, name, eng_opts, kind, chunks = case
    W, B, N, D, seed = cr.SCENES[name]
    iq, raw, grid, _ = cr.scene(W, B, N, D, seed)
    kw = dict(lag_bounds=np.array([[-(N - 2), N - 3]] * (B * (B - 1) // 2), np.int32), whiten=True)
    a, b = grid[len(grid) // 2 + 1], grid[len(grid) // 2]
    with _engine(xc, B, N, W, eng_opts) as eng:
        for x in (iq, raw):
            two = eng.caf(x, [a, b], **kw)
            assert set(two[0].ravel().tolist()) == {0, 1}
            for fine in (False, True):
                five = eng.caf(x, [a, b, a, b, a], fine=fine, **kw)
                assert _launches(eng) == _expected(kind, 5, chunks), _launches(eng)
                assert set(five[0].ravel().tolist()) <= {0, 1}
                _assert_same(_four(five) if fine else five, two, "[a, b, a, b, a] against [a, b]")
            # dop_idx 0: an edge, 0; dop_idx 1: its neighbours are both a < b, a symmetric parabola, 0
            assert not five[1].any()
        zero = np.zeros((W, B, N), np.complex64)
        dop, dfrac, li, lf, pk = eng.caf(zero, grid[:3], fine=True, **kw)
        assert _launches(eng) == _expected(kind, 3, chunks), _launches(eng)
        lo = np.broadcast_to(kw["lag_bounds"][..., 0], li.shape)
        assert not dop.any() and not dfrac.any() and np.array_equal(li, lo) and not lf.any() and not pk.any()


# ---- 5. the scene the request exists for ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [256, 4096])
def test_dc_offset_plain_is_wrong_and_phat_is_right(xc, N):
    iq, grid, lags, hyp = rr.dc_scene(N)
    with _engine(xc, 3, N, 1) as eng:
        plain = eng.caf(iq, grid, fine=True)
        assert np.all(plain[0] == len(grid) // 2) and not np.any(plain[2][0] == lags)      # nu = 0, a lag next to 0
        _assert_request_parity(plain, rr.case_reference("dc%d/plain" % N))
        phat = eng.caf(iq, grid, whiten=True, fine=True)
        assert np.array_equal(phat[0][0], hyp) and np.array_equal(phat[2][0], lags)
        _assert_request_parity(phat, rr.case_reference("dc%d/phat" % N))


# ---- 6. doors ---------------------------------------------------------------------------------------------------------------------
DOORS = [
    (4096, 3, 5, (), "one", 1),
    (4096, 8, 12, (("chunk_windows", 8),), "per", 2),
    (1024, 3, 5, (), "small", 1),
    (8192, 3, 2, (), "four", 1),
]
GUARD = 64


def _guarded(torch, dev, n):
    return [torch.full((n + GUARD,), -77, dtype=t, device=dev)
            for t in (torch.int32, torch.float32, torch.int32, torch.float32, torch.float32)]


@pytest.mark.parametrize("door", DOORS, ids=["N=%d B=%d W=%d" % d[:3] for d in DOORS])
def test_device_pointers_and_mixed_flags(xc, door):
    """The four combinations of RMX_IN_DEVICE and RMX_OUT_DEVICE -- neither (caf), both (caf_device), either alone (the raw
    ABI) -- give the same five arrays bit for bit, write exactly [W][P] elements of each, dop_frac included, and leave the
    guard tails behind them untouched."""
    import torch
    N, B, W, eng_opts, kind, chunks = door
    D = 3
    iq, raw, grid, _ = cr.scene(W, B, N, D, seed=500 + N + B + W)
    P = B * (B - 1) // 2
    n = W * P
    lb = np.array([[-(N // 2), N // 2]] * P, np.int32)
    band = np.array([-0.3, 0.26])
    dev = torch.device("cuda", 0)
    with _engine(xc, B, N, W, eng_opts) as eng:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        for u8 in (False, True):
            x = raw if u8 else iq
            host = eng.caf(x, grid, lag_bounds=lb, band=band, whiten=True, fine=True)
            assert _launches(eng) == _expected(kind, D, chunks), _launches(eng)
            assert len(set(host[0].ravel().tolist())) > 1 and host[1].any()
            x_d = torch.from_numpy(np.ascontiguousarray(x) if u8 else np.ascontiguousarray(x).view(np.float32).reshape(W, B, N, 2)).to(dev)
            o = _guarded(torch, dev, n)
            eng.caf_device(x_d.data_ptr(), W, grid, o[0].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), u8=u8,
                           lag_bounds=lb, band=band, whiten=True, dop_frac_ptr=o[1].data_ptr())
            eng.synchronize()
            assert _launches(eng) == _expected(kind, D, chunks), _launches(eng)
            out = [t.cpu().numpy() for t in o]
            _assert_same([a[:n].reshape(W, P) for a in out], host, "caf_device")
            assert all(np.all(a[n:] == -77) for a in out), "caf_device wrote past [W][P]"
            # without dop_frac_ptr the fifth buffer is not touched
            o = _guarded(torch, dev, n)
            eng.caf_device(x_d.data_ptr(), W, grid, o[0].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), u8=u8,
                           lag_bounds=lb, band=band, whiten=True)
            eng.synchronize()
            out = [t.cpu().numpy() for t in o]
            _assert_same([out[k][:n].reshape(W, P) for k in (0, 2, 3, 4)], _four(host), "caf_device without dop_frac")
            assert np.all(out[1] == -77)
            for flags in (xc.RMX_IN_DEVICE, xc.RMX_OUT_DEVICE):
                lib = xc.load_library()
                in_ptr = C.c_void_p(x_d.data_ptr()) if flags & xc.RMX_IN_DEVICE else x.ctypes.data_as(C.c_void_p)
                if flags & xc.RMX_OUT_DEVICE:
                    o = _guarded(torch, dev, n)
                    ptrs = [C.c_void_p(t.data_ptr()) for t in o]
                else:
                    o = [np.full(n + GUARD, -77, t) for t in (np.int32, np.float32, np.int32, np.float32, np.float32)]
                    ptrs = [a.ctypes.data_as(C.c_void_p) for a in o]
                gp = np.ascontiguousarray(grid, np.float64)
                rc = lib.rmx_caf_batch_request(eng._ctx, in_ptr, W, None, P, gp.ctypes.data_as(C.c_void_p), D,
                                               band.ctypes.data_as(C.c_void_p), 0, xc.RMX_WEIGHT_PHAT, lb.ctypes.data_as(C.c_void_p), 0,
                                               *ptrs, flags | (xc.RMX_IN_U8 if u8 else 0))
                assert rc == 0, (flags, lib.rmx_last_error(eng._ctx))
                assert lib.rmx_synchronize(eng._ctx) == 0
                out = [t.cpu().numpy() if flags & xc.RMX_OUT_DEVICE else t for t in o]
                _assert_same([a[:n].reshape(W, P) for a in out], host, "flags = %d" % flags)
                assert all(np.all(a[n:] == -77) for a in out), "flags = %d wrote past [W][P]" % flags


@pytest.mark.parametrize("u8", [False, True], ids=["complex64", "uint8"])
@pytest.mark.parametrize("N", [4096, 1024])
def test_state_between_calls(xc, N, u8):
    """One engine through plain -> PHAT -> bounded -> plain, then growing and shrinking W and D with every option on (N = 4096:
    the per-hypothesis path after the one-launch path): each answer is, bit for bit, a fresh engine's -- no stale band or
    bounds, no undersized neighbour scratch of k_caf_select_fd."""
    B, WMAX = 3, 16
    iq, raw, grid9, _ = cr.scene(WMAX, B, N, 9, seed=600 + N)
    x = raw if u8 else iq
    lb = np.array([[-(N // 4), N // 4]] * 3, np.int32)
    lb_w = np.tile(lb, (WMAX, 1, 1)) + np.arange(WMAX, dtype=np.int32)[:, None, None]
    every = dict(whiten=True, band=np.array([-0.3, 0.28]), fine=True)
    g5 = grid9[2:7]
    calls = [("plain", g5, 2, {}), ("PHAT", g5, 2, dict(whiten=True)), ("bounded", g5, 2, dict(lag_bounds=lb)), ("plain again", g5, 2, {}),
             ("fine", g5, 2, dict(fine=True)), ("more windows, more hypotheses", grid9, WMAX, dict(lag_bounds=lb_w, **every)),
             ("fewer", grid9[3:6], 2, dict(lag_bounds=lb_w[:2], **every)), ("one hypothesis", grid9[5:6], 3, dict(lag_bounds=lb, **every)),
             ("more again", grid9, WMAX, dict(lag_bounds=lb, **every)), ("per-window bands", g5, 4, dict(band=rr.window_bands(4), fine=True)),
             ("plain at the end", g5, 2, {})]
    kinds = {4096: {True: "one", False: "per"}, 1024: {True: "small", False: "small"}}[N]
    eng_opts = (("chunk_windows", 8),) if N == 4096 else ()

    def run(eng, grid, w, kw):
        out = eng.caf(x[:w], grid, **kw)
        one = w <= 8 and len(grid) > 1
        assert _launches(eng) == _expected(kinds[one], len(grid), 1 if (one or N != 4096) else (w + 7) // 8), _launches(eng)
        return out

    with _engine(xc, B, N, WMAX, eng_opts) as eng:
        for what, grid, w, kw in calls:
            got = run(eng, grid, w, kw)
            with _engine(xc, B, N, WMAX, eng_opts) as fresh:
                want = run(fresh, grid, w, kw)
            _assert_same(got, want, what)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [256, 4096])
def test_refusals_leave_the_outputs_and_the_engine_alone(xc, N):
    """RMX_E_INVAL with a text that names the argument, in the order rmx_caf_batch's checks, the weighted entry's, the bounded
    entry's, dop_frac's; the five output arrays as they were; the next valid call answered as before."""
    B, W, P = 3, 2, 3
    iq, _, grid, _ = cr.scene(W, B, N, 3, seed=700 + N)
    ok_lb = np.array([[-5, 5]] * P, np.int32)
    bad_lb = ok_lb.copy()
    bad_lb[1] = (4, 3)
    far_lb = ok_lb.copy()
    far_lb[2, 1] = N
    few_lb = np.tile(ok_lb, (W, 1, 1))
    few_lb[1, 0] = (-N, 0)
    ok_band, bad_band, thin_band = np.array([-0.2, 0.3]), np.array([0.3, -0.2]), np.array([0.1 / N, 0.2 / N])
    nan_band = np.array([[-0.2, 0.3], [np.nan, 0.3]])
    kw0 = dict(whiten=True, lag_bounds=ok_lb, band=ok_band, fine=True)
    # (arguments of _raw_request, a word of the message)
    refused = [
        (dict(n_dop=0), b"n_dopplers"),
        (dict(n_dop=4097, weighting=7, lb=bad_lb), b"n_dopplers"),                  # rmx_caf_batch's checks come first
        (dict(weighting=7), b"weighting"),
        (dict(weighting=7, band=bad_band, lb=bad_lb), b"weighting"),                # then the weighting,
        (dict(band=bad_band, lb=bad_lb), b"band"),                                  # then the band,
        (dict(band=thin_band), b"keeps no bin"),
        (dict(band=nan_band, band_pw=1), b"band of window 1"),
        (dict(lb=bad_lb, weighting=1), b"lag_bounds"),                              # then the bounds
        (dict(lb=far_lb), b"lag_bounds"),
        (dict(lb=few_lb, lb_pw=1, band=ok_band), b"lag_bounds of window 1, pair 0"),
    ]
    with _engine(xc, B, N, W) as eng:
        before = eng.caf(iq, grid, **kw0)
        plain = eng.caf(iq, grid)
        for args, word in refused:
            rc, o = _raw_request(xc, eng, iq, grid, P, fine=True, **args)
            assert rc == -1, (args, rc)                      # RMX_E_INVAL
            msg = xc.load_library().rmx_last_error(eng._ctx)
            assert word in msg, (args, msg)
            assert all(np.all(a == -77) for a in o), args
            _assert_same(eng.caf(iq, grid, **kw0), before, "the request after a refusal")
        # dop_frac over another output: refused after everything else, whichever array it lies over
        for k, name in ((0, b"dop_idx"), (2, b"lag_int"), (3, b"lag_frac"), (4, b"peak")):
            outs = [np.full((W, P), -77, np.int32), None, np.full((W, P), -77, np.int32), np.full((W, P), -77, np.float32),
                    np.full((W, P), -77, np.float32)]
            outs[1] = outs[k].view(np.float32)
            rc, o = _raw_request(xc, eng, iq, grid, P, weighting=1, lb=ok_lb, outs=outs)
            msg = xc.load_library().rmx_last_error(eng._ctx)
            assert rc == -1 and b"dop_frac overlaps " + name in msg, (k, rc, msg)
            assert all(np.all(o[m] == -77) for m in (0, 2, 3, 4)), k
            rc, _ = _raw_request(xc, eng, iq, grid, P, weighting=7, outs=outs)
            assert rc == -1 and b"weighting" in xc.load_library().rmx_last_error(eng._ctx)
        _assert_same(eng.caf(iq, grid, **kw0), before, "the request after the refusals")
        _assert_same(eng.caf(iq, grid), plain, "the plain call after the refusals")
        # through the binding: RmxError with the library's text
        with pytest.raises(xc.RmxError) as e:
            eng.caf(iq, grid, lag_bounds=far_lb)
        assert e.value.code == -1 and "lag_bounds" in str(e.value)
        with pytest.raises(xc.RmxError) as e:
            eng.caf(iq, grid, band=thin_band, fine=True)
        assert e.value.code == -1 and "keeps no bin" in str(e.value)



# ---- 8. the seam end to end ----------------------------------------------------------------------------------------------------------
def test_seam_doppler_search_measures_lags_and_offsets_under_a_dc_offset(xc):
    """TDoACalculator(doppler_search_hz=...) on the DC-offset scene through both doors, the calculator's own pair loop and the
    processor's batch: with whiten the measurements carry the true lags and the emitter's frequency offsets (buoy2's copy
    against buoy1's, within a tenth of a grid step of the on-grid truth); without it every pair reports 0 Hz and a lag next
    to 0.  The default calculator's measurements carry no offset."""
    from radio_mapper_amd import tdoa_processor as tp
    N, fs = 256, 2.56e6
    iq, grid, lags, hyp = rr.dc_scene(N)
    step_hz = 0.5 / N * fs                      # 5 kHz: the scene's grid spacing
    want_hz = (hyp - len(grid) // 2) * step_hz
    buoys = [("B0", 37.0, -122.0), ("B1", 37.3, -122.0), ("B2", 37.0, -121.6)]
    pos = {bid: tp.BuoyPosition(bid, la, lo, 0.0, timing_accuracy_ns=20) for bid, la, lo in buoys}
    t0 = 1_700_000_000_000_000_000
    dets = [tp.SignalDetection(bid, 121.5, -60.0, "t", t0, la, lo, 0.9, iq_samples=iq[0, b], sample_rate_hz=fs)
            for b, (bid, la, lo) in enumerate(buoys)]

    def lag_of(m):
        return m.time_difference_ns * 1e-9 * fs

    calc = tp.TDoACalculator(doppler_search_hz=(2 * step_hz, step_hz), whiten=True)
    try:
        assert np.allclose(calc.doppler_grid(fs), grid, rtol=0, atol=1e-15)
        meas = calc.calculate_tdoa_measurements(dets, pos)
        assert [(m.buoy1_id, m.buoy2_id) for m in meas] == [("B0", "B1"), ("B0", "B2"), ("B1", "B2")]
        assert np.all(np.abs(np.array([lag_of(m) for m in meas]) - lags) < 0.5)
        got_hz = np.array([m.frequency_offset_hz for m in meas])
        print("frequency offsets", got_hz, "want", want_hz)
        inner = np.abs(hyp - len(grid) // 2) < len(grid) // 2            # (an edge hypothesis has no parabola: exact)
        assert np.all(np.abs(got_hz - want_hz) <= np.where(inner, 0.1 * step_hz, 0.0))
    finally:
        calc.close()
    p = tp.TDoAProcessor(doppler_search_hz=(2 * step_hz, step_hz), whiten=True)
    try:
        for b in pos.values():
            p.register_buoy(b)
        seen = []
        p.hyperbolic_positioner.triangulate_position = lambda m, _pos: seen.extend(m)
        p.process_signal_detections(dets)
        assert len(seen) == 3 and [m.time_difference_ns for m in seen] == [m.time_difference_ns for m in meas]
        assert [m.frequency_offset_hz for m in seen] == [m.frequency_offset_hz for m in meas]
    finally:
        p.tdoa_calculator.close()
    plain = tp.TDoACalculator(doppler_search_hz=(2 * step_hz, step_hz))
    try:
        meas = plain.calculate_tdoa_measurements(dets, pos)
        assert all(abs(m.frequency_offset_hz) < 0.5 * step_hz for m in meas) and all(abs(lag_of(m)) < 4 for m in meas)
    finally:
        plain.close()
    off = tp.TDoACalculator(whiten=True)
    try:
        assert all(m.frequency_offset_hz is None for m in off.calculate_tdoa_measurements(dets, pos))
    finally:
        off.close()
