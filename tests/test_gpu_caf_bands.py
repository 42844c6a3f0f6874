"""rmx_caf_batch_bands, the Doppler search under several bands per window over one set of forward passes, on the GPU: every
route bit for bit against M single-band caf(band=...) calls and against the float32 restatement (tests/caf_bands_ref.py),
the identity with one band, per-window bands and bounds under the one-launch path's virtual windows and across chunk
seams, one-bin bands, the two-emitter scene, the pointer flags and guarded outputs, the refusals, the state an engine
keeps between calls, and the seam with share_doppler.

The scenes hold one emitter per band with its own delays and frequency offsets (caf_bands_ref.scene): the winners differ
between the bands of a window, so a kernel that read another band's or another hypothesis' operand fails.  Parity with the
reference is the rule of tests/test_gpu_caf_request.py with no slot excused: tests/test_caf_bands_cpu.py holds every
case's lag margin and hypothesis margin above 1e-5 on the reference alone."""
import ctypes as C

import numpy as np
import pytest

import caf_bands_ref as br
import caf_ref as cr
import caf_request_ref as rr
import weighted_ref as wr
from test_gpu_caf import _engine, _expected, _launches

pytestmark = pytest.mark.gpu
NAMES = ("dop_idx", "dop_frac", "lag_int", "lag_frac", "peak")
TOL = 1e-5


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
        assert u.dtype == v.dtype and u.shape == v.shape, (what, name, u.shape, v.shape)
        assert np.array_equal(_bits(u), _bits(v)), "%s %s: %d of %d elements differ" % (what, name, int((_bits(u) != _bits(v)).sum()), u.size)


def _four(fine_out):
    return (fine_out[0],) + tuple(fine_out[2:])


def _band(bands, m):
    """band m of a set: [2] of a shared set, [W][2] of a per-window one"""
    return np.ascontiguousarray(np.asarray(bands)[..., m, :])


def _assert_is_the_single_band_calls(eng, x, grid, pairs, bands, kw, got, what, want_launches=None):
    """[:, m] of a fine=True caf_bands result IS caf(band=bands[..., m, :], fine=True), bit for bit"""
    for m in range(np.asarray(bands).shape[-2]):
        single = eng.caf(x, grid, pairs, band=_band(bands, m), fine=True, **kw)
        if want_launches is not None:
            assert _launches(eng) == want_launches, (what, m, _launches(eng))
        _assert_same([a[:, m] for a in got], single, "%s: band %d against caf(band=...)" % (what, m))


def _assert_parity(fine_out, ref):
    """every slot against the restatement: the winner and the integer lag exact (no slot excused), the lag within 1e-5 or
    the flat-peak bound, the peak within 1e-5, dop_frac within 1e-5 or its three-tap one-ulp bound"""
    dop, dfrac, li, lf, pk = fine_out
    assert (dop.dtype, dfrac.dtype, li.dtype, lf.dtype, pk.dtype) == (np.int32, np.float32, np.int32, np.float32, np.float32)
    assert float(ref["hyp_margin"].min()) > br.LAG_MARGIN_BAR and float(ref["lag_margin"].min()) > br.LAG_MARGIN_BAR
    assert dop.shape == ref["dop"].shape
    assert np.array_equal(dop, ref["dop"]), "%d winning hypotheses differ" % int((dop != ref["dop"]).sum())
    assert np.array_equal(li, ref["lag_int"]), "%d integer lags differ (none is excused)" % int((li != ref["lag_int"]).sum())
    want, have = ref["lag_int"] + ref["lag_frac"], li + lf.astype(np.float64)
    rel = np.abs(have - want) / np.maximum(np.abs(want), 1.0)
    print("worst lag %.3e, worst peak %.3e" % (rel.max(), (np.abs(pk - ref["peak"]) / ref["peak"]).max()))
    assert np.all((rel <= TOL) | (rel <= 4.0 * ref["flat_bound"])), "fractional lag outside the rule: %.3e" % rel.max()
    assert np.allclose(pk, ref["peak"], rtol=1e-5, atol=0)
    err = np.abs(dfrac.astype(np.float64) - ref["dop_frac"].astype(np.float64))
    assert np.all((err <= 1e-5) | (err <= ref["dop_frac_bound"])), "dop_frac outside the rule: %.3e" % err.max()
    D = ref["bin_peak"].shape[-1]
    assert np.all(dfrac > -0.5) and np.all(dfrac <= 0.5) and not np.any(dfrac[(dop == 0) | (dop == D - 1)])


# ---- 1. every route ---------------------------------------------------------------------------------------------------------------
# (id, scene, kind, chunks, default options, engine options)
ROUTES = [
    ("small N=16", "n16", "small", 1, {}, ()),
    ("small N=256", "n256", "small", 1, {}, ()),
    ("small N=4096 generic4096", "g4096", "small", 1, {"generic4096": 1}, ()),
    ("four-step N=8192", "n8192", "four", 1, {}, ()),
    ("four-step N=8192 6 buoys", "n8192b6", "four", 1, {}, ()),
    ("one launch DW=40 resident=1", "one8", "one", 1, {}, (("resident", 1),)),
    ("one launch DW=40 resident=0", "one8", "one", 1, {}, (("resident", 0),)),
    ("one launch DW=21 resident=1", "one3", "one", 1, {}, (("resident", 1),)),
    ("one launch DW=21 resident=0", "one3", "one", 1, {}, (("resident", 0),)),
    ("per hypothesis chunks 8+8+4 resident=1", "chunked", "per", 3, {}, (("chunk_windows", 8), ("resident", 1))),
    ("per hypothesis chunks 8+8+4 resident=0", "chunked", "per", 3, {}, (("chunk_windows", 8), ("resident", 0))),
    ("small N=256 chunks 2+2+1", "seam256", "small", 3, {"gen_chunk": 2}, ()),
    ("four-step N=8192 chunks 2+2+1", "seam8192", "four", 3, {"gen_chunk": 2}, ()),
]


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_against_the_single_band_calls_and_the_reference(xc, opts, route):
    """M in {2, 3} x {shared, per-window bands} x {none, PHAT} x {no bounds, per-window bounds} x {default, custom pair list}:
    the launch counts of ONE single-band search over the same chunks, fine=True's other four arrays bit-identical to
    fine=False, uint8 bit-identical to complex64, every band bit for bit the single-band call, and the reference's cases
    against the reference.  Six buoys with the default list on the four-step route: the single-band call takes g_rows_anchor
    there, so those 16 combinations are held to the reference's bars instead, one by one, in the test below."""
    _, name, kind, chunks, defaults, eng_opts = route
    for k, v in defaults.items():
        opts(k, v)
    W, B, N, D, _ = cr.SCENES[name]
    want = _expected(kind, D, chunks, "g_rows_inv")
    with _engine(xc, B, N, W, eng_opts) as eng:
        for custom in (False, True):
            anchor = kind == "four" and B >= 6 and not custom
            single_want = _expected(kind, D, chunks, "g_rows_anchor" if anchor else "g_rows_inv")
            for M in (2, 3):
                for form in ("shared", "perwin"):
                    for rid in br.REQUEST_IDS:
                        case = "%s/%s/%d/%s/%s" % (name, "custom" if custom else "default", M, form, rid)
                        iq, raw, grid, pairs, bands, kw = br.case(case)
                        fine = eng.caf_bands(iq, grid, bands, pairs, fine=True, **kw)
                        assert _launches(eng) == want, (case, _launches(eng))
                        assert all(a.shape == (W, M, len(rr.pair_array(pairs, B))) for a in fine), case
                        got = eng.caf_bands(iq, grid, bands, pairs, **kw)
                        assert _launches(eng) == want, (case, _launches(eng))
                        _assert_same(_four(fine), got, case + ": fine=True against fine=False")
                        fine8 = eng.caf_bands(raw, grid, bands, pairs, fine=True, **kw)
                        assert _launches(eng) == want, (case, "uint8", _launches(eng))
                        _assert_same(fine8, fine, case + ": uint8 against complex64")
                        if not anchor:
                            _assert_is_the_single_band_calls(eng, iq, grid, pairs, bands, kw, fine, case, single_want)
                        if case in br.REFERENCE_CASES and not anchor:
                            print(case)
                            ref = br.case_reference(case)
                            _assert_parity(fine, ref)
                            assert np.any(ref["dop"] != ref["dop"][:, :1]) and np.any(ref["lag_int"] != ref["lag_int"][:, :1])


@pytest.mark.parametrize("case", br.ANCHOR_CASES)
def test_six_buoys_with_the_default_list_are_held_to_the_reference(xc, case):
    """The documented exception: on the four-step route with the default pair list from 6 buoys on the single-band call's
    inverse rows are g_rows_anchor's, which the banded call never takes, so the two need not agree in bits.  Every one of
    the 16 combinations of M, shared / per-window bands and the request is held to the reference's bars, complex64 and
    uint8, no slot excused."""
    W, B, N, D, _ = cr.SCENES["n8192b6"]
    iq, raw, grid, pairs, bands, kw = br.case(case)
    assert pairs is None and B == 6
    ref = br.case_reference(case)
    with _engine(xc, B, N, W) as eng:
        for x in (iq, raw):
            fine = eng.caf_bands(x, grid, bands, fine=True, **kw)
            assert _launches(eng) == _expected("four", D, 1, "g_rows_inv"), _launches(eng)
            _assert_parity(fine, ref)
        eng.caf(iq, grid, band=_band(bands, 0), **kw)
        assert _launches(eng) == _expected("four", D, 1, "g_rows_anchor"), _launches(eng)      # why the bits may differ
    assert np.any(ref["dop"] != ref["dop"][:, :1]) and np.any(ref["lag_int"] != ref["lag_int"][:, :1])


# ---- 2. one band IS the single-band search -----------------------------------------------------------------------------------------
ONE_BAND = [
    ("small N=256", "seam256", "small", 1, ()),
    ("four-step N=8192", "seam8192", "four", 1, ()),
    ("one launch", "one3", "one", 1, ()),
    ("per hypothesis", "chunked", "per", 3, (("chunk_windows", 8),)),
]


@pytest.mark.parametrize("case", ONE_BAND, ids=[c[0] for c in ONE_BAND])
def test_one_band_is_the_single_band_search(xc, case):
    """caf_bands with one band, shared or per window, with and without PHAT and bounds: the launches, family by family, and
    the bits of caf(band=...)"""
    _, name, kind, chunks, eng_opts = case
    W, B, N, D, _ = cr.SCENES[name]
    iq, raw, grid, lags, _ = br.scene_of(name)
    lb = br.bounds_holding(lags, N)
    with _engine(xc, B, N, W, eng_opts) as eng:
        for bands in (br.band_set(1), br.band_set(1, W)):
            for kw in ({}, dict(whiten=True, lag_bounds=lb)):
                for x in (iq, raw):
                    single = eng.caf(x, grid, band=_band(bands, 0), fine=True, **kw)
                    want = _launches(eng)
                    assert want == _expected(kind, D, chunks, "g_rows_inv"), want
                    got = eng.caf_bands(x, grid, bands, fine=True, **kw)
                    assert _launches(eng) == want, _launches(eng)
                    assert all(a.shape == (W, 1, B * (B - 1) // 2) for a in got)
                    _assert_same([a[:, 0] for a in got], single, "one band")


# ---- 3. per-window bands and bounds reach their own (window, band) under every hypothesis --------------------------------------------
# (id, N, W, default options of the cut engine, engine options, kind, chunks)
OWN = [
    ("one launch resident=1", 4096, 3, {}, (("resident", 1),), "one", 1),
    ("one launch resident=0", 4096, 3, {}, (("resident", 0),), "one", 1),
    ("small N=256 chunks 2+2+1", 256, 5, {"gen_chunk": 2}, (), "small", 3),
    ("four-step N=8192 chunks 2+2+1", 8192, 5, {"gen_chunk": 2}, (), "four", 3),
]


@pytest.mark.parametrize("case", OWN, ids=[c[0] for c in OWN])
def test_per_window_bands_and_bounds_reach_their_own_window_and_band(xc, opts, case):
    """Windows whose true lags differ, a narrow interval per window around its own (disjoint between windows), and three
    bands per window with column m different in every window: under the one-launch path the pair kernels see the virtual
    window (hypothesis x W + window) x M + band and must read the band and the bounds of the real (window, band) and operand
    j of the right hypothesis; across chunk seams a chunk must read its own rows.  Then one-bin bands: every peak is the
    single-band call's bit for bit, which pins the bin map and the wrap together."""
    _, N, W, defaults, eng_opts, kind, chunks = case
    M = 3
    iq, raw, grid, bands, lb = br.differing_case(N, W, M)
    for w in range(1, W):
        assert np.all((lb[w, :, 0] > lb[w - 1, :, 1]) | (lb[w, :, 1] < lb[w - 1, :, 0]))
    for m in range(M):
        assert len({tuple(r) for r in bands[:, m].tolist()}) == W
    ref = br._cached(("differing ref", N, W), lambda: (br.reference(iq, grid, bands, None, True, lb),))[0]
    with _engine(xc, 3, N, W, eng_opts) as whole:
        for k, v in defaults.items():
            opts(k, v)
        with _engine(xc, 3, N, W, eng_opts) as cut:
            for x in (iq, raw):
                got = cut.caf_bands(x, grid, bands, lag_bounds=lb, whiten=True, fine=True)
                assert _launches(cut) == _expected(kind, len(grid), chunks, "g_rows_inv"), _launches(cut)
                one = whole.caf_bands(x, grid, bands, lag_bounds=lb, whiten=True, fine=True)
                assert _launches(whole) == _expected(kind, len(grid), 1, "g_rows_inv"), _launches(whole)
                _assert_same(got, one, "chunked against one chunk")
                _assert_is_the_single_band_calls(cut, x, grid, None, bands, dict(lag_bounds=lb, whiten=True), got, "own window")
                _assert_parity(got, ref)
                assert np.all((got[2] >= lb[:, None, :, 0]) & (got[2] <= lb[:, None, :, 1]))
            thin = br.one_bin_bands(N, W, M)
            for kw in ({}, dict(lag_bounds=lb)):
                got = cut.caf_bands(iq, grid, thin, fine=True, **kw)
                assert np.all(got[4] > 0)
                _assert_is_the_single_band_calls(cut, iq, grid, None, thin, kw, got, "one-bin bands")


# ---- 4. the scene the entry exists for --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 2), (4096, 1)], ids=["N=256 W=2", "N=4096 W=1"])
@pytest.mark.parametrize("whiten", [False, True], ids=["none", "phat"])
def test_two_emitters_come_back_from_one_call(xc, shape, whiten):
    """Two emitters in disjoint bands with their own delays and frequency offsets: one call under both bands returns both
    emitters' true lags and hypotheses; the un-banded search returns the strong one's only."""
    N, W = shape
    iq, grid, la, ha, lw, hb = rr.two_emitter_scene(N, W=W)
    bands = np.array([wr.STRONG_BAND, wr.WEAK_BAND])
    with _engine(xc, 3, N, W) as eng:
        dop, dfrac, li, lf, pk = eng.caf_bands(iq, grid, bands, whiten=whiten, fine=True)
        assert _launches(eng) == _expected("one" if N == 4096 else "small", len(grid)), _launches(eng)
        assert np.array_equal(dop[:, 0], np.broadcast_to(ha, (W, 3))) and np.array_equal(li[:, 0], la)
        assert np.array_equal(dop[:, 1], np.broadcast_to(hb, (W, 3))) and np.array_equal(li[:, 1], lw)
        assert not np.array_equal(ha, hb) and not np.array_equal(la, lw)
        _assert_parity((dop, dfrac, li, lf, pk), br.reference(iq, grid, bands, None, whiten, None))
        plain = eng.caf(iq, grid)
        assert np.array_equal(plain[0], np.broadcast_to(ha, (W, 3))) and np.array_equal(plain[1], la)


# ---- 5. pointers ------------------------------------------------------------------------------------------------------------------------
DOORS = [
    (4096, 3, 5, (), "one", 1),
    (4096, 4, 12, (("chunk_windows", 8),), "per", 2),
    (256, 3, 5, (), "small", 1),
    (8192, 3, 2, (), "four", 1),
]
GUARD = 64


def _guarded(torch, dev, n):
    return [torch.full((n + 2 * GUARD,), -77, dtype=t, device=dev)
            for t in (torch.int32, torch.float32, torch.int32, torch.float32, torch.float32)]


@pytest.mark.parametrize("door", DOORS, ids=["N=%d B=%d W=%d" % d[:3] for d in DOORS])
def test_device_pointers_guarded_outputs_and_a_stream(xc, door):
    """The four combinations of RMX_IN_DEVICE and RMX_OUT_DEVICE give the same five arrays bit for bit and write exactly
    W * M * P elements of each inside guarded slabs; the caller's band, bounds, grid and pair arrays are overwritten right
    after an asynchronous call returns; the call runs on a non-default stream."""
    import torch
    N, B, W, eng_opts, kind, chunks = door
    M, D = 3, 3
    iq, raw, grid, lags, _ = br.scene(W, B, N, D, seed=5100 + N + B + W)
    P = B * (B - 1) // 2
    n = W * M * P
    bands = br.band_set(M, W)
    lb = br.bounds_holding(lags, N)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with _engine(xc, B, N, W, eng_opts) as eng, torch.cuda.stream(stream):
        eng.set_stream(stream.cuda_stream)
        for u8 in (False, True):
            x = raw if u8 else iq
            host = eng.caf_bands(x, grid, bands, lag_bounds=lb, whiten=True, fine=True)
            assert _launches(eng) == _expected(kind, D, chunks, "g_rows_inv"), _launches(eng)
            assert len(set(host[0].ravel().tolist())) > 1
            x_d = torch.from_numpy(np.ascontiguousarray(x) if u8 else np.ascontiguousarray(x).view(np.float32).reshape(W, B, N, 2)).to(dev)
            stream.synchronize()
            for with_frac in (True, False):
                o = _guarded(torch, dev, n)
                stream.synchronize()
                ptr = [t.data_ptr() + GUARD * 4 for t in o]
                b2, l2, g2 = bands.copy(), lb.copy(), np.array(grid, np.float64)
                eng.caf_bands_device(x_d.data_ptr(), W, g2, b2, ptr[0], ptr[2], ptr[3], ptr[4], u8=u8, lag_bounds=l2, whiten=True,
                                     dop_frac_ptr=ptr[1] if with_frac else 0)
                b2[:] = 0.4999
                l2[:] = 0
                g2[:] = 0.25
                eng.synchronize()
                out = [t.cpu().numpy() for t in o]
                if with_frac:
                    _assert_same([a[GUARD:GUARD + n].reshape(W, M, P) for a in out], host, "caf_bands_device")
                else:
                    _assert_same([out[k][GUARD:GUARD + n].reshape(W, M, P) for k in (0, 2, 3, 4)], _four(host), "without dop_frac")
                    assert np.all(out[1] == -77)
                assert all(np.all(a[:GUARD] == -77) and np.all(a[GUARD + n:] == -77) for a in out), "wrote outside [W][M][P]"
            lib = xc.load_library()
            for flags in (xc.RMX_IN_DEVICE, xc.RMX_OUT_DEVICE):
                in_ptr = C.c_void_p(x_d.data_ptr()) if flags & xc.RMX_IN_DEVICE else x.ctypes.data_as(C.c_void_p)
                if flags & xc.RMX_OUT_DEVICE:
                    o = _guarded(torch, dev, n)
                    stream.synchronize()
                    ptrs = [C.c_void_p(t.data_ptr() + GUARD * 4) for t in o]
                else:
                    o = [np.full(n + 2 * GUARD, -77, t) for t in (np.int32, np.float32, np.int32, np.float32, np.float32)]
                    ptrs = [C.c_void_p(a.ctypes.data + GUARD * 4) for a in o]
                gp = np.ascontiguousarray(grid, np.float64)
                rc = lib.rmx_caf_batch_bands(eng._ctx, in_ptr, W, None, P, gp.ctypes.data_as(C.c_void_p), D,
                                             bands.ctypes.data_as(C.c_void_p), M, 1, xc.RMX_WEIGHT_PHAT, lb.ctypes.data_as(C.c_void_p), 1,
                                             *ptrs, flags | (xc.RMX_IN_U8 if u8 else 0))
                assert rc == 0, (flags, lib.rmx_last_error(eng._ctx))
                assert lib.rmx_synchronize(eng._ctx) == 0
                out = [t.cpu().numpy() if flags & xc.RMX_OUT_DEVICE else t for t in o]
                _assert_same([a[GUARD:GUARD + n].reshape(W, M, P) for a in out], host, "flags = %d" % flags)
                assert all(np.all(a[:GUARD] == -77) and np.all(a[GUARD + n:] == -77) for a in out), "flags = %d wrote outside" % flags


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def _raw_call(xc, eng, x, grid, P, bands, n_bands=None, bands_pw=0, weighting=0, lb=None, lb_pw=0, outs=None, n_dop=None, fine=True,
              pairs=None, n_win=None):
    """rmx_caf_batch_bands through ctypes with host arrays and poisoned outputs -> (rc, outputs, the text).  n_win, P and
    pairs: the batch shape as passed, whatever the arrays hold (a refused call reads none of them)"""
    lib = xc.load_library()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    W = x.shape[0]
    M = (np.asarray(bands).shape[-2] if bands is not None else 1) if n_bands is None else n_bands
    gp = np.ascontiguousarray(grid, np.float64)
    if outs is None:
        shape = (W, max(M, 1) if M <= 64 else 1, max(P, 1))
        outs = [np.full(shape, -77, np.int32), np.full(shape, -77, np.float32) if fine else None, np.full(shape, -77, np.int32),
                np.full(shape, -77, np.float32), np.full(shape, -77, np.float32)]
    rc = lib.rmx_caf_batch_bands(eng._ctx, vp(x), W if n_win is None else n_win, vp(pairs), P, vp(gp), len(gp) if n_dop is None else n_dop,
                                 vp(bands), M, bands_pw, weighting, vp(lb), lb_pw, *map(vp, outs), 0)
    return rc, outs, lib.rmx_last_error(eng._ctx)


@pytest.mark.parametrize("N", [256, 4096])
def test_refusals_leave_the_outputs_and_the_engine_alone(xc, N):
    """RMX_E_INVAL with the text of tests/host/test_caf_bands_request.cpp, in the entry's order: the head (a NULL buffer, a
    misaligned device pointer, n_dopplers), n_bands, the batch shape and the pair list, the weighting and the bands (window
    and band index named), the bounds, dop_frac over another output; poisoned outputs as they were; the next valid call
    answered as before."""
    import torch
    B, W, P, M = 3, 2, 3, 2
    iq, _, grid, lags, _ = br.scene(W, B, N, 3, seed=7100 + N)
    ok = br.band_set(M)
    ok_w = br.band_set(M, W)
    bad_w = ok_w.copy()
    bad_w[1, 1] = (0.3, -0.2)
    thin = ok.copy()
    thin[1] = (0.1 / N, 0.2 / N)
    nan_w = ok_w.copy()
    nan_w[1, 0, 0] = np.nan
    ok_lb = br.bounds_holding(lags, N)[0]
    bad_lb = ok_lb.copy()
    bad_lb[1] = (4, 3)
    few_lb = np.tile(ok_lb, (W, 1, 1))
    few_lb[1, 0] = (-N, 0)
    kw0 = dict(whiten=True, lag_bounds=ok_lb, fine=True)
    far_pairs = np.array([(0, 1), (0, 3), (1, 2)], np.int32)
    refused = [
        (dict(bands=None), b"NULL buffer"),
        (dict(bands=ok, n_dop=0, n_bands=0), b"n_dopplers 0 not in 1..4096"),            # the head in front of n_bands
        (dict(bands=ok, n_bands=0, weighting=7), b"n_bands 0 not in 1..64"),
        (dict(bands=ok, n_bands=65, lb=bad_lb), b"n_bands 65 not in 1..64"),
        (dict(bands=ok, n_win=W + 1, weighting=7, lb=bad_lb), b"n_windows 3 not in 0..max_windows="),   # the batch shape ...
        (dict(bands=ok, n_win=-1, weighting=7), b"n_windows -1 not in 0..max_windows="),
        (dict(bands=ok, pairs=far_pairs, P=-2, weighting=7), b"n_pairs -2 < 0"),
        (dict(bands=ok, P=2, weighting=7, lb=bad_lb), b"pairs == NULL needs n_pairs == 0 or 3, got 2"),
        (dict(bands=bad_w, bands_pw=1, pairs=far_pairs, weighting=7), b"pair 1 = (0,3) out of range for 3 buoys"),   # ... and the pair list
        (dict(bands=ok, weighting=7, lb=bad_lb), b"unknown weighting 7"),
        (dict(bands=bad_w, bands_pw=1, lb=bad_lb), b"band 1 of window 1: [0.3, -0.2] is not an interval"),
        (dict(bands=thin), b"band 1 of window 0 (one band set shared by every window)"),
        (dict(bands=thin), b"keeps no bin"),
        (dict(bands=nan_w, bands_pw=1), b"band 0 of window 1"),
        (dict(bands=ok, lb=bad_lb, weighting=1), b"lag_bounds of window -1, pair 1: [4, 3]"),
        (dict(bands=ok_w, bands_pw=1, lb=few_lb, lb_pw=1), b"lag_bounds of window 1, pair 0"),
    ]
    with _engine(xc, B, N, W) as eng:
        before = eng.caf_bands(iq, grid, ok, **kw0)
        for args, word in refused:
            rc, o, msg = _raw_call(xc, eng, iq, grid, **dict(dict(P=P), **args))
            assert rc == -1 and word in msg, (args, rc, msg)
            assert all(np.all(a == -77) for a in o), args
            _assert_same(eng.caf_bands(iq, grid, ok, **kw0), before, "the call after a refusal")
        # a device pointer aligned to less than its element: refused in the head, in front of n_dopplers and n_bands, the
        # device arrays (poisoned, with room around the pointer) as they were
        lib = xc.load_library()
        dev = torch.device("cuda", 0)
        n = W * M * P
        x_d = torch.from_numpy(np.ascontiguousarray(iq).view(np.float32).reshape(W, B, N, 2)).to(dev)
        spare = torch.zeros(W * B * N * 2 + 16, dtype=torch.float32, device=dev)
        gp = np.ascontiguousarray(grid, np.float64)
        for which, word in ((3, b"lag_frac is a device pointer 2 bytes past a multiple of 4"), (-1, b"iq is a device pointer 4 bytes past a multiple of 8")):
            o = [torch.full((n + 16,), -77, dtype=t, device=dev) for t in (torch.int32, torch.float32, torch.int32, torch.float32, torch.float32)]
            torch.cuda.synchronize()
            ptrs = [t.data_ptr() + 32 + (2 if k == which else 0) for k, t in enumerate(o)]
            in_ptr = x_d.data_ptr() if which >= 0 else spare.data_ptr() + 4
            rc = lib.rmx_caf_batch_bands(eng._ctx, C.c_void_p(in_ptr), W, None, P, gp.ctypes.data_as(C.c_void_p), 0, ok.ctypes.data_as(C.c_void_p),
                                         0, 0, 7, None, 0, *[C.c_void_p(p) for p in ptrs], xc.RMX_IN_DEVICE | xc.RMX_OUT_DEVICE)
            msg = lib.rmx_last_error(eng._ctx)
            assert rc == -1 and word in msg, (which, rc, msg)
            assert lib.rmx_synchronize(eng._ctx) == 0
            assert all(bool(torch.all(t == -77)) for t in o), which
            _assert_same(eng.caf_bands(iq, grid, ok, **kw0), before, "the call after a misaligned pointer")
        rc, o, msg = _raw_call(xc, eng, iq[:0], grid, P, bands=ok)                        # an empty batch: RMX_OK, nothing written
        assert rc == 0
        for k, name in ((0, b"dop_idx"), (2, b"lag_int"), (3, b"lag_frac"), (4, b"peak")):
            outs = [np.full((W, M, P), -77, np.int32), None, np.full((W, M, P), -77, np.int32), np.full((W, M, P), -77, np.float32),
                    np.full((W, M, P), -77, np.float32)]
            outs[1] = outs[k].view(np.float32)
            rc, o, msg = _raw_call(xc, eng, iq, grid, P, bands=ok, weighting=1, lb=ok_lb, outs=outs)
            assert rc == -1 and b"dop_frac overlaps " + name in msg and b"%d floats" % (W * M * P) in msg, (k, rc, msg)
            assert all(np.all(o[m] == -77) for m in (0, 2, 3, 4)), k
        _assert_same(eng.caf_bands(iq, grid, ok, **kw0), before, "the call after the refusals")
        with pytest.raises(xc.RmxError) as e:
            eng.caf_bands(iq, grid, thin)
        assert e.value.code == -1 and "keeps no bin" in str(e.value)
        with pytest.raises(ValueError):
            eng.caf_bands(iq, grid, np.zeros((65, 2)))


# ---- 7. the state an engine keeps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4096, 1024, 8192])
def test_state_between_calls(xc, N):
    """One engine through caf_bands, caf, correlate_bands and correlate, with growing and shrinking W, M and D (N = 4096:
    the per-hypothesis path after the one-launch path): each answer is, bit for bit, a fresh engine's."""
    B, WMAX = 3, 12
    iq, raw, grid9, lags, _ = br.scene(WMAX, B, N, 9, seed=6100 + N)
    lb = br.bounds_holding(lags, N)
    g5 = grid9[2:7]
    eng_opts = (("chunk_windows", 8),) if N == 4096 else ()
    calls = [("caf_bands", 2, dict(doppler_cps=g5, bands=br.band_set(2))),
             ("caf", 2, dict(doppler_cps=g5, band=np.array(br.EMITTER_BANDS[1]), fine=True)),
             ("caf_bands", WMAX, dict(doppler_cps=grid9, bands=br.band_set(3, WMAX), lag_bounds=lb, whiten=True, fine=True)),
             ("correlate_bands", 5, dict(bands=br.band_set(3, 5), lag_bounds=lb[:5])),
             ("caf_bands", 3, dict(doppler_cps=grid9[3:6], bands=br.band_set(1, 3), fine=True)),
             ("correlate", 4, {}),
             ("caf_bands", 4, dict(doppler_cps=grid9[4:5], bands=br.band_set(3), lag_bounds=lb[:4], fine=True)),
             ("caf", 3, dict(doppler_cps=grid9)),
             ("caf_bands", WMAX, dict(doppler_cps=g5, bands=br.band_set(2, WMAX), whiten=True)),
             ("correlate_bands", 2, dict(bands=br.band_set(2))),
             ("caf_bands", 2, dict(doppler_cps=g5, bands=br.band_set(2)))]

    def run(eng, name, w, kw):
        kw = dict(kw)
        args = [raw[:w] if name == "correlate" else iq[:w]]
        if "doppler_cps" in kw:
            args.append(kw.pop("doppler_cps"))
        if "bands" in kw:
            args.append(kw.pop("bands"))
        return getattr(eng, name)(*args, **kw)

    with _engine(xc, B, N, WMAX, eng_opts) as eng:
        for name, w, kw in calls:
            got = run(eng, name, w, kw)
            with _engine(xc, B, N, WMAX, eng_opts) as fresh:
                want = run(fresh, name, w, kw)
            _assert_same(got, want, "%s W=%d" % (name, w), names=["out%d" % k for k in range(len(got))])


# ---- 8. the seam ------------------------------------------------------------------------------------------------------------------------
def test_seam_share_doppler_gives_the_measurements_of_the_separate_searches(xc):
    """TDoAProcessor with band_limit, share_captures and doppler_search_hz on the two-emitter capture: share_doppler sends both
    frequency groups through ONE caf_bands call; the measurements, frequency_offset_hz included, are those of the two
    separate searches in the same order, with and without bound_lags; with the flag off nothing changes."""
    from radio_mapper_amd import tdoa_processor as tp
    N, fs, fc = 4096, 2.048e6, 121.0e6
    iq, grid, la, ha, lw, hb = rr.two_emitter_scene(N, W=1)
    step_hz = 0.5 / N * fs
    buoys = [("B0", 37.0, -122.0), ("B1", 37.3, -122.0), ("B2", 37.0, -121.6)]
    f_of = {"strong": fc + 0.10 * fs, "weak": fc - 0.25 * fs}
    t0 = 1_700_000_000_000_000_000

    def run(bound_lags, **flags):
        p = tp.TDoAProcessor(band_limit=True, doppler_search_hz=(2 * step_hz, step_hz), **flags)
        p.tdoa_calculator.bound_lags = bound_lags
        for bid, lat, lng in buoys:
            p.register_buoy(tp.BuoyPosition(bid, lat, lng, 0.0, timing_accuracy_ns=20))
        calls, groups = [], []
        eng_of = p.tdoa_calculator._engine

        def engine(*a, **k):
            eng = eng_of(*a, **k)
            if not getattr(eng, "_recorded", False):
                for name in ("caf", "caf_bands"):
                    def rec(*aa, _f=getattr(eng, name), _n=name, **kk):
                        calls.append((_n, np.asarray(aa[0]).shape[0]))
                        return _f(*aa, **kk)
                    setattr(eng, name, rec)
                eng._recorded = True
            return eng
        p.tdoa_calculator._engine = engine
        p.hyperbolic_positioner.triangulate_position = lambda meas, pos: groups.append(list(meas))
        dets = []
        for f in f_of.values():
            dets += [tp.SignalDetection(bid, f / 1e6, -60.0, "t", t0, lat, lng, 0.9, iq_samples=iq[0, b], sample_rate_hz=fs,
                                        center_freq_hz=fc, bandwidth_hz=0.1 * fs) for b, (bid, lat, lng) in enumerate(buoys)]
        p.process_signal_detections(dets)
        p.tdoa_calculator.close()
        return calls, [[(m.buoy1_id, m.buoy2_id, m.frequency_mhz, m.time_difference_ns, m.confidence, m.frequency_offset_hz) for m in g]
                       for g in groups]

    for bound_lags in (False, True):
        calls_on, meas_on = run(bound_lags, share_captures=True, share_doppler=True)
        calls_off, meas_off = run(bound_lags, share_captures=True)
        assert calls_on == [("caf_bands", 1)] and calls_off == [("caf", 2)], (calls_on, calls_off)
        assert run(bound_lags, share_doppler=True)[0] == calls_off           # share_doppler needs share_captures
        assert len(meas_on) == 2 and meas_on == meas_off
        if not bound_lags:
            for g, lags, hyp in zip(meas_on, (la[0], lw[0]), (ha, hb)):
                assert [round(m[3] * 1e-9 * fs) for m in g] == lags.tolist()
                assert np.all(np.abs(np.array([m[5] for m in g]) - (hyp - len(grid) // 2) * step_hz) <= 0.1 * step_hz)
