"""rmx_caf_batch_quality, the refined and qualified lags of the Doppler search, on the GPU: the smallest shape of every route
against the float64 restatement (tests/caf_quality_ref.py) at the bars of the refined and the quality entries, the two
kernels bit for bit against the engine's own correlate(refine, quality) on host-rotated windows, the identities with
rmx_caf_batch_request, the launch counts of the one-launch path and of the second sweep, the caller's memory and the
refusals through the raw ABI, and a dead receiver.

The scenes' slots win under different hypotheses, pair by pair and window by window (tests/test_caf_quality_cpu.py asserts
it on the reference, with the margins that make exact winners and exact coarse lags fair demands): a slot that read
another slot's winner -- under the one-launch virtual window or across the second sweep -- misses the parity bars."""
import ctypes as C

import numpy as np
import pytest

import caf_quality_ref as cq
import caf_ref as cr
import caf_request_ref as rq
import caller_memory_ref as cm
import quality_ref as qr
from test_gpu_caf import _engine, _expected, _launches

pytestmark = pytest.mark.gpu
U = cq.REFINE


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


def _assert_same(a, b, what):
    assert len(a) == len(b), what
    for k, (u, v) in enumerate(zip(a, b)):
        assert u.dtype == v.dtype and u.shape == v.shape, (what, k)
        assert np.array_equal(_bits(u), _bits(v)), "%s, array %d: %d of %d elements differ" % (what, k, int((_bits(u) != _bits(v)).sum()), u.size)


def _with_tail(want, kind, D, chunks, quality, refine):
    """the launch counts of rmx_caf_batch_request plus what the entry adds: one launch of each kernel where every hypothesis
    is resident; elsewhere, per chunk, D more forward launches and D launches of each kernel"""
    want = dict(want)
    n = 1 if kind == "one" else chunks * D
    if kind != "one" and (quality or refine):
        for fam in {"small": ("g_fwd_small",), "four": ("g_cols_fwd", "g_rows_fwd"), "per": ("k_fwd",)}[kind]:
            want[fam] += n
    if quality:
        want["k_quality"] = n
    if refine:
        want["k_refine"] = n
    return want


def _assert_parity(got, ref, N, refine):
    """got = (dop, dop_frac, lag_int, lag_frac, peak, quality) of caf(fine=True, refine, quality=True)"""
    dop, dfrac, li, lf, pk, qual = got
    assert (dop.dtype, li.dtype, lf.dtype, pk.dtype, qual.dtype) == (np.int32, np.int32, np.float32, np.float32, np.float32)
    assert ref["hyp_margin"].min() > cr.MARGIN_BAR and ref["lag_margin"].min() > rq.LAG_MARGIN_BAR
    assert np.array_equal(dop, ref["dop"]), "%d winners differ" % int((dop != ref["dop"]).sum())
    have = li + lf.astype(np.float64)
    if refine:
        want = ref["fine_int"] + ref["fine_frac"]
        err = np.abs(have - want)
        print("worst refined lag error %.3e, worst peak %.3e" % (err.max(), (np.abs(pk - ref["fine_peak"]) / ref["fine_peak"]).max()))
        assert np.all((err <= 1e-5 * np.maximum(np.abs(want), 1.0)) | (err <= ref["fine_bound"])), "refined lag outside the rule: %.3e" % err.max()
        assert np.all(np.abs(pk - ref["fine_peak"]) <= 1e-5 * ref["fine_peak"] + 1e-6 * ref["full_max"])
    else:
        assert np.array_equal(li, ref["lag_int"]), "%d coarse lags differ" % int((li != ref["lag_int"]).sum())
        want = ref["lag_int"] + ref["lag_frac"]
        rel = np.abs(have - want) / np.maximum(np.abs(want), 1.0)
        assert np.all((rel <= 1e-5) | (rel <= 4.0 * ref["flat_bound"])), "coarse lag outside the rule: %.3e" % rel.max()
        assert np.allclose(pk, ref["peak"], rtol=1e-5, atol=0)
    rq_ = ref["quality"]
    assert np.all(np.isfinite(qual))
    for k, name in ((qr.COHERENCE, "coherence"), (qr.RMS_BW, "rms_bw"), (qr.NEFF, "n_eff")):
        rel = np.abs(qual[..., k] - rq_[..., k]) / np.abs(rq_[..., k])
        assert rel.max() <= 1e-4, "%s off by %.3e" % (name, rel.max())
    a, b = qr.et_over_p2(qual, N), qr.et_over_p2(rq_, N)
    assert np.all(np.abs(a - b) <= 1e-4 * b), "psr (as Et / p0^2) off by %.3e" % (np.abs(a - b) / b).max()


# ---- 1. every route: parity, identities, launch counts ------------------------------------------------------------------------
# (id, scene, kind, chunks, default options, engine options, row family with the default list / with the custom one)
ROUTES = [
    ("small N=16", "n16", "small", 1, {}, (), None, None),
    ("small N=256", "n256", "small", 1, {}, (), None, None),
    ("four-step N=8192 B=4", "n8192b4", "four", 1, {}, (), "g_rows_inv", "g_rows_inv"),
    ("four-step N=8192 B=6 anchor", "n8192b6", "four", 1, {}, (), "g_rows_anchor", "g_rows_inv"),
    ("one launch W=3 resident=0", "one3", "one", 1, {}, (("resident", 0),), None, None),
    ("one launch W=3 resident=1", "one3", "one", 1, {}, (("resident", 1),), None, None),
    ("N=4096 chunks 8+4", "chunked12", "per", 2, {}, (("chunk_windows", 8),), None, None),
    ("small N=256 chunks 2+2+1", "seam256", "small", 3, {"gen_chunk": 2}, (), None, None),
    ("four-step N=8192 chunks 2+2+1", "seam8192", "four", 3, {"gen_chunk": 2}, (), "g_rows_inv", "g_rows_inv"),
]


@pytest.mark.parametrize("custom", [False, True], ids=["default all", "custom phat"])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_against_the_reference(xc, opts, route, custom):
    """The default pair list under per-window bounds + per-window bands + PHAT, the custom one under PHAT: the request call's
    launches and bits when nothing is asked; quality alone leaves the five other arrays alone; refine moves neither dop_idx
    nor dop_frac nor quality; uint8 equals complex64; parity with refine = 0 and refine = 8."""
    _, name, kind, chunks, defaults, eng_opts, rows_def, rows_custom = route
    for k, v in defaults.items():
        opts(k, v)
    W, B, N, D, _ = cq.SCENES[name]
    iq, raw, grid, pairs, kw = cq.case(name, custom)
    ref = cq.case_reference(name, custom)
    want = _expected(kind, D, chunks, rows_custom if custom else rows_def)
    with _engine(xc, B, N, W, eng_opts) as eng:
        base = eng.caf(iq, grid, pairs, fine=True, **kw)
        assert _launches(eng) == want, _launches(eng)
        none = eng.caf(iq, grid, pairs, fine=True, refine=0, quality=False, **kw)
        assert _launches(eng) == want, _launches(eng)
        _assert_same(none, base, "refine=0, quality=False against the request call")
        q0 = eng.caf(iq, grid, pairs, fine=True, quality=True, **kw)
        assert _launches(eng) == _with_tail(want, kind, D, chunks, True, False), _launches(eng)
        _assert_same(q0[:5], base, "quality=True: the five other arrays")
        _assert_parity(q0, ref, N, 0)
        full = eng.caf(iq, grid, pairs, fine=True, refine=U, quality=True, **kw)
        assert _launches(eng) == _with_tail(want, kind, D, chunks, True, True), _launches(eng)
        _assert_same(full[:2], base[:2], "refine: dop_idx and dop_frac")
        _assert_same(full[5:], q0[5:], "refine: quality is computed with the coarse peak")
        _assert_parity(full, ref, N, U)
        assert np.all(np.abs(full[2] - base[2]) <= 1)
        only = eng.caf(iq, grid, pairs, refine=U, **kw)
        assert _launches(eng) == _with_tail(want, kind, D, chunks, False, True), _launches(eng)
        _assert_same(only, (full[0],) + full[2:5], "refine without quality and without dop_frac")
        full8 = eng.caf(raw, grid, pairs, fine=True, refine=U, quality=True, **kw)
        _assert_same(full8, full, "uint8 against complex64")
    if chunks > 1 and kind != "per":   # a chunked call equals a one-chunk call
        xc.clear_default_options()
        with _engine(xc, B, N, W, eng_opts) as whole:
            one = whole.caf(iq, grid, pairs, fine=True, refine=U, quality=True, **kw)
            assert _launches(whole) == _with_tail(_expected(kind, D, 1, rows_custom if custom else rows_def), kind, D, 1, True, True)
            _assert_same(full, one, "chunked against one chunk")


def test_chunked_4096_equals_the_one_launch_path(xc):
    """N = 4096, W = 12: chunks of 8 + 4 through the second sweep against every hypothesis resident in one launch -- the
    same kernels read the same spectra, so all six arrays agree bit for bit."""
    W, B, N, D, _ = cq.SCENES["chunked12"]
    iq, raw, grid, pairs, kw = cq.case("chunked12", False)
    with _engine(xc, B, N, W, (("chunk_windows", 8),)) as cut, _engine(xc, B, N, W) as whole:
        a = cut.caf(iq, grid, fine=True, refine=U, quality=True, **kw)
        b = whole.caf(iq, grid, fine=True, refine=U, quality=True, **kw)
        assert _launches(whole) == _with_tail(_expected("one", D), "one", D, 1, True, True), _launches(whole)
        _assert_same(a, b, "second sweep against one launch")


# ---- 2. the two kernels bit for bit against correlate() on host-rotated windows ---------------------------------------------
# (id, N, W, engine options): tests/test_gpu_caf_request.py's EXACT
EXACT = [
    ("N=256", 256, 3, ()),
    ("N=8192", 8192, 2, ()),
    ("N=4096 one launch", 4096, 3, ()),
    ("N=4096 chunked", 4096, 12, (("chunk_windows", 8),)),
]


def _take(a, dop):
    """a [W][P][...][D] at the winner -> [W][P][...]"""
    idx = dop.reshape(dop.shape + (1,) * (a.ndim - 2))
    return np.take_along_axis(a, np.broadcast_to(idx, a.shape[:-1] + (1,)), axis=-1)[..., 0]


@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_refine_and_quality_bit_for_bit_against_correlate(xc, case):
    """Buoys 2 and 3 rotated on the host, CROSS_PAIRS: under PHAT and under band + bounds, caf(refine=U, quality=True) IS
    correlate(host-rotated, refine=U, quality=True, the same request) taken at the coarse first maximum, on all four
    outputs, and so is refine = 0: k_quality<CafWinner> and k_refine<CafWinner> are the plain bodies on the same spectra."""
    _, N, W, eng_opts = case
    iq, raw, grid, _ = cr.scene(W, 4, N, 3, seed=300 + N + W)
    pairs = cr.CROSS_PAIRS
    lb = np.array([[-(N // 2), N // 3]] * len(pairs), np.int32)
    with _engine(xc, 4, N, W, eng_opts) as eng:
        for rid, kw in (("phat", dict(whiten=True)), ("band + bounds", dict(band=np.array([-0.28, 0.31]), lag_bounds=lb))):
            per = {0: [], U: []}
            for nu in grid:
                x = iq.copy()
                x[:, 2:] = cr.rot_mul(iq[:, 2:], cr.libm_phasor(nu, N))
                for u in per:
                    per[u].append(eng.correlate(x, pairs, refine=u, quality=True, **kw))
            coarse = [np.stack([r[k] for r in per[0]], axis=-1) for k in range(4)]
            dop = cr.first_max(coarse[2])
            assert len(set(dop.ravel().tolist())) > 1
            for u in per:
                want = [_take(np.stack([r[k] for r in per[u]], axis=-1), dop) for k in range(4)]
                for x in (iq, raw):
                    got = eng.caf(x, grid, pairs, refine=u, quality=True, **kw)
                    assert np.array_equal(got[0], dop), rid
                    _assert_same(got[1:], want, "%s, refine=%d: caf against correlate() of the host-rotated windows" % (rid, u))


# ---- 3. the caller's memory, the refusals and a dead receiver through the raw ABI ------------------------------------------
OUT_NAMES = ("dop_idx", "dop_frac", "lag_int", "lag_frac", "peak", "quality")


def _raw_call(xc, eng, iq_ptr, W, P, grid, ptrs, refine=U, u8=False, weighting=1, flags=None):
    lib = xc.load_library()
    gp = np.ascontiguousarray(grid, np.float64)
    vp = lambda p: None if not p else C.c_void_p(p)   # noqa: E731
    flags = (xc.RMX_IN_DEVICE | xc.RMX_OUT_DEVICE) if flags is None else flags
    return lib.rmx_caf_batch_quality(eng._ctx, vp(iq_ptr), W, None, P, gp.ctypes.data_as(C.c_void_p), len(gp), None, 0, weighting, None, 0,
                                     refine, vp(ptrs["dop_idx"]), vp(ptrs["dop_frac"]), vp(ptrs["lag_int"]), vp(ptrs["lag_frac"]),
                                     vp(ptrs["peak"]), vp(ptrs["quality"]), flags | (xc.RMX_IN_U8 if u8 else 0))


def _slab(torch, arrays, placement):
    lay = cm.layout(arrays, placement)
    before = cm.fill(lay)
    t = torch.from_numpy(before).to(torch.device("cuda", 0))
    assert t.data_ptr() % cm.BASE_ALIGN == 0
    return lay, before, t


MEMORY = [("one launch", "one3", ()), ("small chunks 2+2+1", "seam256", ()), ("N=4096 chunks 8+4", "chunked12", (("chunk_windows", 8),))]


@pytest.mark.parametrize("placement", cm.PLACEMENTS)
@pytest.mark.parametrize("case", MEMORY, ids=[c[0] for c in MEMORY])
def test_device_pointers_between_guards(xc, opts, case, placement):
    """RMX_OUT_DEVICE with every output between two guards: the six arrays are those of the host door bit for bit, every
    element is written, no guard word and no byte of the input changes."""
    import torch
    _, name, eng_opts = case
    if name == "seam256":
        opts("gen_chunk", 2)
    W, B, N, D, _ = cq.SCENES[name]
    iq, raw, grid, _, _ = cq.case(name, False)
    P = B * (B - 1) // 2
    slots = W * P
    arrays = [("lag_int", np.int32, slots), ("lag_frac", np.float32, slots), ("peak", np.float32, slots), ("quality", np.float32, 4 * slots),
              ("dop_idx", np.int32, slots), ("dop_frac", np.float32, slots)]
    with _engine(xc, B, N, W, eng_opts) as eng:
        want = eng.caf(iq, grid, whiten=True, fine=True, refine=U, quality=True)
        lay, before, t = _slab(torch, arrays, placement)
        in_lay = cm.layout([("iq", np.complex64, iq.size)], placement)
        in_before = cm.fill(in_lay)
        cm.put(in_before, in_lay, "iq", iq)
        t_in = torch.from_numpy(in_before).to(torch.device("cuda", 0))
        ptrs = {n: t.data_ptr() + lay.entries[n].offset for n in OUT_NAMES}
        rc = _raw_call(xc, eng, t_in.data_ptr() + in_lay.entries["iq"].offset, W, P, grid, ptrs)
        assert rc == 0, eng._lib.rmx_last_error(eng._ctx)
        eng.synchronize()
        after = t.cpu().numpy()
        bad = cm.check(before, after, lay, OUT_NAMES)
        assert not bad, "%d findings, the first: %s" % (len(bad), bad[:8])
        assert np.array_equal(t_in.cpu().numpy(), in_before)
        got = [cm.cut(after, lay, n, (W, P, 4) if n == "quality" else (W, P)) for n in OUT_NAMES]
        _assert_same(got, want, "device door against host door")


def test_refusals_in_their_order_leave_every_output_untouched(xc):
    """rmx_caf_batch_request's own refusals first (here: the weighting), then refine with its value, then quality over
    another output with the array's name, then a misaligned device quality; and an empty batch is RMX_OK.  Nothing is
    written by any of them."""
    import torch
    W, B, N, D, _ = cq.SCENES["seam256"]
    iq, _, grid, _, _ = cq.case("seam256", False)
    P = B * (B - 1) // 2
    slots = W * P
    arrays = [("lag_int", np.int32, slots), ("lag_frac", np.float32, slots), ("peak", np.float32, slots), ("quality", np.float32, 4 * slots),
              ("dop_idx", np.int32, slots), ("dop_frac", np.float32, slots)]
    lay, before, t = _slab(torch, arrays, "aligned")
    t_in = torch.from_numpy(np.ascontiguousarray(iq).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))
    ptrs = {n: t.data_ptr() + lay.entries[n].offset for n in OUT_NAMES}
    with _engine(xc, B, N, W) as eng:
        def refused(text, **kw):
            moved = dict(ptrs, **{k: v for k, v in kw.items() if k in ptrs})
            rest = {k: v for k, v in kw.items() if k not in ptrs}
            rc = _raw_call(xc, eng, t_in.data_ptr(), W, P, grid, moved, **rest)
            msg = eng._lib.rmx_last_error(eng._ctx).decode()
            assert rc == -1 and text in msg, (rc, msg)   # RMX_E_INVAL
            eng.synchronize()
            assert np.array_equal(t.cpu().numpy(), before), "a refused call wrote: " + msg
        refused("unknown weighting 7", weighting=7, refine=3, quality=ptrs["peak"])             # the request entry's own come first
        refused("refine = 3", refine=3, quality=ptrs["peak"] + 2)                               # then refine, with the value
        for name in ("dop_idx", "dop_frac", "lag_int", "lag_frac", "peak"):
            refused("quality overlaps %s" % name, quality=ptrs[name] + 2)                      # then the overlap, naming the array
        refused("quality is a device pointer 2 bytes past a multiple of 4", quality=ptrs["quality"] + 2)
        refused("dop_frac overlaps peak", dop_frac=ptrs["peak"], refine=3)                      # (dop_frac's own check precedes refine)
        lib = xc.load_library()
        for w, p in ((0, P), (W, 0)):
            rc = lib.rmx_caf_batch_quality(eng._ctx, C.c_void_p(t_in.data_ptr()), w, np.zeros((1, 2), np.int32).ctypes.data_as(C.c_void_p) if p == 0 else None, p,
                                           np.ascontiguousarray(grid).ctypes.data_as(C.c_void_p), len(grid), None, 0, 1, None, 0, U,
                                           *[C.c_void_p(ptrs[n]) for n in OUT_NAMES], xc.RMX_IN_DEVICE | xc.RMX_OUT_DEVICE)
            assert rc == 0
        eng.synchronize()
        assert np.array_equal(t.cpu().numpy(), before)


@pytest.mark.parametrize("case", [("N=256", 256, ()), ("N=4096 one launch", 4096, ()), ("N=8192", 8192, ())], ids=lambda c: c[0])
def test_a_dead_receiver_gives_four_zeros(xc, case):
    """buoy 1 all zeros: its pairs' peak is 0 under every hypothesis -- hypothesis 0 wins --, the four figures are 0, nothing
    is NaN, and the live pair keeps its values"""
    _, N, eng_opts = case
    iq, _, grid, _ = cr.scene(2, 3, N, 3, seed=77 + N)
    x = iq.copy()
    x[:, 1] = 0
    with _engine(xc, 3, N, 2, eng_opts) as eng:
        for kw in ({}, dict(whiten=True)):
            dop, li, lf, pk, qual = eng.caf(x, grid, refine=U, quality=True, **kw)
            assert np.all(np.isfinite(qual)) and np.all(np.isfinite(lf)) and np.all(np.isfinite(pk))
            for q in (0, 2):   # pairs (0, 1) and (1, 2)
                assert not qual[:, q].any() and not pk[:, q].any() and not dop[:, q].any()
            assert np.all(qual[:, 1] > 0) and np.all(pk[:, 1] > 0)
