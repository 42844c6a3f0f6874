"""rmx_caf_batch, the Doppler-grid search, on the GPU: every route against the oracle's per-hypothesis loop
(tests/caf_ref.py), the chunk seams, the rotation and the selection bit for bit, ties between hypotheses, the pointer
flags, the state an engine keeps between calls, the limits of n_dopplers and the two fall-back thresholds of the
one-launch path.

Parity is the project's rule (tests/test_gpu_parity.py), applied to the winning row: dop_idx exact where the oracle's best
hypothesis stands more than 1e-3 above its second best -- asserted of every scene, never masked --, lag_int exact unless the
oracle's own two largest magnitudes are within 1e-5 and the GPU's lag is the second of them, lag_int + lag_frac within
1e-5 max(|lag|, 1) or within four times oracle.parabola_ulp_bound (a flat peak), peak to rtol 1e-5.  Everything else here is
exact equality.  Every case also reads rmx_last_timing_kind: the kernel families that ran, and how often."""
import ctypes as C

import numpy as np
import pytest

import caf_ref as cr

pytestmark = pytest.mark.gpu
TOL = 1e-5
NAMES = ("dop_idx", "lag_int", "lag_frac", "peak")


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


# ---- scenes and references: computed once, shared, never written to ---------------------------------------------------
_SCENES, _REFS = {}, {}


def _scene(name):
    if name not in _SCENES:
        iq, raw, grid, k = cr.scene_of(name)
        for a in (iq, raw, grid):
            a.setflags(write=False)
        _SCENES[name] = (iq, raw, grid)
    return _SCENES[name]


def _ref(name, custom):
    if (name, custom) not in _REFS:
        iq, _, grid = _scene(name)
        _REFS[name, custom] = cr.reference(iq, grid, cr.custom_pairs(iq.shape[1]) if custom else None)
    return _REFS[name, custom]


def _assert_parity(got, ref):
    dop, li, lf, pk = got
    assert (dop.dtype, li.dtype, lf.dtype, pk.dtype) == (np.int32, np.int32, np.float32, np.float32)
    margin = float(ref["hyp_margin"].min())
    print("hypothesis margin %.3e" % margin)
    assert margin > cr.MARGIN_BAR                       # the condition on the inputs: holds for every pair-window
    assert np.array_equal(dop, ref["dop"]), "%d winning hypotheses differ" % int((dop != ref["dop"]).sum())
    ri, rf, rp = ref["lag_int"], ref["lag_frac"], ref["peak"]
    bad = li != ri
    excused = bad & (ref["lag_margin"] <= TOL) & (li == ref["lag_second"])
    assert not np.any(bad & ~excused), "%d integer lags differ" % int(np.sum(bad & ~excused))
    ok = ~bad
    want, have = ri + rf, li + lf.astype(np.float64)
    rel = np.abs(have - want) / np.maximum(np.abs(want), 1.0)
    print("worst lag %.3e, worst peak %.3e" % (rel[ok].max(), (np.abs(pk - rp) / rp)[ok].max()))
    assert np.all(((rel <= TOL) | (rel <= 4.0 * ref["flat_bound"]))[ok]), "fractional lag outside the rule: %.3e" % rel[ok].max()
    assert np.allclose(pk[ok], rp[ok], rtol=1e-5, atol=0)


def _assert_same(a, b, what=""):
    for name, u, v in zip(NAMES, a, b):
        assert u.dtype == v.dtype and u.shape == v.shape, (what, name)
        assert np.array_equal(u.view(np.int32), v.view(np.int32)), \
            "%s %s: %d of %d elements differ" % (what, name, int((u.view(np.int32) != v.view(np.int32)).sum()), u.size)


def _launches(eng):
    return {k: v["launches"] for k, v in eng.last_timing_by_kernel().items()}


def _expected(kind, D, chunks=1, rows="g_rows_inv"):
    """launch counts of one rmx_caf_batch call: per chunk the un-rotated spectra once, then per hypothesis the de-rotated
    spectra, the pair kernels and k_caf_select -- or, N = 4096 in one launch, two k_fwd, one pair launch, one selection"""
    f, p = chunks * (1 + D), chunks * D
    if kind == "small":
        return {"g_fwd_small": f, "g_pair_small": p, "k_caf_select": p}
    if kind == "four":
        return {"g_cols_fwd": f, "g_rows_fwd": f, rows: p, "g_cols_inv": p, "g_final": p, "k_caf_select": p}
    if kind == "one":
        return {"k_fwd": 2, "k_win|k_pair": 1, "k_caf_select": 1}
    assert kind == "per"
    return {"k_fwd": f, "k_win|k_pair": p, "k_caf_select": p}


def _engine(xc, B, N, W, eng_opts=()):
    eng = xc.XcorrEngine(B, N, W)
    eng.set_option("timing", 1)
    for k, v in eng_opts:
        eng.set_option(k, v)
    return eng


# ---- 1. every route against the oracle ---------------------------------------------------------------------------------
# (id, scene, kind, chunks, default options, engine options, row family with the default list / with the custom one)
ROUTES = [
    ("small N=16", "n16", "small", 1, {}, (), None, None),
    ("small N=256", "n256", "small", 1, {}, (), None, None),
    ("small N=2048", "n2048", "small", 1, {}, (), None, None),
    ("small N=4096 generic4096", "g4096", "small", 1, {"generic4096": 1}, (), None, None),
    ("four-step N=8192", "n8192", "four", 1, {}, (), "g_rows_inv", "g_rows_inv"),
    ("four-step N=16384", "n16384", "four", 1, {}, (), "g_rows_inv", "g_rows_inv"),
    ("four-step N=65536", "n65536", "four", 1, {}, (), "g_rows_inv", "g_rows_inv"),
    ("four-step N=8192 anchor", "n8192b6", "four", 1, {}, (), "g_rows_anchor", "g_rows_inv"),
    ("one launch DW=40", "one8", "one", 1, {}, (), None, None),
    ("one launch DW=21", "one3", "one", 1, {}, (), None, None),
    ("one launch ppb=3", "one8", "one", 1, {}, (("pairs_per_block", 3),), None, None),
    ("one launch resident=1", "one8", "one", 1, {}, (("resident", 1),), None, None),
    ("one launch resident=0", "one8", "one", 1, {}, (("resident", 0),), None, None),
    ("one launch resident=0 DW=21", "one3", "one", 1, {}, (("resident", 0),), None, None),
    ("per hypothesis chunks 8+8+4", "chunked", "per", 3, {}, (("chunk_windows", 8),), None, None),
    ("per hypothesis resident=1", "chunked", "per", 3, {}, (("chunk_windows", 8), ("resident", 1)), None, None),
    ("per hypothesis resident=0", "chunked", "per", 3, {}, (("chunk_windows", 8), ("resident", 0)), None, None),
]


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_against_the_oracle(xc, opts, route):
    _, name, kind, chunks, defaults, eng_opts, rows_def, rows_custom = route
    for k, v in defaults.items():
        opts(k, v)
    iq, raw, grid = _scene(name)
    W, B, N = iq.shape
    with _engine(xc, B, N, W, eng_opts) as eng:
        for custom in (False, True):
            pairs = cr.custom_pairs(B) if custom else None
            got = eng.caf(iq, grid, pairs)
            assert _launches(eng) == _expected(kind, len(grid), chunks, rows_custom if custom else rows_def), (custom, _launches(eng))
            got8 = eng.caf(raw, grid, pairs)
            assert _launches(eng) == _expected(kind, len(grid), chunks, rows_custom if custom else rows_def), (custom, _launches(eng))
            _assert_same(got8, got, "uint8 against complex64 (custom list: %s)" % custom)
            _assert_parity(got, _ref(name, custom))


# ---- 2. chunk seams on the generic paths --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("seam256", "small"), ("seam8192", "four")])
def test_chunk_seams_of_the_generic_paths(xc, opts, name, kind):
    """gen_chunk = 2 cuts five windows into chunks of 2, 2 and 1: g_fwd_small / g_cols_fwd with first_item > 0 and a
    phasor table, k_caf_select with first > 0.  Oracle parity, and the bits of an engine that took the batch whole."""
    iq, raw, grid = _scene(name)
    W, B, N = iq.shape
    assert W == 5
    with _engine(xc, B, N, W) as whole:
        opts("gen_chunk", 2)
        with _engine(xc, B, N, W) as cut:
            for custom in (False, True):
                pairs = cr.custom_pairs(B) if custom else None
                ref = _ref(name, custom)
                assert len({tuple(r) for r in ref["dop"].tolist()}) > 1   # a window taken from the wrong chunk would show
                for x in (iq, raw):
                    got = cut.caf(x, grid, pairs)
                    assert _launches(cut) == _expected(kind, len(grid), 3), _launches(cut)
                    one = whole.caf(x, grid, pairs)
                    assert _launches(whole) == _expected(kind, len(grid), 1), _launches(whole)
                    _assert_same(got, one, "chunks of two against one chunk")
                    _assert_parity(got, ref)


# ---- 3. rotation and selection, bit for bit -----------------------------------------------------------------------------
# (id, N, W, default options that send correlate() through the kernels the search uses, engine options, families of that
#  correlate(), kind of the search with D = 3, its chunks)
EXACT = [
    ("N=256", 256, 3, {"wfused": 0, "wscr": 0}, (), {"g_fwd_small", "g_pair_small"}, "small", 1),
    ("N=8192", 8192, 2, {"wscr": 0, "fused": 0}, (), {"g_cols_fwd", "g_rows_fwd", "g_rows_inv", "g_cols_inv", "g_final"}, "four", 1),
    ("N=4096 one launch", 4096, 3, {}, (), {"k_fwd", "k_win|k_pair"}, "one", 1),
    ("N=4096 chunked", 4096, 12, {}, (("chunk_windows", 8),), {"k_fwd", "k_win|k_pair"}, "per", 2),
]


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_rotation_and_selection_bit_for_bit(xc, opts, case, D):
    """The search IS: rotate x_j by the table, correlate as the plain call does, keep the d-major first maximum.  So with
    buoys 2 and 3 rotated on the host -- the table's values (caf_ref.libm_phasor, which test_caf_ref_cpu.py holds equal to
    the oracle's doppler_phasor), the product as gen::rot_mul rounds it (caf_ref.rot_mul) -- the engine's own correlate()
    of every hypothesis, reduced by caf_ref.first_max, must give caf()'s four arrays bit for bit: rot_mul in the three
    loaders, the phasor table, spec_j and both selection kernels, without a tolerance.
    (The rotation is NOT taken from numpy's complex64 product, as the oracle takes it: that product fuses a multiply into
    the add on CPUs with FMA and then differs from rot_mul in the last bit.  test_every_route_against_the_oracle holds
    the search to the oracle's own rotation under the parity rule.)"""
    _, N, W, defaults, eng_opts, corr_families, kind, chunks = case
    for k, v in defaults.items():
        opts(k, v)
    iq, raw, grid, _ = cr.scene(W, 4, N, 3, seed=300 + N + W)
    if D == 1:
        grid = grid[2:]                                   # one hypothesis, nu = 0.5 / N
        kind = {"one": "per"}.get(kind, kind)             # (a single hypothesis never takes the one-launch path)
    assert np.all(grid[-1:] != 0.0)
    pairs = cr.CROSS_PAIRS
    with _engine(xc, 4, N, W, eng_opts) as eng:
        per_d = []
        for nu in grid:
            x = iq.copy()
            x[:, 2:] = cr.rot_mul(iq[:, 2:], cr.libm_phasor(nu, N))
            per_d.append(eng.correlate(x, pairs))
            assert set(_launches(eng)) == corr_families, _launches(eng)
        li, lf, pk = (np.stack([r[k] for r in per_d], axis=-1) for k in range(3))
        dop = cr.first_max(pk)
        want = (dop, cr.take(li, dop), cr.take(lf, dop), cr.take(pk, dop))
        if D == 3:
            assert len(set(dop.ravel().tolist())) > 1       # more than one hypothesis wins somewhere
        for x in (iq, raw):
            got = eng.caf(x, grid, pairs)
            assert _launches(eng) == _expected(kind, D, chunks), _launches(eng)
            _assert_same(got, want, "caf against correlate() of the host-rotated windows")


# ---- 4. ties between hypotheses -----------------------------------------------------------------------------------------
# (id, scene, engine options, kind, chunks): the four situations in which a selection kernel runs
SELECT = [
    ("N=256", "seam256", (), "small", 1),
    ("N=8192", "seam8192", (), "four", 1),
    ("N=4096 one launch", "one3", (), "one", 1),
    ("N=4096 chunked", "chunked", (("chunk_windows", 8),), "per", 3),
]


@pytest.mark.parametrize("case", SELECT, ids=[c[0] for c in SELECT])
def test_ties_between_hypotheses_keep_the_lowest_index(xc, case):
    """[a, b, a, b, a] repeats its peaks exactly, so strict > must answer as for [a, b]: dop_idx 0 or 1 only, all four arrays
    bit for bit.  All-zero windows tie at 0 in every hypothesis: hypothesis 0, the plain call's lag -(N - 1), peak 0."""
    _, name, eng_opts, kind, chunks = case
    iq, raw, grid = _scene(name)
    W, B, N = iq.shape
    a, b = grid[len(grid) // 2 + 1], grid[len(grid) // 2]
    with _engine(xc, B, N, W, eng_opts) as eng:
        for x in (iq, raw):
            two = eng.caf(x, [a, b])
            five = eng.caf(x, [a, b, a, b, a])
            assert _launches(eng) == _expected(kind, 5, chunks), _launches(eng)
            assert set(two[0].ravel().tolist()) == {0, 1}     # both win somewhere: a tie moved to a later d would show for each
            assert set(five[0].ravel().tolist()) <= {0, 1}, sorted(set(five[0].ravel().tolist()))
            _assert_same(five, two, "[a, b, a, b, a] against [a, b]")
        zero = np.zeros((W, B, N), np.complex64)
        dop, li, lf, pk = eng.caf(zero, grid[:3])
        assert _launches(eng) == _expected(kind, 3, chunks), _launches(eng)
        assert not dop.any() and np.all(li == -(N - 1)) and not lf.any() and not pk.any()
        assert np.array_equal(li, eng.correlate(zero)[0])


# ---- 5. doors -------------------------------------------------------------------------------------------------------------
# (N, B, W, engine options, kind, chunks).  (8, 12, chunk 8): a partial last chunk; (8, 20, chunk 16): 448 output slots in the
# first chunk, so k_caf_select's second block is partial, and a second chunk that starts at slot 448
DOORS = [
    (4096, 3, 5, (), "one", 1),
    (4096, 8, 12, (("chunk_windows", 8),), "per", 2),
    (4096, 8, 20, (("chunk_windows", 16),), "per", 2),
    (1024, 3, 5, (), "small", 1),
    (8192, 3, 2, (), "four", 1),
]
GUARD = 64


def _guarded(torch, dev, n):
    return [torch.full((n + GUARD,), -77, dtype=torch.int32, device=dev), torch.full((n + GUARD,), -77, dtype=torch.int32, device=dev),
            torch.full((n + GUARD,), -77.0, dtype=torch.float32, device=dev), torch.full((n + GUARD,), -77.0, dtype=torch.float32, device=dev)]


@pytest.mark.parametrize("door", DOORS, ids=["N=%d B=%d W=%d" % d[:3] for d in DOORS])
def test_device_pointers_and_mixed_flags(xc, door):
    """XcorrEngine.caf_device (RMX_IN_DEVICE | RMX_OUT_DEVICE) and the raw ABI with either flag alone: the host call's
    arrays bit for bit, exactly [W][P] elements written and the guard tail behind them untouched."""
    import torch
    N, B, W, eng_opts, kind, chunks = door
    D = 3
    iq, raw, grid, _ = cr.scene(W, B, N, D, seed=500 + N + B + W)
    P = B * (B - 1) // 2
    n = W * P
    dev = torch.device("cuda", 0)
    lib = xc.load_library()
    with _engine(xc, B, N, W, eng_opts) as eng:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        for u8 in (False, True):
            x = raw if u8 else iq
            host = eng.caf(x, grid)
            assert _launches(eng) == _expected(kind, D, chunks), _launches(eng)
            assert len(set(host[0].ravel().tolist())) > 1
            x_d = torch.from_numpy(np.ascontiguousarray(x) if u8 else np.ascontiguousarray(x).view(np.float32).reshape(W, B, N, 2)).to(dev)
            # both flags, through the binding
            o = _guarded(torch, dev, n)
            eng.caf_device(x_d.data_ptr(), W, grid, *(t.data_ptr() for t in o), u8=u8)
            eng.synchronize()
            assert _launches(eng) == _expected(kind, D, chunks), _launches(eng)
            out = [t.cpu().numpy() for t in o]
            _assert_same([a[:n].reshape(W, P) for a in out], host, "caf_device")
            assert all(np.all(a[n:] == -77) for a in out), "caf_device wrote past [W][P]"
            # one flag each, through the raw ABI
            gp = np.ascontiguousarray(grid, np.float64)
            for flags in (xc.RMX_IN_DEVICE, xc.RMX_OUT_DEVICE):
                in_ptr = C.c_void_p(x_d.data_ptr()) if flags & xc.RMX_IN_DEVICE else x.ctypes.data_as(C.c_void_p)
                if flags & xc.RMX_OUT_DEVICE:
                    o = _guarded(torch, dev, n)
                    ptrs = [C.c_void_p(t.data_ptr()) for t in o]
                else:
                    o = [np.full(n + GUARD, -77, np.int32), np.full(n + GUARD, -77, np.int32), np.full(n + GUARD, -77, np.float32),
                         np.full(n + GUARD, -77, np.float32)]
                    ptrs = [a.ctypes.data_as(C.c_void_p) for a in o]
                rc = lib.rmx_caf_batch(eng._ctx, in_ptr, W, None, P, gp.ctypes.data_as(C.c_void_p), D, *ptrs,
                                       flags | (xc.RMX_IN_U8 if u8 else 0))
                assert rc == 0, (flags, lib.rmx_last_error(eng._ctx))
                assert lib.rmx_synchronize(eng._ctx) == 0
                out = [t.cpu().numpy() if flags & xc.RMX_OUT_DEVICE else t for t in o]
                _assert_same([a[:n].reshape(W, P) for a in out], host, "flags = %d" % flags)
                assert all(np.all(a[n:] == -77) for a in out), "flags = %d wrote past [W][P]" % flags


# ---- 6. state between calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["complex64", "uint8"])
@pytest.mark.parametrize("N", [4096, 1024])
def test_state_between_calls(xc, N, u8):
    """One engine through grids of the same length, shorter, longer (N = 4096: the per-hypothesis path after the
    one-launch path, over two chunks), a correlate() in between and the first grid again: each answer is, bit for bit, that
    of a fresh engine given that one call -- no stale phasor table, no undersized per-hypothesis or spectrum buffer."""
    B, WMAX = 3, 16
    iq, raw, grid9, _ = cr.scene(WMAX, B, N, 9, seed=600 + N)
    x = raw if u8 else iq
    grid_a = grid9[2:7]
    assert len(grid_a) == 5 and grid_a[2] == 0.0
    calls = [("A", grid_a, 2), ("B: as long, other values", grid_a[::-1].copy(), 2), ("correlate", None, WMAX),
             ("C: shorter", np.array([grid9[5], grid9[3]]), 2), ("D: longer, more windows", grid9, WMAX), ("A again", grid_a, 2)]
    kinds = {4096: {2: "one", WMAX: "per"}, 1024: {2: "small", WMAX: "small"}}[N]
    eng_opts = (("chunk_windows", 8),) if N == 4096 else ()

    def run(eng, grid, w):
        if grid is None:
            return eng.correlate(x[:w])
        out = eng.caf(x[:w], grid)
        assert _launches(eng) == _expected(kinds[w], len(grid), 2 if kinds[w] == "per" else 1), _launches(eng)
        return out

    with _engine(xc, B, N, WMAX, eng_opts) as eng:
        for what, grid, w in calls:
            got = run(eng, grid, w)
            with _engine(xc, B, N, WMAX, eng_opts) as fresh:
                want = run(fresh, grid, w)
            for u, v in zip(got, want):
                assert np.array_equal(u.view(np.int32), v.view(np.int32)), what
            if grid is not None and len(grid) > 2:
                assert len(set(got[0].ravel().tolist())) > 2, what      # the grid matters: several hypotheses win
    # the answers to A and B mirror each other (B is A reversed, the margins are far from a tie): a stale table would not
    with _engine(xc, B, N, WMAX, eng_opts) as eng:
        da, db = eng.caf(x[:2], grid_a)[0], eng.caf(x[:2], grid_a[::-1].copy())[0]
    assert np.array_equal(da, 4 - db)


# ---- 7. limits of n_dopplers ----------------------------------------------------------------------------------------------
def test_4096_hypotheses_are_accepted(xc):
    iq, raw, grid, at = cr.limit_scene()
    ref = cr.reference(iq, grid)
    assert ref["dop"][0, 0] == at
    with _engine(xc, 2, 256, 1) as eng:
        got = eng.caf(iq, grid)
        assert _launches(eng) == _expected("small", 4096), _launches(eng)
        _assert_same(eng.caf(raw, grid), got, "uint8 against complex64")
    _assert_parity(got, ref)


@pytest.mark.parametrize("N", [256, 4096])
def test_refused_grids_leave_the_outputs_and_the_engine_alone(xc, N):
    """n_dopplers = 0 and 4097 and a NULL grid: RMX_E_INVAL, a message that names the argument, the four output arrays as
    they were, and the next call answered as before."""
    B, W = 3, 2
    iq, _, grid, _ = cr.scene(W, B, N, 3, seed=700 + N)
    long_grid = np.ascontiguousarray((np.arange(4097) - 2048) / 8192.0)
    lib = xc.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    with _engine(xc, B, N, W) as eng:
        before = eng.caf(iq, grid)
        for n_dop, gp, word in ((0, vp(long_grid), b"n_dopplers"), (4097, vp(long_grid), b"n_dopplers"), (-1, vp(long_grid), b"n_dopplers"),
                                (3, None, b"NULL")):
            o = [np.full((W, 3), -77, np.int32), np.full((W, 3), -77, np.int32), np.full((W, 3), -77, np.float32),
                 np.full((W, 3), -77, np.float32)]
            rc = lib.rmx_caf_batch(eng._ctx, vp(iq), W, None, 3, gp, n_dop, *map(vp, o), 0)
            assert rc == -1, (n_dop, rc)                      # RMX_E_INVAL
            assert word in lib.rmx_last_error(eng._ctx), (n_dop, lib.rmx_last_error(eng._ctx))
            assert all(np.all(a == -77) for a in o), n_dop
            _assert_same(eng.caf(iq, grid), before, "the call after a refusal")
        with pytest.raises(xc.RmxError) as e:
            eng.caf(iq, long_grid)
        assert e.value.code == -1 and "n_dopplers" in str(e.value)
        # 4096 of them pass the same check (the answer itself: test_4096_hypotheses_are_accepted)
        if N == 256:
            assert eng.caf(iq, long_grid[:4096])[0].shape == (W, 3)


# ---- 8. the fall-back thresholds of the one-launch path -------------------------------------------------------------------
def test_one_launch_path_up_to_the_scratch_cap_and_one_above(xc):
    """rmx_caf_batch takes all hypotheses in one launch while their de-rotated spectra fit 1 GiB:
        n_dopplers * n_windows * B * (8 * kThreads) * sizeof(float4) <= 2^30,   kThreads = 512 (fft_r16.hpp),
    i.e. 64 KiB a spectrum, 16384 spectra.  B = 4, W = 4: D = 16384 / 16 = 1024 is the last grid in one launch, 1025 the
    first that goes hypothesis by hypothesis.  The grid is [a, b] tiled, so the answer is that of [a, b], bit for bit."""
    B, W, N = 4, 4, 4096
    spectrum_bytes = 8 * 512 * 16
    d_cap = (1 << 30) // (spectrum_bytes * W * B)
    assert d_cap == 1024 and d_cap * W * B * spectrum_bytes == 1 << 30
    iq, raw, grid, _ = cr.scene(W, B, N, 3, seed=800)
    a, b = grid[2], grid[1]
    with _engine(xc, B, N, W) as eng:
        two = eng.caf(iq, [a, b])
        assert _launches(eng) == _expected("one", 2) and set(two[0].ravel().tolist()) == {0, 1}
        for D, kind in ((d_cap, "one"), (d_cap + 1, "per")):
            tiled = np.resize(np.array([a, b]), D)
            for x in (iq, raw):
                got = eng.caf(x, tiled)
                assert _launches(eng) == _expected(kind, D), (D, _launches(eng))
                _assert_same(got, two, "%d hypotheses against two" % D)


def test_one_launch_path_up_to_one_chunk_and_one_above(xc):
    """n_windows == chunk_windows is still one launch; one chunk more runs hypothesis by hypothesis, chunk by chunk"""
    B, N, D = 4, 4096, 4
    iq, raw, grid, _ = cr.scene(16, B, N, 3, seed=801)
    a, b = grid[2], grid[1]
    tiled = np.resize(np.array([a, b]), D)
    with _engine(xc, B, N, 16, (("chunk_windows", 8),)) as eng:
        for W, kind, chunks in ((8, "one", 1), (16, "per", 2)):
            for x in (iq, raw):
                two = eng.caf(x[:W], [a, b])
                assert _launches(eng) == _expected(kind, 2, chunks), (W, _launches(eng))
                assert set(two[0].ravel().tolist()) == {0, 1}
                got = eng.caf(x[:W], tiled)
                assert _launches(eng) == _expected(kind, D, chunks), (W, _launches(eng))
                _assert_same(got, two, "W = %d" % W)
