"""rmx_caf_batch_integrated, the Doppler search integrated over groups of K windows, on the GPU: the smallest shape that
reaches each integrating body on every route against the float restatement (tests/caf_integrated_ref.py) at the bars of
tests/test_gpu_caf_quality.py, with the launch counts of each route; integrate = 1 against rmx_caf_batch_quality in bits and
launches; the whole call bit for bit against the engine's own correlate(integrate, refine, quality) on host-rotated windows;
and the caller's memory, every refusal in its order, a dead receiver and two identical calls through the raw ABI.

N = 4096 in chunks: the option chunk_windows is a multiple of 8 and at least 8, so the chunked shapes are W = 16 under
chunks of 8 (K = 2) and W = 18 under the same 8 with K = 3, which rounds down to whole groups -- chunks of 6."""
import ctypes as C

import numpy as np
import pytest

import caf_integrated_ref as ci
import caf_ref as cr
import caller_memory_ref as cm
from test_gpu_caf import _engine, _expected, _launches
from test_gpu_caf_quality import OUT_NAMES, _assert_parity, _assert_same, _slab, _take, _with_tail

pytestmark = pytest.mark.gpu
U = ci.REFINE


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


# ---- 1. every route: parity, identities, launch counts ------------------------------------------------------------------------
# (id, scene, kind, chunks, default options, engine options, row family with the default list / with the custom one)
ROUTES = [
    ("small N=16 K=2", "n16k2", "small", 1, {}, (), None, None),
    ("small N=16 K=3", "n16k3", "small", 1, {}, (), None, None),
    ("small N=256 K=2", "n256k2", "small", 1, {}, (), None, None),
    ("small N=256 K=3", "n256k3", "small", 1, {}, (), None, None),
    ("four-step N=8192 B=4", "n8192b4", "four", 1, {}, (), "g_rows_inv", "g_rows_inv"),
    ("four-step N=8192 B=6 anchor", "n8192b6", "four", 1, {}, (), "g_rows_anchor", "g_rows_inv"),
    ("one launch resident=0", "one4", "one", 1, {}, (("resident", 0),), None, None),
    ("one launch resident=1", "one4", "one", 1, {}, (("resident", 1),), None, None),
    ("N=4096 K=2 chunks 8+8", "chunk16k2", "per", 2, {}, (("chunk_windows", 8),), None, None),
    ("N=4096 K=3 chunks 8->6+6+6", "chunk18k3", "per", 3, {}, (("chunk_windows", 8),), None, None),
    ("small N=256 chunks 2+2+2", "n256k2", "small", 3, {"gen_chunk": 2}, (), None, None),
    ("four-step N=8192 chunks 2+2+2", "seam8192", "four", 3, {"gen_chunk": 2}, (), "g_rows_inv", "g_rows_inv"),
    ("one group small K=W", "group256", "small", 1, {}, (), None, None),
    ("one group N=4096 K=W", "group4096", "one", 1, {}, (), None, None),
]


@pytest.mark.parametrize("custom", [False, True], ids=["default all", "custom phat"])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_against_the_reference(xc, opts, route, custom):
    """The default pair list under per-group bounds + per-window bands + PHAT, the custom one under PHAT.  The launches are
    the search's own, chunk by chunk of whole groups; with refine = 0 and quality off nothing follows the selection; quality
    alone leaves the five other arrays alone; refine moves neither dop_idx nor dop_frac nor quality; uint8 equals
    complex64; parity with refine = 0 and refine = 8; a chunked call equals a one-chunk call."""
    _, name, kind, chunks, defaults, eng_opts, rows_def, rows_custom = route
    for k, v in defaults.items():
        opts(k, v)
    W, B, N, D, K, _ = ci.SCENES[name]
    iq, raw, grid, K, pairs, kw = ci.case(name, custom)
    ref = ci.case_reference(name, custom)
    rows = rows_custom if custom else rows_def
    want = _expected(kind, D, chunks, rows)
    with _engine(xc, B, N, W, eng_opts) as eng:
        base = eng.caf(iq, grid, pairs, fine=True, integrate=K, **kw)
        assert _launches(eng) == want, _launches(eng)
        assert all(a.shape == (W // K, len(ref["dop"][0])) for a in base)
        q0 = eng.caf(iq, grid, pairs, fine=True, quality=True, integrate=K, **kw)
        assert _launches(eng) == _with_tail(want, kind, D, chunks, True, False), _launches(eng)
        _assert_same(q0[:5], base, "quality=True: the five other arrays")
        _assert_parity(q0, ref, N, 0)
        full = eng.caf(iq, grid, pairs, fine=True, refine=U, quality=True, integrate=K, **kw)
        assert _launches(eng) == _with_tail(want, kind, D, chunks, True, True), _launches(eng)
        _assert_same(full[:2], base[:2], "refine: dop_idx and dop_frac")
        _assert_same(full[5:], q0[5:], "refine: quality is computed with the coarse peak")
        _assert_parity(full, ref, N, U)
        assert np.all(np.abs(full[2] - base[2]) <= 1)
        dfb = np.abs(base[1].astype(np.float64) - ref["dop_frac"])
        print("worst dop_frac error %.3e" % dfb.max())
        assert np.all((dfb <= 1e-5) | (dfb <= ref["dop_frac_bound"])), "dop_frac outside the rule: %.3e" % dfb.max()
        only = eng.caf(iq, grid, pairs, refine=U, integrate=K, **kw)
        assert _launches(eng) == _with_tail(want, kind, D, chunks, False, True), _launches(eng)
        _assert_same(only, (full[0],) + full[2:5], "refine without quality and without dop_frac")
        full8 = eng.caf(raw, grid, pairs, fine=True, refine=U, quality=True, integrate=K, **kw)
        _assert_same(full8, full, "uint8 against complex64")
    if chunks > 1:   # a chunked call equals a one-chunk call (N = 4096: the one-launch path, bit for bit)
        xc.clear_default_options()
        one_kind = "one" if kind == "per" else kind
        with _engine(xc, B, N, W, ()) as whole:
            one = whole.caf(iq, grid, pairs, fine=True, refine=U, quality=True, integrate=K, **kw)
            assert _launches(whole) == _with_tail(_expected(one_kind, D, 1, rows), one_kind, D, 1, True, True), _launches(whole)
            _assert_same(full, one, "chunked against one chunk")


@pytest.mark.parametrize("case", [("small", "n256k2", ()), ("four-step", "n8192b4", ()), ("one launch", "one4", ()),
                                  ("N=4096 chunked", "chunk16k2", (("chunk_windows", 8),))], ids=lambda c: c[0])
def test_one_window_per_group_is_the_quality_entry(xc, case):
    """integrate = 1 IS caf(refine, quality): the same launches, the same bits, all six arrays"""
    _, name, eng_opts = case
    W, B, N, D, _, _ = ci.SCENES[name]
    iq, raw, grid, _, pairs, _ = ci.case(name, True)
    with _engine(xc, B, N, W, eng_opts) as eng:
        for more in (dict(refine=U, quality=True), dict(quality=True), dict()):
            a = eng.caf(iq, grid, pairs, fine=True, whiten=True, **more)
            la = _launches(eng)
            b = eng.caf(iq, grid, pairs, fine=True, whiten=True, integrate=1, **more)
            assert _launches(eng) == la
            _assert_same(a, b, "integrate = 1 against the call without it")
        # ... through the C entry itself (the binding sends K = 1 to rmx_caf_batch_quality)
        P = len(pairs)
        outs = [np.zeros((W, P), np.int32), np.zeros((W, P), np.float32), np.zeros((W, P), np.int32), np.zeros((W, P), np.float32),
                np.zeros((W, P), np.float32), np.zeros((W, P, 4), np.float32)]
        vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
        x = np.ascontiguousarray(iq)
        gp = np.ascontiguousarray(grid, np.float64)
        pl = np.ascontiguousarray(pairs, np.int32)
        rc = xc.load_library().rmx_caf_batch_integrated(eng._ctx, vp(x), W, vp(pl), P, vp(gp), len(gp), 1, None, 0, 1, None, 0, U,
                                                        *[vp(o) for o in outs], 0)
        assert rc == 0, eng._lib.rmx_last_error(eng._ctx)
        lb = _launches(eng)
        want = eng.caf(iq, grid, pairs, fine=True, whiten=True, refine=U, quality=True)
        assert _launches(eng) == lb
        _assert_same(outs, want, "rmx_caf_batch_integrated(integrate = 1) against rmx_caf_batch_quality")


# ---- 2. bit for bit against correlate() on host-rotated windows -----------------------------------------------------------------
# (id, N, W, K, engine options)
EXACT = [
    ("N=256", 256, 6, 2, ()),
    ("N=8192", 8192, 4, 2, ()),
    ("N=4096 one launch", 4096, 4, 2, ()),
    ("N=4096 chunked", 4096, 16, 2, (("chunk_windows", 8),)),
]


@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_bit_for_bit_against_correlate_on_host_rotated_windows(xc, case):
    """Buoys 2 and 3 rotated on the host, CROSS_PAIRS: under PHAT and under band + bounds, caf(integrate=K, refine=u,
    quality=True) IS correlate(host-rotated, integrate=K, refine=u, quality=True, the same request) taken at the coarse
    first maximum, on all four outputs, for u = 0 and u = 8: the integrating pair kernels with the second operand set,
    k_quality<CafWinner> and k_refine<CafWinner> over K windows are the plain bodies on the same spectra."""
    _, N, W, K, eng_opts = case
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
                    per[u].append(eng.correlate(x, pairs, integrate=K, refine=u, quality=True, **kw))
            coarse = [np.stack([r[k] for r in per[0]], axis=-1) for k in range(4)]
            dop = cr.first_max(coarse[2])
            assert dop.shape == (W // K, len(pairs)) and len(set(dop.ravel().tolist())) > 1
            for u in per:
                want = [_take(np.stack([r[k] for r in per[u]], axis=-1), dop) for k in range(4)]
                for x in (iq, raw):
                    got = eng.caf(x, grid, pairs, refine=u, quality=True, integrate=K, **kw)
                    assert np.array_equal(got[0], dop), rid
                    _assert_same(got[1:], want, "%s, refine=%d: caf against correlate() of the host-rotated windows" % (rid, u))


# ---- 3. the caller's memory, the refusals and a dead receiver through the raw ABI ------------------------------------------
def _raw_call(xc, eng, iq_ptr, W, P, grid, ptrs, K, refine=U, weighting=1, flags=None, bounds=None, per_group=0, n_dopplers=None):
    lib = xc.load_library()
    gp = np.ascontiguousarray(grid, np.float64)
    vp = lambda p: None if not p else C.c_void_p(p)   # noqa: E731
    flags = (xc.RMX_IN_DEVICE | xc.RMX_OUT_DEVICE) if flags is None else flags
    return lib.rmx_caf_batch_integrated(eng._ctx, vp(iq_ptr), W, None, P, gp.ctypes.data_as(C.c_void_p), len(gp) if n_dopplers is None else n_dopplers,
                                        K, None, 0, weighting, None if bounds is None else bounds.ctypes.data_as(C.c_void_p), per_group,
                                        refine, vp(ptrs["dop_idx"]), vp(ptrs["dop_frac"]), vp(ptrs["lag_int"]), vp(ptrs["lag_frac"]),
                                        vp(ptrs["peak"]), vp(ptrs["quality"]), flags)


def _arrays(slots):
    return [("lag_int", np.int32, slots), ("lag_frac", np.float32, slots), ("peak", np.float32, slots), ("quality", np.float32, 4 * slots),
            ("dop_idx", np.int32, slots), ("dop_frac", np.float32, slots)]


MEMORY = [("one launch", "one4", {}, ()), ("small chunks 2+2+2", "n256k2", {"gen_chunk": 2}, ()),
          ("four-step", "n8192b4", {}, ()), ("N=4096 chunks 8+8", "chunk16k2", {}, (("chunk_windows", 8),))]


@pytest.mark.parametrize("placement", cm.PLACEMENTS)
@pytest.mark.parametrize("case", MEMORY, ids=[c[0] for c in MEMORY])
def test_device_pointers_between_guards(xc, opts, case, placement):
    """RMX_OUT_DEVICE with every output -- exactly G * P elements, quality 4 G P -- between two guards: the six arrays are
    those of the host door bit for bit, every element is written, no guard word and no byte of the input changes; a second
    identical call gives identical bits."""
    import torch
    _, name, defaults, eng_opts = case
    for k, v in defaults.items():
        opts(k, v)
    W, B, N, D, K, _ = ci.SCENES[name]
    iq, raw, grid, _, _, _ = ci.case(name, False)
    P = B * (B - 1) // 2
    G = W // K
    with _engine(xc, B, N, W, eng_opts) as eng:
        want = eng.caf(iq, grid, whiten=True, fine=True, refine=U, quality=True, integrate=K)
        lay, before, t = _slab(torch, _arrays(G * P), placement)
        in_lay = cm.layout([("iq", np.complex64, iq.size)], placement)
        in_before = cm.fill(in_lay)
        cm.put(in_before, in_lay, "iq", iq)
        t_in = torch.from_numpy(in_before).to(torch.device("cuda", 0))
        ptrs = {n: t.data_ptr() + lay.entries[n].offset for n in OUT_NAMES}
        after = []
        for _ in range(2):
            rc = _raw_call(xc, eng, t_in.data_ptr() + in_lay.entries["iq"].offset, W, P, grid, ptrs, K)
            assert rc == 0, eng._lib.rmx_last_error(eng._ctx)
            eng.synchronize()
            after.append(t.cpu().numpy())
        bad = cm.check(before, after[0], lay, OUT_NAMES)
        assert not bad, "%d findings, the first: %s" % (len(bad), bad[:8])
        assert np.array_equal(t_in.cpu().numpy(), in_before)
        got = [cm.cut(after[0], lay, n, (G, P, 4) if n == "quality" else (G, P)) for n in OUT_NAMES]
        _assert_same(got, want, "device door against host door")
        assert np.array_equal(after[0], after[1]), "two identical calls differ"


def test_refusals_in_their_order_leave_every_output_untouched(xc, opts):
    """Every refusal of the entry in its order, each one made with every later mistake present too: the head
    (n_dopplers), integrate and the group count with their values, the batch shape, the weighting, the bounds by
    "group", dop_frac's overlap, refine, quality's overlap and alignment, then the route: a K that no chunk holds.
    Nothing is written by any of them."""
    import torch
    opts("gen_chunk", 2)
    W, B, N, D, K, _ = ci.SCENES["n256k2"]
    iq, _, grid, _, _, _ = ci.case("n256k2", False)
    P = B * (B - 1) // 2
    G = W // K
    lay, before, t = _slab(torch, _arrays(G * P), "aligned")
    t_in = torch.from_numpy(np.ascontiguousarray(iq).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))
    ptrs = {n: t.data_ptr() + lay.entries[n].offset for n in OUT_NAMES}
    bad_lb = np.zeros((G, P, 2), np.int32)
    bad_lb[G - 1, P - 1] = (5, 4)
    with _engine(xc, B, N, W) as eng:
        def refused(text, code=-1, **kw):
            moved = dict(ptrs, **{k: v for k, v in kw.items() if k in ptrs})
            rest = {k: v for k, v in kw.items() if k not in ptrs}
            rest.setdefault("K", K)
            rest.setdefault("W", W)
            w = rest.pop("W")
            rc = _raw_call(xc, eng, t_in.data_ptr(), w, P, grid, moved, **rest)
            msg = eng._lib.rmx_last_error(eng._ctx).decode()
            assert rc == code and text in msg, (rc, msg)
            eng.synchronize()
            assert np.array_equal(t.cpu().numpy(), before), "a refused call wrote: " + msg
        rest = dict(weighting=7, bounds=bad_lb, per_group=1, dop_frac=ptrs["peak"], refine=3, quality=ptrs["peak"] + 2)
        refused("n_dopplers 0 not in", n_dopplers=0, K=0, **rest)
        refused("integrate = 0:", K=0, **rest)
        refused("n_windows = 6 is not a positive multiple of integrate = 4", K=4, **rest)
        refused("n_windows 66 not in 0..max_windows=6", W=66, K=3, **rest)
        refused("unknown weighting 7", **rest)
        rest.pop("weighting")
        refused("lag_bounds of group %d, pair %d" % (G - 1, P - 1), **rest)
        rest.pop("bounds"), rest.pop("per_group")
        refused("dop_frac overlaps peak", **rest)
        rest.pop("dop_frac")
        refused("refine = 3", **rest)
        rest.pop("refine")
        for name in ("dop_idx", "dop_frac", "lag_int", "lag_frac", "peak"):
            refused("quality overlaps %s" % name, quality=ptrs[name] + 2)
        refused("%d x 4 floats" % (G * P), quality=ptrs["peak"] + 2)                  # the extents are G * P slots
        refused("quality is a device pointer 2 bytes past a multiple of 4", quality=ptrs["quality"] + 2)
        # the route: groups of 3 windows under chunks of 2 -- never a silent split
        refused("integrate = 3 windows per group is more than the largest chunk this ctx can hold, 2 windows", K=3)
    xc.clear_default_options()
    W4, K4 = 16, 16
    t_in4 = torch.zeros(W4 * 3 * 4096 * 2, dtype=torch.float32, device=torch.device("cuda", 0))
    with _engine(xc, 3, 4096, W4, (("chunk_windows", 8),)) as eng:
        rc = _raw_call(xc, eng, t_in4.data_ptr(), W4, 3, grid, ptrs, K4)
        msg = eng._lib.rmx_last_error(eng._ctx).decode()
        assert rc == -1 and "integrate = 16 windows per group is more than the largest chunk this ctx can hold, 8 windows" in msg, (rc, msg)
        eng.synchronize()
        assert np.array_equal(t.cpu().numpy(), before), "a refused call wrote: " + msg


@pytest.mark.parametrize("case", [("N=256", 256, ()), ("N=4096 one launch", 4096, ()), ("N=8192", 8192, ())], ids=lambda c: c[0])
def test_a_dead_receiver_gives_four_zeros(xc, case):
    """buoy 1 all zeros: its pairs' integrated peak is 0 under every hypothesis -- hypothesis 0 wins --, the four figures
    are 0, nothing is NaN, the lags are finite, and the live pair keeps its values"""
    _, N, eng_opts = case
    iq, _, grid, _ = cr.scene(4, 3, N, 3, seed=77 + N)
    x = iq.copy()
    x[:, 1] = 0
    with _engine(xc, 3, N, 4, eng_opts) as eng:
        for kw in ({}, dict(whiten=True)):
            dop, li, lf, pk, qual = eng.caf(x, grid, refine=U, quality=True, integrate=2, **kw)
            assert qual.shape == (2, 3, 4)
            assert np.all(np.isfinite(qual)) and np.all(np.isfinite(lf)) and np.all(np.isfinite(pk)) and np.all(np.abs(li) < N)
            for q in (0, 2):   # pairs (0, 1) and (1, 2)
                assert not qual[:, q].any() and not pk[:, q].any() and not dop[:, q].any()
            assert np.all(qual[:, 1] > 0) and np.all(pk[:, 1] > 0)
