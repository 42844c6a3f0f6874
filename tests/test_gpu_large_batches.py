"""Every route at batches whose input or scratch passes 2^31 / 2^32 bytes, and whose grids pass 65 535 rows.

The other sweeps run a few windows to a few hundred MiB; here a byte offset, an element index or a grid row leaves the range
those shapes use.  tests/large_batch_ref.py has the method: a batch is T base windows repeated (window w = base window
w % T, T = 7 or 5), built on the device by index_select; the expected value of every slot is the float64 reference of its
base window; every slot of every batch is compared (no base window has a slot with a margin under 1e-5:
tests/test_large_batch_ref_cpu.py, which also shows that each of three narrow address rules would fail these comparisons).

Bars: the plain and bounded calls by test_gpu_far_lags._assert_bars against far_lag_ref.ref64_batch (integer lag equal on
every slot, |lag_frac - ref| <= 1e-5 absolute or the flat-peak bound, peak 1e-5 relative); the weighted, integrated,
refined, qualified and Doppler-search calls by the rule of their own GPU file against its reference.  A bounded call's
windows contain the reference's peak with room on both sides, so its expected values are the unbounded reference's.

Every case asserts the kernel families that ran and their launch counts (option timing = 1), states its device footprint,
and frees its tensors and its engine before the next one.  A failure names the windows around the byte boundary."""
import gc

import numpy as np
import pytest

import caf_ref as cr
import far_lag_ref as F
import integrated_ref as ir
import large_batch_ref as lb
import quality_ref as qr
import refined_ref as rr
import weighted_ref as wr
from oracle import xcorr_ref as orc

pytestmark = pytest.mark.gpu

FOUR = {"g_cols_fwd", "g_cols_inv", "g_final"}
TWO_PASS = FOUR | {"g_rows_fwd", "g_rows_inv"}
ANCHOR = FOUR | {"g_rows_fwd", "g_rows_anchor"}
RFUSED = FOUR | {"g_rows_fused"}
KWIN = "k_win|k_pair"
MAX_GRID_ROWS = 65535       # host_plan.hpp: kMaxGridY
MAX_CHUNK = 4096            # host_plan.hpp: kGenericMaxChunk


@pytest.fixture(scope="module")
def xc():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    assert xcorr.device_count() > 0, "no MI355X visible"
    return xcorr


@pytest.fixture
def opts(xc):
    xc.clear_default_options()
    yield xc.set_default_option
    xc.clear_default_options()


@pytest.fixture(autouse=True)
def _free_device_memory():
    """each case's tensors and engine are gone before the next case allocates"""
    yield
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


_REFS = {}


def _ref(key, make):
    """a reference over the base windows, computed once per module and never changed"""
    if key not in _REFS:
        ref = make()
        for a in (ref.values() if isinstance(ref, dict) else ref if isinstance(ref, tuple) else (ref,)):
            np.asarray(a).setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def _upload(base, W):
    """the batch on the device: the base windows (complex64 [T][B][N] or uint8 [T][B][2N]) uploaded, then window w = base
    window w % T by index_select"""
    import torch
    dev = torch.device("cuda", 0)
    host = np.array(base)   # (a writable copy of the shared base windows)
    t = torch.from_numpy(host.view(np.float32) if host.dtype == np.complex64 else host).to(dev)
    big = t.index_select(0, torch.arange(W, device=dev) % len(base))
    torch.cuda.synchronize()
    assert big.is_contiguous() and big.shape[0] == W
    return big


def _outputs(rows, P, quality=False, dop=False):
    import torch
    dev = torch.device("cuda", 0)
    o = {"lag_int": torch.zeros((rows, P), dtype=torch.int32, device=dev), "lag_frac": torch.zeros((rows, P), dtype=torch.float32, device=dev),
         "peak": torch.zeros((rows, P), dtype=torch.float32, device=dev)}
    if quality:
        o["quality"] = torch.zeros((rows, P, 4), dtype=torch.float32, device=dev)
    if dop:
        o["dop"] = torch.zeros((rows, P), dtype=torch.int32, device=dev)
    return o


def _correlate(eng, big, W, P, u8=False, quality=False, **req):
    """one device-door call -> ((lag_int, lag_frac, peak[, quality]) as numpy, {family: launches})"""
    rows = W // req.get("integrate", 1)
    o = _outputs(rows, P, quality)
    eng.correlate_device(big.data_ptr(), W, o["lag_int"].data_ptr(), o["lag_frac"].data_ptr(), o["peak"].data_ptr(), u8=u8,
                         quality_ptr=o["quality"].data_ptr() if quality else 0, **req)
    eng.synchronize()
    tk = {k: v["launches"] for k, v in eng.last_timing_by_kernel().items()}
    print("launches", tk, "scratch %.2f GiB" % (eng.scratch_bytes() / 2.0 ** 30))
    return tuple(o[n].cpu().numpy() for n in ("lag_int", "lag_frac", "peak") + (("quality",) if quality else ())), tk


def _named(what, plan_text, li, ri, rule):
    """runs the comparison `rule`; a failure also names the rows whose integer lag is wrong, and where the boundary lies"""
    li, ri = np.asarray(li), np.asarray(ri)
    rows = np.unique(np.nonzero(li != ri)[0])
    print("%s: %d rows x %d slots compared, %d rows with a wrong integer lag" % (what, li.shape[0], li[0].size, len(rows)))
    try:
        rule()
    except AssertionError as e:
        raise AssertionError("%s: %s\nrows with a wrong integer lag: %d, first %s, last %s\n%s" % (
            what, e, len(rows), rows[:8].tolist(), rows[-8:].tolist(), plan_text)) from e


def _bars(got, ref, base, pairs, T, what, plan_text):
    """the plain and bounded rule (test_gpu_far_lags._assert_bars) on every slot of the batch"""
    import test_gpu_far_lags as tf
    rows, P = got[0].shape
    want = lb.expand(ref[:3], rows, T)
    pairs = np.asarray(pairs).reshape(-1, 2)
    xs = lambda k: (base[(k // P) % T, pairs[k % P, 0]], base[(k // P) % T, pairs[k % P, 1]])   # noqa: E731
    _named(what, plan_text, got[0], want[0], lambda: tf._assert_bars(got, want, xs, what))


def _bounds_around(ref, N, W, T):
    """per-window lag windows [W][P][2] that hold the reference's peak with 100 lags below it and 50 above"""
    ri = np.asarray(ref[0])
    b = np.stack([np.maximum(ri - 100, -(N - 1)), np.minimum(ri + 50, N - 1)], axis=-1).astype(np.int32)
    assert np.all(b[..., 0] < ri) and np.all(ri < b[..., 1])
    return np.ascontiguousarray(b[lb.window_map(W, T)])


def _ref64(c, pairs=None):
    iq, raw, _ = lb.base_scene(c["N"], c["B"], c["T"])
    pl = orc.pair_list(c["B"]) if pairs is None else np.asarray(pairs, np.int32)
    ref = _ref(("ref64", c["N"], c["B"], c["T"], pl.tobytes()), lambda: F.ref64_batch(iq, pl))
    assert ref[3].min() > 1e-5 and lb.distinct(ref[0])
    return iq, raw, pl, ref


def _plan_text(c):
    return "%s, %s: %s" % (c["id"], c["buffer"], lb.describe(lb.case_plan(c)))


# ---- input past 2^32 bytes: the whole-window kernels --------------------------------------------------------------------
# (case, default options, engine options, timing family, launches): one persistent grid per launch
WHOLE = [
    # k_win / k_win_lb: a chunk holds at most 16384 windows of 8 buoys; 16376 puts byte 2^32 (window 16384) INSIDE the
    # second launch (windows 16376 ... 16447) and byte 2^31 inside the first
    ("I1", {}, {"small4096": 0, "chunk_windows": 16376}, KWIN, 2),
    # k_win<U8>: windows 32768 (sample index 2^31) and 65536 inside the third and fifth launch
    ("I2", {}, {"small4096": 0, "chunk_windows": 16376}, KWIN, 5),
    ("I3", {"wscr": 2}, {}, "g_win_*", 1),                                   # k_win8kl
    ("I5-g_win_fused", {"wscr": 0}, {}, "g_win_*", 1),
    ("I5-g_win_scr", {"wscr": 2, "wfused": 0}, {}, "g_win_*", 1),
    ("I5-g_win_scr14", {"wscr": 2, "kwin8k": 0}, {}, "g_win_*", 1),
    ("I5-g_win_eo15", {"wscr": 2, "kwin16k": 0}, {}, "g_win_*", 1),
]


@pytest.mark.parametrize("cid,dflt,eopts,family,launches", WHOLE, ids=[w[0] for w in WHOLE])
def test_input_past_4gib_through_the_whole_window_kernels(xc, opts, cid, dflt, eopts, family, launches):
    """I1, I2, I3, I5: 4.0 ... 4.1 GiB of input on the device, outputs of at most 22 MiB, scratch under 0.6 GiB: under 5 GiB.
    Plain, and (where the kernel has a bounded instantiation: k_win_lb, k_win8kl) per-window bounds."""
    c = lb.CASES[cid]
    N, B, W, T, P = c["N"], c["B"], c["W"], c["T"], c["P"]
    u8 = c["elem"] == 1
    iq, raw, pl, ref = _ref64(c)
    for k, v in dflt.items():
        opts(k, v)
    big = _upload(raw if u8 else iq, W)
    assert big.numel() * big.element_size() == W * c["unit_bytes"] > 1 << 32
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        for k, v in eopts.items():
            eng.set_option(k, v)
        got, tk = _correlate(eng, big, W, P, u8=u8)
        assert tk == {family: launches}, tk
        _bars(got, ref, iq, pl, T, cid + " plain", _plan_text(c))
        if cid in ("I1", "I3"):
            got, tk = _correlate(eng, big, W, P, u8=u8, lag_bounds=_bounds_around(ref, N, W, T))
            assert tk == {family: launches}, tk
            _bars(got, ref, iq, pl, T, cid + " per-window bounds", _plan_text(c))


def test_input_past_4gib_through_k16(xc, opts):
    """I4: N 16384, 8 buoys, 4160 windows (4.06 GiB of input, 0.5 GiB of scratch): k16_fwd + k16_pairs, which take the batch
    in chunks of the scratch's window slots -- one forward and one pair launch per chunk, the last chunks wholly beyond 2^32."""
    c = lb.CASES["I4"]
    iq, raw, pl, ref = _ref64(c)
    opts("kwin16k", 2)
    big = _upload(iq, c["W"])
    with xc.XcorrEngine(c["B"], c["N"], c["W"]) as eng:
        eng.set_option("timing", 1)
        got, tk = _correlate(eng, big, c["W"], c["P"])
        assert set(tk) == {"k16_fwd", "k16_pairs"} and tk["k16_fwd"] == tk["k16_pairs"] <= -(-c["W"] // 256), tk
        _bars(got, ref, iq, pl, c["T"], "I4 plain", _plan_text(c))
        got, tk = _correlate(eng, big, c["W"], c["P"], lag_bounds=_bounds_around(ref, c["N"], c["W"], c["T"]))
        assert set(tk) == {"k16_fwd", "k16_pairs"}, tk
        _bars(got, ref, iq, pl, c["T"], "I4 per-window bounds", _plan_text(c))


def test_input_past_4gib_through_the_small_kernels_bounded(xc, opts):
    """I6: N 1024, 16 buoys, 32 832 windows, per-window bounds: g_fwd_small + g_pair_small<LagBounds> in nine chunks of 4096
    windows, first_item of the last chunks past 2^32 bytes.  4.01 GiB of input, 1 GiB of spectra, 47 MiB of outputs."""
    c = lb.CASES["I6"]
    iq, raw, pl, ref = _ref64(c)
    big = _upload(iq, c["W"])
    chunks = -(-c["W"] // MAX_CHUNK)
    with xc.XcorrEngine(c["B"], c["N"], c["W"]) as eng:
        eng.set_option("timing", 1)
        got, tk = _correlate(eng, big, c["W"], c["P"], lag_bounds=_bounds_around(ref, c["N"], c["W"], c["T"]))
        assert tk == {"g_fwd_small": chunks, "g_pair_small": chunks} and chunks == 9, tk
        _bars(got, ref, iq, pl, c["T"], "I6 per-window bounds", _plan_text(c))


def test_input_past_4gib_through_the_four_step(xc, opts):
    """I7: N 65536, 3 buoys, 2795 windows (the planner's count: window 2730 straddles byte 2^32, 2731 ... 2794 lie beyond),
    gen_chunk 256: g_cols_fwd, g_rows_fused, g_cols_inv, g_final, eleven launches each.  4.09 GiB of input, 1.5 GiB of
    spectra and products."""
    c = lb.CASES["I7"]
    iq, raw, pl, ref = _ref64(c)
    opts("gen_chunk", 256)
    opts("fused", 2)
    big = _upload(iq, c["W"])
    chunks = -(-c["W"] // 256)
    with xc.XcorrEngine(c["B"], c["N"], c["W"]) as eng:
        eng.set_option("timing", 1)
        got, tk = _correlate(eng, big, c["W"], c["P"])
        assert tk == {k: chunks for k in RFUSED} and chunks == 11, tk
        _bars(got, ref, iq, pl, c["T"], "I7 plain", _plan_text(c))


def test_host_input_past_4gib_through_the_pipelined_copy(xc, opts):
    """I8: I1's shape through the host door: the copy is cut into sub-chunks of 512 windows at offsets past 2^32, each
    followed by its k_win launch (33 of them).  4.02 GiB in host memory and as much in the ctx's device copy."""
    c = lb.CASES["I8"]
    iq, raw, pl, ref = _ref64(c)
    host = np.ascontiguousarray(iq[lb.window_map(c["W"], c["T"])])
    assert host.nbytes > 1 << 32
    with xc.XcorrEngine(c["B"], c["N"], c["W"]) as eng:
        eng.set_option("timing", 1)
        eng.set_option("small4096", 0)
        got = eng.correlate(host)
        tk = {k: v["launches"] for k, v in eng.last_timing_by_kernel().items()}
        print("launches", tk)
        assert tk == {KWIN: -(-c["W"] // 512)}, tk
    del host
    _bars(got, ref, iq, pl, c["T"], "I8 host door", _plan_text(c))


# ---- library scratch past 2^32 bytes inside one chunk ----------------------------------------------------------------------
def test_spectrum_scratch_past_4gib_n4096(xc, opts):
    """S1: N 4096, 20 buoys, 4096 windows, fused = 0: ONE chunk whose d_spec is 5 GiB (k_fwd stores, k_pair_*, k_refine and
    k_quality read past byte 2^32 of it); plain (k_pair_res, then resident = 0: k_pair_str), PHAT, then refine = 4 with
    quality.  2.5 GiB of input, 5 GiB of spectra, 22 MiB of outputs: under 8 GiB."""
    import test_gpu_quality as tq
    import test_gpu_refined as tr
    import test_gpu_weighted as tw
    c = lb.CASES["S1"]
    N, B, W, T, P = c["N"], c["B"], c["W"], c["T"], c["P"]
    iq, raw, pl, ref = _ref64(c)
    text = _plan_text(c)
    big = _upload(iq, W)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        eng.set_option("fused", 0)
        got, tk = _correlate(eng, big, W, P)
        assert tk == {"k_fwd": 1, KWIN: 1}, tk
        assert eng.scratch_bytes() > 5 << 30
        _bars(got, ref, iq, pl, T, "S1 plain", text)
        eng.set_option("resident", 0)                          # k_pair_str instead of k_pair_res
        got, tk = _correlate(eng, big, W, P)
        assert tk == {"k_fwd": 1, KWIN: 1}, tk
        _bars(got, ref, iq, pl, T, "S1 plain, the streaming pair kernel", text)
        eng.set_option("resident", 1)
        got, tk = _correlate(eng, big, W, P, whiten=True)
        assert tk == {"k_fwd": 1, KWIN: 1}, tk
        want = lb.expand(_ref(("phat", N, B, T), lambda: wr.weighted_batch(iq, None, True, with_bound=True)), W, T)
        _named("S1 whiten", text, got[0], want[0], lambda: tw._assert_parity(*got, want))
        got, tk = _correlate(eng, big, W, P, quality=True, refine=4)
        assert tk == {"k_fwd": 1, KWIN: 1, "k_quality": 1, "k_refine": 1}, tk
        want = lb.expand(_ref(("refined", N, B, T), lambda: rr.refined_batch(iq, 4)), W, T)
        _named("S1 refine = 4", text, got[0], want[0], lambda: tr._assert_refined(got[:3], want, N, what="S1 refine = 4"))
        wq = _ref(("quality", N, B, T), lambda: qr.quality_batch(iq))[lb.window_map(W, T)]
        _named("S1 quality", text, got[0], want[0], lambda: tq._assert_quality(got[3], wq, N, "S1 quality"))


def test_derotated_spectra_past_4gib_doppler_search(xc, opts):
    """S2: S1's shape through the Doppler search with three hypotheses: the per-hypothesis sweep, one chunk: d_spec and the
    de-rotated set 5 GiB each, hyp_items of 778 240 slots.  2.5 GiB of input: under 13 GiB."""
    import test_gpu_caf as tc
    c = lb.CASES["S2"]
    N, B, W, T, P = c["N"], c["B"], c["W"], c["T"], c["P"]
    iq, raw, _ = lb.base_scene(N, B, T, doppler=True)
    grid = lb.caf_grid(N)
    ref = _ref(("caf", N, B, T), lambda: cr.reference(iq, grid))
    assert lb.distinct(ref["lag_int"])
    big = _upload(iq, W)
    o = _outputs(W, P, dop=True)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        eng.set_option("fused", 0)
        eng.caf_device(big.data_ptr(), W, grid, o["dop"].data_ptr(), o["lag_int"].data_ptr(), o["lag_frac"].data_ptr(), o["peak"].data_ptr())
        eng.synchronize()
        tk = {k: v["launches"] for k, v in eng.last_timing_by_kernel().items()}
        print("launches", tk, "scratch %.2f GiB" % (eng.scratch_bytes() / 2.0 ** 30))
        assert tk == {"k_fwd": 4, KWIN: 3, "k_caf_select": 3}, tk
    got = tuple(o[n].cpu().numpy() for n in ("dop", "lag_int", "lag_frac", "peak"))
    want = lb.expand(ref, W, T)
    _named("S2 Doppler search", _plan_text(c), got[1], want["lag_int"], lambda: tc._assert_parity(got, want))


def test_four_step_spectra_past_4gib_custom_pairs(xc, opts):
    """S3: N 65536, 8 buoys, 600 windows, pairs (0, 7) and (3, 4): one chunk whose g_spec is 4.7 GiB (g_cols_fwd and the
    forward rows write, the inverse rows read buoys 7 and 4 of the last windows past byte 2^32).  2.3 GiB of input, 1.2 GiB
    of products: under 9 GiB."""
    c = lb.CASES["S3"]
    pairs = np.array([(0, 7), (3, 4)], np.int32)
    iq, raw, pl, ref = _ref64(c, pairs)
    big = _upload(iq, c["W"])
    with xc.XcorrEngine(c["B"], c["N"], c["W"]) as eng:
        eng.set_option("timing", 1)
        got, tk = _correlate(eng, big, c["W"], 2, pairs=pairs)
        assert tk == {k: 1 for k in TWO_PASS}, tk
        assert eng.scratch_bytes() > (1 << 32) + (1 << 30)
        _bars(got, ref, iq, pl, c["T"], "S3 custom pairs", _plan_text(c))


# ---- more than 65 535 grid rows ---------------------------------------------------------------------------------------------
def _grid_chunk(W, P, K=1):
    """the chunk plan_route cuts for one band: whole groups, at most MAX_GRID_ROWS rows of g_cols_inv, at most 4096 windows"""
    return min(min(W, MAX_CHUNK), (MAX_GRID_ROWS // P) * K) // K * K


def test_products_past_4gib_and_67200_grid_rows(xc, opts):
    """S4 and G1: N 8192, 16 buoys, 560 windows, PHAT, default options: 67 200 slots, which the plan cuts into chunks of 546
    and 14 windows (65 520 and 1680 rows of g_cols_inv); the first chunk's g_prod is 8.0 GiB.  0.55 GiB of input, 1.1 GiB of
    spectra, 8.2 GiB of products, 0.3 GiB of tile records and halo: under 11 GiB."""
    import test_gpu_weighted as tw
    N, B, W, T = 8192, 16, 560, 7
    P = B * (B - 1) // 2
    c = lb.CASES["S4"]
    assert _grid_chunk(W, P) == c["W"] == 546 and W * P == 67200
    iq, raw, _ = lb.base_scene(N, B, T)
    big = _upload(iq, W)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        got, tk = _correlate(eng, big, W, P, whiten=True)
        assert tk == {k: 2 for k in ANCHOR}, tk
        assert eng.scratch_bytes() > 8 << 30
    want = lb.expand(_ref(("phat", N, B, T), lambda: wr.weighted_batch(iq, None, True, with_bound=True)), W, T)
    _named("S4 / G1 whiten", _plan_text(c), got[0], want[0], lambda: tw._assert_parity(*got, want))


GRID = [("plain", 8, 2400, 1), ("bounded", 8, 2400, 1), ("integrate2", 8, 4800, 2), ("integrate2-10buoys", 10, 3200, 2)]


@pytest.mark.parametrize("what,B,W,K", GRID, ids=[g[0] for g in GRID])
def test_more_than_65535_slots_through_the_four_step(xc, opts, what, B, W, K):
    """G2: N 1024 through the four-step kernels (small_maxl 1024, no whole-window kernel): 8 buoys x 2400 windows = 67 200
    slots, plain and bounded, in chunks of 2340 and 60 windows; integrate = 2 on 4800 windows (67 200 slots: a chunk of 4096
    windows is 57 344 rows, the cap on the chunk's windows is reached first at 8 buoys) and on 10 buoys x 3200 windows
    (72 000 slots: chunks of 2912 and 288 windows, whole groups).  At most 0.3 GiB of input and spectra and 2.3 GiB of
    products."""
    import test_gpu_integrated as ti
    N, T = 1024, 7
    P = B * (B - 1) // 2
    assert W * P // K > MAX_GRID_ROWS
    opts("small_maxl", 1024)
    opts("wscr", 0)
    iq, raw, _ = lb.base_scene(N, B, T)
    pl = orc.pair_list(B)
    chunk = _grid_chunk(W, P, K)
    chunks = -(-W // chunk)
    assert chunk % K == 0 and chunk * P // K <= MAX_GRID_ROWS and chunks == 2
    big = _upload(iq, W)
    text = "G2 %s: %d windows, %d slots, chunks of %d windows" % (what, W, W * P // K, chunk)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        if K == 1:
            ref = _ref(("ref64", N, B, T, pl.tobytes()), lambda: F.ref64_batch(iq, pl))
            req = {"lag_bounds": _bounds_around(ref, N, W, T)} if what == "bounded" else {}
            got, tk = _correlate(eng, big, W, P, **req)
            assert tk == {k: chunks for k in TWO_PASS}, tk
            _bars(got, ref, iq, pl, T, text, text)
        else:
            ref = _ref(("integ", N, B, T, K), lambda: ir.integrated_batch(lb.group_scene(iq, K), K, with_bound=True))
            got, tk = _correlate(eng, big, W, P, integrate=K)
            assert tk == {k: chunks for k in TWO_PASS}, tk
            want = lb.expand(ref, W // K, T)
            _named(text, text, got[0], want[0], lambda: ti._assert_parity(*got, want, text))
