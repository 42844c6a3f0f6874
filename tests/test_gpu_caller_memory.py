"""What include/rmx.h promises about memory the library does not own, held on every correlation and Doppler-search route:
a call writes exactly its output arrays and nothing in front of, behind or between them, never its input; with
RMX_IN_DEVICE | RMX_OUT_DEVICE it works on the caller's HBM at the caller's placement -- aligned to 256 bytes or only to
the element, as a slice of a larger buffer is --; and everything it queues is ordered on the ctx stream, a stream that
does not synchronise with the null stream included, two asynchronous calls back to back.

Every buffer lies in a guarded slab of tests/caller_memory_ref.py (tests/test_caller_memory_cpu.py shows that its checker
reports a single altered word).  The expected values are never computed here: they are the recorded digests of
tests/golden/route_table.json (the host door, aligned buffers) or a host-door call on a fresh engine, bit for bit.

  a. every row of the route table through the device door, at both placements: launches, digest, guards, fill, input
  b. the several-band entries (the table has no row for them), plain and with PHAT, bounds, refinement and quality
  c. uint8 input on every kernel family, at the element-aligned placement
  d. pointers aligned to less than their element are refused (decided by reading the kernels, see include/rmx.h)
  e. the host door with guards around numpy outputs (fetch_out's packed copy, the fourth array's copy)
  f. stream order on a torch.cuda.Stream(): input produced, two calls and both outputs consumed without a host wait"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import caller_memory_ref as cm
import radio_mapper_amd as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from record_routes import TABLE, _pairs, _windows, digest  # noqa: E402

pytestmark = pytest.mark.gpu

with open(TABLE) as _f:
    ROWS = json.load(_f)["cases"]
BY_NAME = {r["name"]: r for r in ROWS}
FS = 10e6
# recorded for the pipelined host copy, whose tail rule differs from the device door's; n4096_b3_w521_device is its twin
HOST_COPY_ROW = "n4096_b3_w521_host"
ROWS_A = [r for r in ROWS if r["name"] != HOST_COPY_ROW]


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


# ---- guarded slabs on the device and in numpy ------------------------------------------------------------------------
class Guarded:
    """one slab of caller_memory_ref: `before` is what it held when the call was queued"""

    def __init__(self, arrays, placement, values=None, device=True):
        self.lay = cm.layout(arrays, placement)
        self.before = cm.fill(self.lay)
        for name, v in (values or {}).items():
            cm.put(self.before, self.lay, name, v)
        if device:
            import torch
            self.t = torch.from_numpy(self.before).to(torch.device("cuda", 0))
            self.base = self.t.data_ptr()
        else:
            self.t = None
            self.host = cm.numpy_slab(self.lay.nbytes)
            self.host[:] = self.before
            self.base = self.host.ctypes.data
        assert self.base % cm.BASE_ALIGN == 0, "the slab base is aligned as the layout presumes"

    def ptr(self, name):
        return self.base + self.lay.entries[name].offset

    def after(self):
        return self.host if self.t is None else self.t.cpu().numpy()

    def body(self, name):
        """the device tensor's bytes of one array (for copies queued by the test)"""
        e = self.lay.entries[name]
        return self.t[e.offset:e.back]


def _in_arrays(iq):
    return [("iq", iq.dtype, iq.size)]


def _out_arrays(slots, quality=False, caf=False):
    a = [("lag_int", np.int32, slots), ("lag_frac", np.float32, slots), ("peak", np.float32, slots)]
    if quality:
        a.append(("quality", np.float32, 4 * slots))
    if caf:
        a.append(("dop_idx", np.int32, slots))                 # (listed last: lag_int, lag_frac, peak keep 4, 8, 12 mod 16)
    return a


def _results(slab, out, shape, quality=False, caf=False):
    """the output arrays cut out of a slab's bytes, in the order the host door returns them"""
    names = (["dop_idx"] if caf else []) + ["lag_int", "lag_frac", "peak"] + (["quality"] if quality else [])
    return [cm.cut(slab, out.lay, n, tuple(shape) + ((4,) if n == "quality" else ())) for n in names]


def _few(findings):
    return "%d findings, the first: %s" % (len(findings), findings[:8])


def _assert_memory(inp, out, after_in, after_out, written):
    """no guard word changed, front or back; no fill left in a written body, no byte changed in another one; the input
    slab, guards included, is byte for byte what it was"""
    bad = cm.check(out.before, after_out, out.lay, written)
    assert not bad, "outputs: " + _few(bad)
    if inp is not None:
        bad = cm.check(inp.before, after_in, inp.lay, [])
        assert not bad, "input: " + _few(bad)
        assert np.array_equal(inp.before, after_in)


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, "array %d differs in %d elements"
                                                                      % (k, int((a.view(np.uint32) != b.view(np.uint32)).sum())))


def _launches(eng):
    return {k: v["launches"] for k, v in sorted(eng.last_timing_by_kernel().items())}


def _bounds(P, lo=-64, hi=64):
    return np.tile(np.array([[lo, hi]], np.int32), (P, 1))


def _row_kw(row, P):
    """the request of a table row as correlate() / correlate_device() take it (tools/record_routes.py: run_case)"""
    kw = dict(pairs=_pairs(row["pairs"], row["B"]), band=row["band"], whiten=row["whiten"], integrate=row["integrate"],
              refine=row["refine"])
    if row["bounded"]:
        kw["lag_bounds"] = _bounds(P)
    return kw


def _n_pairs(row):
    pairs = _pairs(row["pairs"], row["B"])
    return len(pairs) if pairs is not None else row["B"] * (row["B"] - 1) // 2


def _set_defaults(xc, row):
    xc.clear_default_options()
    for k, v in row["defaults"].items():
        xc.set_default_option(k, v)


def _engine(xc, row, timing=True):
    eng = xc.XcorrEngine(row["B"], row["N"], row["max_windows"])
    for k, v in row["options"].items():
        eng.set_option(k, v)
    if timing:
        eng.set_option("timing", 1)
    return eng


def _by_value(row, got):
    """tests/test_gpu_routes.py's rule for a row recorded as not reproducible (digest null; none today)"""
    ref = [np.asarray(a, dtype=g.dtype).reshape(g.shape) for a, g in zip(row["arrays"], got)]
    caf = row["kind"] == "caf"
    if caf:
        assert np.array_equal(got[0], ref[0])
    li, lf, pk = got[1 if caf else 0:][:3]
    ri, rf, rp = ref[1 if caf else 0:][:3]
    assert np.array_equal(li, ri)
    lag, rlag = li + lf.astype(np.float64), ri + rf.astype(np.float64)
    assert np.all(np.abs(lag - rlag) <= 1e-5 * np.maximum(np.abs(rlag), 1.0))
    assert np.allclose(pk, rp, rtol=1e-5, atol=0)
    if row["quality"]:
        assert np.allclose(got[3], ref[3], rtol=1e-5, atol=0)


def _device_call(eng, row, inp, out, W, P, u8, kw):
    """the row's call through the device binding, every pointer into the two slabs"""
    if row["kind"] == "caf":
        eng.caf_device(inp.ptr("iq"), W, row["dopplers"], out.ptr("dop_idx"), out.ptr("lag_int"), out.ptr("lag_frac"),
                       out.ptr("peak"), pairs=kw["pairs"], u8=u8)
    else:
        eng.correlate_device(inp.ptr("iq"), W, out.ptr("lag_int"), out.ptr("lag_frac"), out.ptr("peak"), u8=u8,
                             quality_ptr=out.ptr("quality") if row["quality"] else 0, **kw)


# ---- a. every row of the route table through the device door --------------------------------------------------------------
@pytest.mark.parametrize("placement", cm.PLACEMENTS)
@pytest.mark.parametrize("row", ROWS_A, ids=[r["name"] for r in ROWS_A])
def test_table_row_through_the_device_door(xc, row, placement):
    """The device door at either placement is the recorded host door bit for bit, launches the family the row is named
    for, and touches nothing but its outputs; a row recorded as a refusal raises the same text and writes nothing."""
    import torch
    caf, W, P = row["kind"] == "caf", row["W"], _n_pairs(row)
    rows_out = W // row["integrate"]
    _set_defaults(xc, row)
    try:
        iq = _windows(row)
        inp = Guarded(_in_arrays(iq), placement, {"iq": iq})
        out = Guarded(_out_arrays(rows_out * P, row["quality"], caf), placement)
        written = [a[0] for a in _out_arrays(1, row["quality"], caf)]
        with _engine(xc, row) as eng:
            torch.cuda.synchronize()
            if "error" in row:
                with pytest.raises(xc.RmxError) as e:
                    _device_call(eng, row, inp, out, W, P, row["u8"], _row_kw(row, P))
                eng.synchronize()
                assert str(e.value) == row["error"]
                after_out = out.after()
                assert np.array_equal(out.before, after_out), "a refused call writes nothing"
                _assert_memory(inp, out, inp.after(), after_out, [])
                return
            _device_call(eng, row, inp, out, W, P, row["u8"], _row_kw(row, P))
            eng.synchronize()
            launches = _launches(eng)
        print(row["name"], placement, launches)
        assert launches == row["launches"]
        after_in, after_out = inp.after(), out.after()
        got = _results(after_out, out, (rows_out, P), row["quality"], caf)
        if row["digest"] is not None:
            assert digest(got) == row["digest"]
        else:
            _by_value(row, got)
        _assert_memory(inp, out, after_in, after_out, written)
    finally:
        xc.clear_default_options()


# ---- b. the several-band entries ---------------------------------------------------------------------------------------------
BAND_SHAPES = [(3, 256, 6), (3, 4096, 6), (3, 8192, 6), (3, 65536, 6), (8, 65536, 2)]
BAND_MODES = {"plain": dict(), "phat_bounds_refine4_quality": dict(whiten=True, refine=4, quality=True)}
M_BANDS = 3


def _band_sets(W):
    """bands[w][m]: three disjoint bands per window whose edges move with the window, inside [-0.45, 0.45]; the narrowest
    is 0.17 wide, 87 bins of the shortest transform here (L = 512), so every band keeps far more than 16 bins"""
    w = np.arange(W, dtype=np.float64)[:, None]
    lo = np.array([[-0.42, -0.10, 0.20]]) + w * np.array([[0.005, -0.010, 0.010]])
    hi = np.array([[-0.25, 0.12, 0.45]]) + w * np.array([[0.010, 0.005, -0.005]])
    bands = np.stack([lo, hi], axis=-1)
    assert bands.shape == (W, M_BANDS, 2) and np.all(np.abs(bands) <= 0.45) and np.all(bands[..., 1] - bands[..., 0] >= 16.5 / 512)
    return bands


_band_expected = {}


def _banded_case(xc, B, N, W, mode, seed=23):
    """(windows, bands, request, host-door result of a fresh engine), computed once per shape and mode"""
    key = (B, N, W, mode, seed)
    if key not in _band_expected:
        if len(_band_expected) >= 4:
            _band_expected.clear()
        iq = rm.synth.make_windows(W, B, N, FS, seed=seed)[0]
        bands = _band_sets(W)
        kw = dict(BAND_MODES[mode])
        if kw:
            kw["lag_bounds"] = _bounds(B * (B - 1) // 2)
        with xc.XcorrEngine(B, N, W) as eng:
            want = eng.correlate_bands(iq, bands, **kw)
        _band_expected[key] = (iq, bands, kw, want)
    return _band_expected[key]


def _banded_device(eng, inp, out, W, bands, kw, pairs=None):
    q = kw.get("quality", False)
    eng.correlate_bands_device(inp.ptr("iq"), W, bands, out.ptr("lag_int"), out.ptr("lag_frac"), out.ptr("peak"), pairs=pairs,
                               lag_bounds=kw.get("lag_bounds"), whiten=kw.get("whiten", False), refine=kw.get("refine", 0),
                               quality_ptr=out.ptr("quality") if q else None)


@pytest.mark.parametrize("placement", cm.PLACEMENTS)
@pytest.mark.parametrize("mode", list(BAND_MODES))
@pytest.mark.parametrize("shape", BAND_SHAPES, ids=["b%d_n%d_w%d" % s for s in BAND_SHAPES])
def test_bands_through_the_device_door(xc, opts, shape, mode, placement):
    """rmx_xcorr_batch_bands(_quality) on the caller's HBM: the [W][M][P] (x 4) outputs of the host door bit for bit,
    the virtual windows of every pair kernel inside the arrays.  8 buoys at N = 65536 is the shape whose weighted call
    runs g_rows_anchor, which the banded call must not."""
    import torch
    B, N, W = shape
    P = B * (B - 1) // 2
    opts("ncus", 8)
    iq, bands, kw, want = _banded_case(xc, B, N, W, mode)
    quality = kw.get("quality", False)
    inp = Guarded(_in_arrays(iq), placement, {"iq": iq})
    out = Guarded(_out_arrays(W * M_BANDS * P, quality), placement)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        torch.cuda.synchronize()
        _banded_device(eng, inp, out, W, bands, kw)
        eng.synchronize()
        launches = _launches(eng)
    print(shape, mode, placement, launches)
    assert "g_rows_anchor" not in launches and "g_rows_fused" not in launches
    after_in, after_out = inp.after(), out.after()
    _same(_results(after_out, out, (W, M_BANDS, P), quality), want, (shape, mode, placement))
    _assert_memory(inp, out, after_in, after_out, [a[0] for a in _out_arrays(1, quality)])


# ---- c. uint8 input on every kernel family --------------------------------------------------------------------------------------
def _first_row_of_each_family_set():
    """The selection rule: walk the table in its order and keep the first non-error correlation row for each distinct
    SET of kernel families (the keys of its "launches"), whatever the counts -- so a family added to the table later is
    picked up here.  The pipelined host-copy row is left out as in (a)."""
    seen, picked = set(), []
    for r in ROWS_A:
        if r["kind"] != "xcorr" or "error" in r:
            continue
        key = tuple(sorted(r["launches"]))
        if key not in seen:
            seen.add(key)
            picked.append(r)
    return picked


U8_ROWS = _first_row_of_each_family_set()


@pytest.mark.parametrize("row", U8_ROWS, ids=[r["name"] for r in U8_ROWS])
def test_uint8_input_on_every_family(xc, row):
    """raw uint8 I,Q windows aligned to one I,Q pair (2 mod 16) through the device door: the host door's result on the same
    bytes, bit for bit, with the same launches"""
    import torch
    W, P = row["W"], _n_pairs(row)
    rows_out = W // row["integrate"]
    u8row = dict(row, u8=True)
    _set_defaults(xc, row)
    try:
        raw = _windows(u8row)
        assert raw.dtype == np.uint8 and raw.shape == (W, row["B"], 2 * row["N"])
        kw = _row_kw(row, P)
        with _engine(xc, row) as eng:
            want = eng.correlate(raw, quality=row["quality"], **kw)
            want_launches = _launches(eng)
        inp = Guarded(_in_arrays(raw), "natural", {"iq": raw})
        assert inp.ptr("iq") % 16 == 2
        out = Guarded(_out_arrays(rows_out * P, row["quality"]), "natural")
        with _engine(xc, row) as eng:
            torch.cuda.synchronize()
            _device_call(eng, row, inp, out, W, P, True, kw)
            eng.synchronize()
            launches = _launches(eng)
        print(row["name"], launches)
        assert launches == want_launches and set(launches) == set(row["launches"])
        after_in, after_out = inp.after(), out.after()
        _same(_results(after_out, out, (rows_out, P), row["quality"]), list(want), row["name"])
        _assert_memory(inp, out, after_in, after_out, [a[0] for a in _out_arrays(1, row["quality"])])
    finally:
        xc.clear_default_options()


# ---- d. pointers aligned to less than their element are refused -----------------------------------------------------------------
def test_pointers_aligned_to_less_than_the_element_are_refused(xc):
    """Decided by reading, not by trying (include/rmx.h, host_request.hpp: check_alignment): the kernels index a device
    `iq` as uchar2 / float2 and load it with 16- and 64-bit buffer loads, and store 4-byte outputs.  A device pointer
    aligned to less -- uint8 input at an odd address among them -- is RMX_E_INVAL with a text naming the array, before
    anything is queued or written; the same pointer as a HOST pointer is taken."""
    import torch
    B, N, W, P = 3, 256, 2, 3
    iq, _, raw = rm.synth.make_windows(W, B, N, FS, seed=3, return_u8=True)
    dev = torch.device("cuda", 0)
    x_c = torch.full((iq.nbytes + 16,), cm.FILL_BYTE, dtype=torch.uint8, device=dev)
    x_c[8:8 + iq.nbytes] = torch.from_numpy(iq.view(np.uint8).reshape(-1)).to(dev)
    x_u = torch.full((raw.nbytes + 16,), cm.FILL_BYTE, dtype=torch.uint8, device=dev)
    x_u[2:2 + raw.nbytes] = torch.from_numpy(raw.reshape(-1)).to(dev)
    out = Guarded(_out_arrays(W * P, True) + [("dop_idx", np.int32, W * P)], "natural")
    o = {n: out.ptr(n) for n in ("lag_int", "lag_frac", "peak", "quality", "dop_idx")}
    torch.cuda.synchronize()
    with xc.XcorrEngine(B, N, W) as eng:
        def refused(text, iq_ptr, u8=False, caf=False, **moved):
            p = dict(o, **moved)
            with pytest.raises(xc.RmxError) as e:
                if caf:
                    eng.caf_device(iq_ptr, W, [0.0, 1e-4], p["dop_idx"], p["lag_int"], p["lag_frac"], p["peak"], u8=u8)
                else:
                    eng.correlate_device(iq_ptr, W, p["lag_int"], p["lag_frac"], p["peak"], u8=u8, quality_ptr=p["quality"])
            assert e.value.code == -1 and str(e.value) == "rmx error -1: " + text
        c64 = "complex64 input must be aligned to 8 bytes (one sample)"
        pair = "uint8 input must be aligned to 2 bytes (one I,Q pair)"
        word = " bytes past a multiple of 4: an output must be aligned to 4 bytes (one element)"
        for caf in (False, True):
            refused("iq is a device pointer 4 bytes past a multiple of 8: " + c64, x_c.data_ptr() + 12, caf=caf)
            refused("iq is a device pointer 1 bytes past a multiple of 8: " + c64, x_c.data_ptr() + 9, caf=caf)
            refused("iq is a device pointer 1 bytes past a multiple of 2: " + pair, x_u.data_ptr() + 3, u8=True, caf=caf)
            refused("lag_int is a device pointer 2" + word, x_c.data_ptr() + 8, caf=caf, lag_int=o["lag_int"] + 2)
            refused("lag_frac is a device pointer 1" + word, x_u.data_ptr() + 2, u8=True, caf=caf, lag_frac=o["lag_frac"] + 1)
            refused("peak is a device pointer 3" + word, x_c.data_ptr() + 8, caf=caf, peak=o["peak"] + 3)
        refused("quality is a device pointer 2" + word, x_c.data_ptr() + 8, quality=o["quality"] + 2)
        refused("dop_idx is a device pointer 1" + word, x_c.data_ptr() + 8, caf=True, dop_idx=o["dop_idx"] + 1)
        eng.synchronize()
        assert np.array_equal(out.before, out.after()), "a refused call writes nothing"
        # the element-aligned pointers themselves are taken, and a host pointer needs nothing: an odd uint8 address
        host = np.empty(raw.nbytes + 2, np.uint8)
        first = 1 - host.ctypes.data % 2
        odd = host[first:first + raw.nbytes].reshape(raw.shape)
        odd[...] = raw
        assert odd.ctypes.data % 2 == 1 and odd.flags.c_contiguous
        want = eng.correlate(raw)
        _same(eng.correlate(odd), want, "uint8 windows at an odd host address")
        eng.correlate_device(x_u.data_ptr() + 2, W, o["lag_int"], o["lag_frac"], o["peak"], u8=True)
        eng.synchronize()
        _same(_results(out.after(), out, (W, P)), want, "uint8 windows at 2 mod 16 on the device")


# ---- e. the host door with guards ----------------------------------------------------------------------------------------------
HOST_TAGS = ("bounded", "band_phat", "integ2", "refine4", "quality", "quality_band", "all", "all_two_chunks",
             "quality_two_chunks", "plain_two_chunks")
HOST_ROWS = [BY_NAME["n%d_%s" % (N, tag)] for N in (256, 4096) for tag in HOST_TAGS]


@pytest.mark.parametrize("placement", cm.PLACEMENTS)
@pytest.mark.parametrize("row", HOST_ROWS, ids=[r["name"] for r in HOST_ROWS])
def test_host_door_with_guards(xc, row, placement):
    """The feature rows of the table through the raw ABI with host pointers, the numpy outputs between guards: the copies
    out of the ctx's device block (fetch_out's packed path with its 256-byte strides, the fourth array's copy) end where
    the arrays end."""
    W, P = row["W"], _n_pairs(row)
    rows_out, quality = W // row["integrate"], row["quality"]
    _set_defaults(xc, row)
    try:
        iq = np.ascontiguousarray(_windows(row))
        keep = iq.copy()
        kw = _row_kw(row, P)
        out = Guarded(_out_arrays(rows_out * P, quality), placement, device=False)
        if placement == "natural":
            assert [out.ptr(n) % 16 for n in ("lag_int", "lag_frac", "peak")] == [4, 8, 12]
        with _engine(xc, row) as eng:
            pairs, pp, _ = eng._pairs_arg(kw["pairs"])
            lb, per_window = xc.check_lag_bounds(kw.get("lag_bounds"), rows_out, P)
            bd, band_pw = xc.check_band(kw["band"], W)
            eng._xcorr(iq.ctypes.data_as(C.c_void_p), W, pp, P, kw["integrate"], bd, band_pw, kw["whiten"], lb, per_window,
                       C.c_void_p(out.ptr("lag_int")), C.c_void_p(out.ptr("lag_frac")), C.c_void_p(out.ptr("peak")), 0, kw["refine"],
                       C.c_void_p(out.ptr("quality")) if quality else None)
            launches = _launches(eng)
        assert launches == row["launches"]
        after = out.after()
        assert digest(_results(after, out, (rows_out, P), quality)) == row["digest"]
        _assert_memory(None, out, None, after, [a[0] for a in _out_arrays(1, quality)])
        assert np.array_equal(iq.view(np.uint8), keep.view(np.uint8)), "the host input is untouched"
    finally:
        xc.clear_default_options()


# ---- f. stream order on a stream that does not synchronise with the null stream ---------------------------------------------
STREAM_ROWS = ["n4096_b8_w17_tail", "n4096_b3_w2", "n1024_b3_w5", "n8192_b8_w9", "n16384_b3_w4_k16min4", "n65536_b3_w2_cu32",
               "n4096_all"]
BIG_BYTES = 256 << 20


@pytest.fixture(scope="module")
def big_copy():
    """256 MiB pinned -> device: something for the producer of a call's input to queue behind"""
    import torch
    return torch.empty(BIG_BYTES, dtype=torch.uint8, pin_memory=True), torch.empty(BIG_BYTES, dtype=torch.uint8,
                                                                                   device=torch.device("cuda", 0))


def _second_call(row, kw, B):
    """call 2 of a stream case: the reversed pair list and, where the row has them, other bounds and another band"""
    kw2 = dict(kw)
    pl = kw["pairs"] if kw["pairs"] is not None else rm.xcorr.pair_list(B)
    kw2["pairs"] = np.ascontiguousarray(pl[::-1])
    if "lag_bounds" in kw:
        kw2["lag_bounds"] = _bounds(len(pl), -32, 96)
    if kw.get("band") is not None:
        kw2["band"] = [-0.3, 0.1]
    return kw2


def _queue_and_wait(s, big_copy, inp, pinned_in, calls, outs):
    """Everything of one stream case on `s`, with no host wait until the one at the end: the large copy, the producer of the
    input, the calls, the consumers of their outputs.  Returns the slabs' bytes as the consumers copied them."""
    import torch
    pinned_out = [torch.empty(o.lay.nbytes, dtype=torch.uint8, pin_memory=True) for o in outs]
    for p in pinned_out:
        p.fill_(0)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        big_copy[1].copy_(big_copy[0], non_blocking=True)
        if inp is not None:
            inp.body("iq").copy_(pinned_in, non_blocking=True)
        for call in calls:
            call()
        for p, o in zip(pinned_out, outs):
            p.copy_(o.t, non_blocking=True)
    s.synchronize()
    return [p.numpy().copy() for p in pinned_out]


def _stream_case(xc, big_copy, make_engine, iq, other, host_call, device_call, requests, shape_of, arrays_of):
    """requests: the two calls' keyword sets.  host_call(eng, windows, kw) -> arrays; device_call(eng, inp, out, kw) queues.
    Expected per call: the host door of a fresh engine given that one call; it must differ from the same call on the
    OTHER windows, which the device input holds until the producer's copy lands."""
    import torch
    want = []
    for kw in requests:
        with make_engine() as eng:
            w = list(host_call(eng, iq, kw))
        with make_engine() as eng:
            stale = list(host_call(eng, other, kw))
        assert any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(w, stale)), "the two inputs give one result"
        want.append(w)
    inp = Guarded(_in_arrays(iq), "natural", {"iq": other})
    outs = [Guarded(arrays_of(kw), "natural") for kw in requests]
    pinned_in = torch.from_numpy(np.ascontiguousarray(iq).view(np.uint8).reshape(-1).copy()).pin_memory()
    s = torch.cuda.Stream()
    with make_engine() as eng:
        eng.set_stream(s.cuda_stream)
        calls = [lambda kw=kw, out=out: device_call(eng, inp, out, kw) for kw, out in zip(requests, outs)]
        after = _queue_and_wait(s, big_copy, inp, pinned_in, calls, outs)
        eng.synchronize()
    for k, (kw, out, a) in enumerate(zip(requests, outs, after)):
        names = [x[0] for x in arrays_of(kw)]
        bad = cm.check(out.before, a, out.lay, names)
        assert not bad, "call %d: %s" % (k + 1, _few(bad))
        _same([cm.cut(a, out.lay, n, shape_of(kw, n)) for n in names], want[k], "call %d" % (k + 1))
    # the input slab now holds the produced windows between untouched guards
    now = inp.before.copy()
    cm.put(now, inp.lay, "iq", iq)
    assert np.array_equal(inp.after(), now)


@pytest.mark.parametrize("name", STREAM_ROWS)
def test_two_calls_queued_on_a_side_stream(xc, big_copy, name):
    """Table rows on a torch.cuda.Stream(): the input arrives by an asynchronous copy queued behind a large one, two calls
    with different pair lists (bounds, band) follow on the SAME engine and their outputs are copied out, all without a
    host wait.  A call that read its input early, a pair table, band or bounds staged over the ones an earlier call
    still reads, or a copy on another stream would show in the bytes."""
    row = BY_NAME[name]
    B, N, W, P = row["B"], row["N"], row["W"], _n_pairs(row)
    rows_out, quality = W // row["integrate"], row["quality"]
    _set_defaults(xc, row)
    try:
        iq = np.ascontiguousarray(_windows(row)).copy()
        other = rm.synth.make_windows(W, B, N, FS, seed=row["seed"] + 1)[0]
        kw1 = _row_kw(row, P)

        def device_call(eng, inp, out, kw):
            eng.correlate_device(inp.ptr("iq"), W, out.ptr("lag_int"), out.ptr("lag_frac"), out.ptr("peak"),
                                 quality_ptr=out.ptr("quality") if quality else 0, **kw)

        _stream_case(xc, big_copy, lambda: _engine(xc, row, timing=False), iq, other,
                     lambda eng, x, kw: eng.correlate(x, quality=quality, **kw), device_call, [kw1, _second_call(row, kw1, B)],
                     lambda kw, n: (rows_out, P) + ((4,) if n == "quality" else ()), lambda kw: _out_arrays(rows_out * P, quality))
    finally:
        xc.clear_default_options()


def test_two_banded_calls_queued_on_a_side_stream(xc, opts, big_copy):
    """the N = 4096 banded case of (b) with PHAT, bounds, refinement and quality, then its pairs reversed under other
    bounds and the band sets in the opposite order"""
    B, N, W = BAND_SHAPES[1]
    P = B * (B - 1) // 2
    opts("ncus", 8)
    iq, bands, kw, _ = _banded_case(xc, B, N, W, "phat_bounds_refine4_quality")
    other = rm.synth.make_windows(W, B, N, FS, seed=24)[0]
    kw1 = dict(kw, bands=bands, pairs=None)
    kw2 = dict(kw, bands=np.ascontiguousarray(bands[:, ::-1]), pairs=np.ascontiguousarray(rm.xcorr.pair_list(B)[::-1]),
               lag_bounds=_bounds(P, -32, 96))

    def host_call(eng, x, k):
        return eng.correlate_bands(x, k["bands"], pairs=k["pairs"], lag_bounds=k["lag_bounds"], whiten=True, refine=4, quality=True)

    def device_call(eng, inp, out, k):
        _banded_device(eng, inp, out, W, k["bands"], k, pairs=k["pairs"])

    _stream_case(xc, big_copy, lambda: xc.XcorrEngine(B, N, W), iq, other, host_call, device_call, [kw1, kw2],
                 lambda k, n: (W, M_BANDS, P) + ((4,) if n == "quality" else ()), lambda k: _out_arrays(W * M_BANDS * P, True))


def test_pipelined_host_copy_on_a_side_stream(xc, big_copy):
    """n4096_b3_w521_host's shape through the raw ABI with RMX_OUT_DEVICE alone: the windows travel from host memory on the
    library's own copy stream, sub-chunk by sub-chunk, while the ctx stream -- a side stream with a large copy in front --
    runs the kernels; the outputs are consumed on that stream.  Expected: the row's digest."""
    import torch
    row = BY_NAME[HOST_COPY_ROW]
    W, P = row["W"], _n_pairs(row)
    _set_defaults(xc, row)
    try:
        iq = np.ascontiguousarray(_windows(row))
        keep = iq.copy()
        out = Guarded(_out_arrays(W * P), "natural")
        lib = xc.load_library()
        s = torch.cuda.Stream()
        with _engine(xc, row, timing=False) as eng:
            eng.set_stream(s.cuda_stream)

            def call():
                rc = lib.rmx_xcorr_batch(eng._ctx, iq.ctypes.data_as(C.c_void_p), W, None, 0, C.c_void_p(out.ptr("lag_int")),
                                         C.c_void_p(out.ptr("lag_frac")), C.c_void_p(out.ptr("peak")), xc.RMX_OUT_DEVICE)
                assert rc == 0, lib.rmx_last_error(eng._ctx)

            after, = _queue_and_wait(s, big_copy, None, None, [call], [out])
            eng.synchronize()
        bad = cm.check(out.before, after, out.lay, ["lag_int", "lag_frac", "peak"])
        assert not bad, _few(bad)
        assert digest(_results(after, out, (W, P))) == row["digest"]
        assert np.array_equal(iq.view(np.uint8), keep.view(np.uint8))
    finally:
        xc.clear_default_options()
