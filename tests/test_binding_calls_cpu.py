"""Replay of tests/golden/binding_calls.json (tools/record_binding_calls.py): every call that XcorrEngine makes into the
library, that MultiXcorrEngine makes on its engines and that TDoACalculator.measure_lags / measure_band_lags make on theirs --
the entry or method, every argument, the host arrays' contents, the shapes that come back, and for the wrong calls the
exception and its text -- is what the table holds (the odd calls written out, the cross products as one digest per row).  The table was recorded with xcorr.py, multi.py and tdoa_processor.py of
the commit in front of the checked request (xcorr.LagRequest), so this pins "the one request makes the calls that the six
methods, the five closures and the two folds made".  No GPU, no library: fakes throughout.  Behind the replay, what no table
can say about the request: it keeps its arrays alive, and cutting it into blocks does not change it."""
import ctypes as C
import gc
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_binding_calls as rec  # noqa: E402

from radio_mapper_amd import xcorr  # noqa: E402

TABLE = rec.load()


def _blocks():
    """the tool's names, per cross product, and the names of the rows that are written out"""
    by_block = {}
    for n in rec.names():
        by_block.setdefault(rec._block(n), []).append(n)
    return by_block


def test_table_is_the_tool_s_list():
    """the committed table holds exactly the combinations the tool walks today: none can drop out silently"""
    blocks = _blocks()
    assert TABLE["name"] == rec.NAME and [r[0] for r in TABLE["rows"]] == blocks.pop(None)
    assert set(TABLE["combinations"]) == set(blocks) == {"engine", "multi", "calc"}
    for k, c in TABLE["combinations"].items():
        assert c["count"] == len(blocks[k]) == len(c["outcomes"]) and c["names"] == rec._digest(blocks[k], 16), k
    n = [sum(1 for _ in f()) for f in (rec.engine_combinations, rec.multi_combinations, rec.calculator_combinations)]
    assert n == [2 * 2 * 2 * 3 * (3 + 2 + 3 * 2) * 2 * 2 * 2 * 2, (3 * 3 + 3 * 2 + 3 * 3 * 2) * 2 * 3 * 2 * 2 + 24, 2 * (144 + 18 + 6 + 48)]
    assert n == [TABLE["combinations"][k]["count"] for k in ("engine", "multi", "calc")]
    assert sum(isinstance(r[1], dict) for r in TABLE["rows"]) >= 50      # the wrong calls, each with its exception


def test_every_call_is_the_recorded_one():
    """row by row: the rows that are written out against their text, every row of the cross products against its digest
    (tools/record_binding_calls.py prints a row in full on either commit)"""
    full = rec.walk()
    got, blocks = rec.compact(full), _blocks()
    for new, old in zip(got["rows"], TABLE["rows"]):
        assert new == old, f"{old[0]}: the first call that differs"
    assert len(got["rows"]) == len(TABLE["rows"])
    outcome = dict((r[0], r[1]) for r in full["rows"])
    for k, c in TABLE["combinations"].items():
        for name, new, old in zip(blocks[k], got["combinations"][k]["outcomes"], c["outcomes"]):
            assert new == old, f"{name}: the first combination that differs (NAME in tools/record_binding_calls.py); now {outcome[name]}"
    assert got["arrays"] == TABLE["arrays"]


class _Reading:
    """a library whose one entry reads the lag bounds, the band and the pairs while the call is running"""
    def __init__(self):
        self.seen = None

    def rmx_xcorr_batch_weighted(self, ctx, iq, W, pp, P, bd, bd_pw, wt, lb, lb_pw, li, lf, pk, flags):
        read = lambda p, t, shape: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape).tolist()   # noqa: E731
        self.seen = (read(pp, C.c_int32, (P, 2)), read(bd, C.c_double, (2,)), read(lb, C.c_int32, (P, 2)))
        return 0


def test_a_request_keeps_the_checked_arrays_alive_until_the_call():
    lib = _Reading()
    eng = rec.make_engine(lib)
    pairs, bounds, band = [[1, 0], [2, 1]], [[-3, 4], [-5, 6]], [-0.25, 0.125]
    req = xcorr.lag_request("xcorr", 3, 4, pairs, bounds, band)
    pairs[0][0], bounds[1][1], band[0] = 2, 99, 0.0          # the caller's own lists change and go away ...
    del pairs, bounds, band
    gc.collect()
    junk = [np.full(64, 7, np.int32) for _ in range(64)]     # ... and what they held may be handed out again
    out = np.zeros((3, 8), np.int32)
    ptrs = [None, None] + [out[k].ctypes.data_as(C.c_void_p) for k in range(3)] + [None]
    eng._call(req, C.c_void_p(64), ptrs, 0)
    assert lib.seen == ([[1, 0], [2, 1]], [-0.25, 0.125], [[-3, 4], [-5, 6]]) and len(junk) == 64
    # the request holds the arrays the entry read, of the types the ABI names
    assert req.pairs.dtype == np.int32 and req.bounds.dtype == np.int32 and req.band.dtype == np.float64
    assert all(a.flags.c_contiguous for a in (req.pairs, req.bounds, req.band))


def _request():
    rng = np.random.default_rng(5)
    lb = np.sort(rng.integers(-15, 16, size=(6, 3, 2)), axis=-1)
    bands = np.sort(rng.uniform(-0.5, 0.5, size=(12, 2, 2)), axis=-1)
    return xcorr.lag_request("bands", 3, 12, None, lb, bands, True, 2, 4, True), lb, bands


def _snapshot(req):
    return [v.copy() if isinstance(v, np.ndarray) else v for v in req]


def _same(a, b):
    return all(np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v for u, v in zip(a, b))


def test_cutting_a_request_into_blocks_does_not_change_it():
    req, lb, bands = _request()
    before = _snapshot(req)
    first = [req.cut(g0, g1) for g0, g1 in ((0, 2), (2, 4), (4, 6))]
    again = [req.cut(g0, g1) for g0, g1 in ((0, 2), (2, 4), (4, 6))]
    assert _same(before, _snapshot(req))
    for (b0, d0), (b1, d1), (g0, g1) in zip(first, again, ((0, 2), (2, 4), (4, 6))):
        assert np.array_equal(b0, b1) and np.array_equal(d0, d1)
        assert np.array_equal(b0, lb[g0:g1]) and np.array_equal(d0, bands[2 * g0:2 * g1])      # bounds by group, bands by window
    assert [(n, np.dtype(t).name, s) for n, t, s in req.outputs()] == [
        ("lag_int", "int32", (6, 2, 3)), ("lag_frac", "float32", (6, 2, 3)), ("peak", "float32", (6, 2, 3)),
        ("quality", "float32", (6, 2, 3, 4))]
    for change in (lambda: setattr(req, "K", 1), lambda: req.__setitem__(2, 1)):    # a tuple: nothing to set
        try:
            change()
        except (AttributeError, TypeError):
            continue
        raise AssertionError("a request must not take a new value")
    shared = xcorr.lag_request("caf", 3, 12, None, lb[0], bands[0, 0], False, None, 0, False, [0.0], True)
    assert shared.cut(3, 5)[0] is shared.bounds and shared.cut(3, 5)[1] is shared.band                 # what every row shares goes whole
    assert [n for n, _, _ in shared.outputs()] == ["dop_idx", "dop_frac", "lag_int", "lag_frac", "peak"]


def test_two_threads_cutting_one_request_get_their_own_blocks():
    req, lb, bands = _request()
    before = _snapshot(req)
    got, start = {}, threading.Barrier(2)

    def worker(rank):
        start.wait()
        for _ in range(200):
            got[rank] = [req.cut(g, g + 1) for g in range(3 * rank, 3 * rank + 3)]
    threads = [threading.Thread(target=worker, args=(r,)) for r in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for rank in (0, 1):
        for k, (b, d) in enumerate(got[rank]):
            g = 3 * rank + k
            assert np.array_equal(b, lb[g:g + 1]) and np.array_equal(d, bands[2 * g:2 * g + 2])
    assert _same(before, _snapshot(req))
