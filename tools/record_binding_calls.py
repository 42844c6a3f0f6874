"""CPU only: every call the Python binding makes, as a table -- the behaviour pin of radio-mapper_amd/xcorr.py, multi.py and
tdoa_processor.py.  Nothing here runs a kernel: 3 buoys, N = 16, at most 12 windows.

1. XcorrEngine over a fake library with the thirteen batch entries (nine rmx_xcorr_batch*, four rmx_caf_batch*): the full
   cross product of the options of correlate / correlate_bands / caf and their device-pointer twins.  Per combination: the
   entry's name, every scalar, for every pointer whether it is NULL, the contents of the host arrays (pairs, bounds,
   band(s), grid), the flags, and the shapes and dtypes of what the method returns.
2. doubly-wrong calls (the exception's type and text), the empty batches (no call) and a few odd ones.
3. MultiXcorrEngine over recording stub engines (devices [0, 1, 2], 12 windows, K in 1, 2, 3, one configuration whose engines
   hold two windows only), TDoACalculator.measure_lags / measure_band_lags with and without a channel axis: the method
   called on the engine, the window range, the positional and keyword arguments and the gathered shapes.

A row's name is its options, one character each (NAME below).  Arrays are written once, under "arrays", and referred to
as "@k" ("L@k": the caller's own list went through untouched).  The stored table (compact()) writes out the rows of 2. and the
seam; of the cross products it keeps one digest per row, which walk() reproduces in full on either commit.

usage: python tools/record_binding_calls.py OUT.json
       Record with the three modules of the commit BEFORE a change to them, never with the changed ones; an existing
       OUT.json is not overwritten.  tests/test_binding_calls_cpu.py replays tests/golden/binding_calls.json on the tree."""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "binding_calls.json")
B, N, M = 3, 16, 2
NAME = "family (X correlate, B correlate_bands, C caf) door (h host arrays, d device pointers) uint8 custom-pairs " \
       "bounds (0 none, 1 shared, 2 per row) band(s) (0 none, 1 shared, 2 per window) whiten K U quality fine"

HEAD = ["ctx", "iq", "n_windows", "pairs", "n_pairs"]
GRID = ["grid", "n_dopplers"]
WEIGHT = ["band", "band_pw", "weighting"]
SETS = ["band", "n_bands", "band_pw", "weighting"]
BOUNDS = ["bounds", "bounds_pw"]
OUT = ["lag_int", "lag_frac", "peak"]
DOP = ["dop_idx", "dop_frac"]
ENTRIES = {   # the parameters of include/rmx.h, in order
    "rmx_xcorr_batch": HEAD + OUT + ["flags"],
    "rmx_xcorr_batch_bounded": HEAD + BOUNDS + OUT + ["flags"],
    "rmx_xcorr_batch_weighted": HEAD + WEIGHT + BOUNDS + OUT + ["flags"],
    "rmx_xcorr_batch_bands": HEAD + SETS + BOUNDS + OUT + ["flags"],
    "rmx_xcorr_batch_integrated": HEAD + ["integrate"] + WEIGHT + BOUNDS + OUT + ["flags"],
    "rmx_xcorr_batch_refined": HEAD + ["integrate"] + WEIGHT + BOUNDS + ["refine"] + OUT + ["flags"],
    "rmx_xcorr_batch_quality": HEAD + ["integrate"] + WEIGHT + BOUNDS + ["refine"] + OUT + ["quality", "flags"],
    "rmx_xcorr_batch_bands_quality": HEAD + SETS + BOUNDS + ["refine"] + OUT + ["quality", "flags"],
    "rmx_xcorr_batch_bands_integrated": HEAD + ["integrate"] + SETS + BOUNDS + ["refine"] + OUT + ["quality", "flags"],
    "rmx_caf_batch": HEAD + GRID + ["dop_idx"] + OUT + ["flags"],
    "rmx_caf_batch_request": HEAD + GRID + WEIGHT + BOUNDS + DOP + OUT + ["flags"],
    "rmx_caf_batch_quality": HEAD + GRID + WEIGHT + BOUNDS + ["refine"] + DOP + OUT + ["quality", "flags"],
    "rmx_caf_batch_integrated": HEAD + GRID + ["integrate"] + WEIGHT + BOUNDS + ["refine"] + DOP + OUT + ["quality", "flags"],
}
POINTERS = ("iq", "lag_int", "lag_frac", "peak", "quality", "dop_idx", "dop_frac")


class Arrays:
    """every array of the table once: key(a) -> "@k" """
    def __init__(self):
        self.table, self.keys = {}, {}

    def key(self, a):
        a = np.asarray(a)
        entry = [a.dtype.name, list(a.shape), a.reshape(-1).tolist()]
        sig = json.dumps(entry)
        if sig not in self.keys:
            self.keys[sig] = "@%d" % len(self.keys)
            self.table[self.keys[sig]] = entry
        return self.keys[sig]

    def value(self, v):
        """an argument as an engine method receives it"""
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, np.generic):
            return f"{v.dtype.name}({v.item()})"
        if isinstance(v, np.ndarray):
            return self.key(v)
        return "L" + self.key(v)


def _null(p):
    return p is None or (isinstance(p, C.c_void_p) and not p.value)


def _read(p, ctype, shape):
    if _null(p):
        return None
    if 0 in shape:
        return np.zeros(shape, np.ctypeslib.as_ctypes_type(ctype))
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape).copy()


class FakeLib:
    """the thirteen entries: each describes its arguments as "entry:argument,..." ("p" a pointer, "-" NULL, "@k" a host
    array, read while the call is running), writes nothing and returns RMX_OK"""
    def __init__(self, arrays):
        self.arrays, self.calls = arrays, []

    def __getattr__(self, name):
        if name not in ENTRIES:
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(self.describe(name, args))
            return 0
        return entry

    def describe(self, name, args):
        names = ENTRIES[name]
        assert len(args) == len(names), (name, len(args))
        d = dict(zip(names, args))
        W, P, K = d["n_windows"], d["n_pairs"], d.get("integrate", 1)
        shapes = {"pairs": (C.c_int32, (P, 2)),
                  "bounds": (C.c_int32, ((W // K, P, 2) if d.get("bounds_pw") else (P, 2))),
                  "band": (C.c_double, ((W,) if d.get("band_pw") else ()) + ((d["n_bands"],) if "n_bands" in d else ()) + (2,)),
                  "grid": (C.c_double, (d.get("n_dopplers", 0),))}
        out = []
        for n, v in zip(names[1:], args[1:]):
            if n in POINTERS:
                out.append(None if _null(v) else "p")
            elif n in shapes:
                a = _read(v, *shapes[n])
                out.append(None if a is None else self.arrays.key(a))
            else:
                assert isinstance(v, int) and not isinstance(v, bool), (name, n, v)
                out.append(v)
        return name[4:] + ":" + ",".join("-" if v is None else str(v) for v in out)


def make_engine(lib):
    """an XcorrEngine without rmx_create, as the CPU tests build theirs"""
    sys.path.insert(0, ROOT)
    from radio_mapper_amd import xcorr

    class Engine(xcorr.XcorrEngine):
        def __init__(self):
            self.n_buoys, self.n_samples, self.max_windows, self.device, self._lib, self._ctx = B, N, 12, 0, lib, None

        def _check(self, rc):
            assert rc == 0

        def __del__(self):
            pass
    return Engine()


# -- the options ---------------------------------------------------------------------------------------------------------
PAIRS = [(1, 0), (2, 2)]
GRID_CPS = [-0.001, 0.0, 0.001]


def _bounds(kind, rows, P):
    if kind == 0:
        return None
    shared = [[-3 - q, 4 + q] for q in range(P)]
    return shared if kind == 1 else [[[lo - r, hi + r] for lo, hi in shared] for r in range(rows)]


def _band(kind, W):
    if kind == 0:
        return None
    return [-0.25, 0.125] if kind == 1 else [[-0.25 + w / 64.0, 0.125 + w / 64.0] for w in range(W)]


def _bands(kind, W):
    shared = [[-0.5, 0.5], [0.0, 0.25]]
    return shared if kind == 1 else [[[lo + w / 64.0, hi] for lo, hi in shared] for w in range(W)]


def _iq(W, u8, lead=()):
    """windows tagged with their index in the first sample (the stubs read it back)"""
    shape = tuple(lead) + (W,)
    n = int(np.prod(shape))
    if u8:
        iq = np.zeros((n, B, 2 * N), np.uint8)
        iq[:, 0, 0] = np.arange(n)
    else:
        iq = np.zeros((n, B, N), np.complex64)
        iq[:, 0, 0] = np.arange(n)
    return iq.reshape(shape + iq.shape[1:])


def _shapes(out):
    """(4, 3) int32, (4, 3) float32 -> "4x3:i4,4x3:f4" """
    return None if out is None else ",".join("x".join(str(n) for n in a.shape) + ":" + a.dtype.str[1:] for a in out)


def _outcome(arrays, log, fn):
    """fn() -> [the calls, the shapes returned] or {"error": [type, text], "calls": the calls made before it}; `log` is the
    list the fake library appends to"""
    del log[:]
    try:
        out = fn()
    except Exception as e:   # noqa: BLE001  (the table records it)
        return {"error": [type(e).__name__, str(e)], "calls": list(log)}
    return [list(log), _shapes(out)]


# -- 1. XcorrEngine ------------------------------------------------------------------------------------------------------
def engine_combinations():
    for fam in "XBC":
        axes = [("h", "d"), (0, 1), (0, 1), (0, 1, 2), (1, 2) if fam == "B" else (0, 1, 2), (0, 1), (1, 2), (0, 4), (0, 1),
                (0, 1) if fam == "C" else (0,)]
        for combo in itertools.product(*axes):
            yield (fam,) + combo


def engine_call(eng, combo, W=4):
    fam, door, u8, custom, b, d, whiten, K, U, quality, fine = combo
    pairs = PAIRS if custom else None
    P = 2 if custom else 3
    kw = dict(pairs=pairs, lag_bounds=_bounds(b, W // K, P), whiten=bool(whiten), integrate=K, refine=U)
    if fam == "B":
        lead = (_bands(d, W),)
    else:
        lead = (GRID_CPS,) if fam == "C" else ()
        kw["band"] = _band(d, W)
    if door == "h":
        name = {"X": "correlate", "B": "correlate_bands", "C": "caf"}[fam]
        if fam == "C":
            kw["fine"] = bool(fine)
        return getattr(eng, name)(_iq(W, u8), *lead, quality=bool(quality), **kw)
    kw["u8"] = bool(u8)
    if quality:
        kw["quality_ptr"] = 4096
    if fam == "X":
        return eng.correlate_device(64, W, 128, 256, 512, **kw)
    if fam == "B":
        return eng.correlate_bands_device(64, W, lead[0], 128, 256, 512, **kw)
    if fine:
        kw["dop_frac_ptr"] = 2048
    return eng.caf_device(64, W, lead[0], 1024, 128, 256, 512, **kw)


def odd_engine_calls(eng):
    """(name, call): doubly-wrong calls in each method's order of checks, the empty batches, the defaults"""
    iq, lb, bad_lb = _iq(4, 0), _bounds(1, 4, 3), [[0, 1]]
    bands = _bands(1, 4)
    dev = (64, 4, 128, 256, 512)
    return [
        ("correlate:iq+integrate", lambda: eng.correlate(iq[:, :2], integrate=3)),
        ("correlate:integrate+refine", lambda: eng.correlate(iq, integrate=3, refine=3)),
        ("correlate:integrate_none", lambda: eng.correlate(iq, integrate=None)),
        ("correlate:refine+pairs", lambda: eng.correlate(iq, refine=3, pairs=[0, 1, 2])),
        ("correlate:refine_bool", lambda: eng.correlate(iq, refine=False)),
        ("correlate:pairs+bounds", lambda: eng.correlate(iq, pairs=[0, 1, 2], lag_bounds=bad_lb)),
        ("correlate:bounds+band", lambda: eng.correlate(iq, lag_bounds=bad_lb, band=[0.3, 0.1])),
        ("correlate:bounds_per_window_under_integrate", lambda: eng.correlate(iq, lag_bounds=_bounds(2, 4, 3), integrate=2)),
        ("correlate:band_nan", lambda: eng.correlate(iq, band=[float("nan"), 0.1])),
        ("correlate_device:integrate+refine", lambda: eng.correlate_device(*dev, integrate=3, refine=3)),
        ("correlate_device:refine_bool", lambda: eng.correlate_device(*dev, refine=False)),
        ("correlate_device:bounds+band", lambda: eng.correlate_device(*dev, lag_bounds=bad_lb, band=[0.3, 0.1])),
        ("correlate_bands:iq+bands", lambda: eng.correlate_bands(iq[0], None)),
        ("correlate_bands:integrate+refine", lambda: eng.correlate_bands(iq, bands, integrate=3, refine=3)),
        ("correlate_bands:refine+bands", lambda: eng.correlate_bands(iq, None, refine=3)),
        ("correlate_bands:pairs+bands", lambda: eng.correlate_bands(iq, None, pairs=[0, 1, 2])),
        ("correlate_bands:bands+bounds", lambda: eng.correlate_bands(iq, [[0.3, 0.1]], lag_bounds=bad_lb)),
        ("correlate_bands:65_bands", lambda: eng.correlate_bands(iq, [[0.0, 0.1]] * 65)),
        ("correlate_bands_device:refine+bands", lambda: eng.correlate_bands_device(64, 4, None, 128, 256, 512, refine=3)),
        ("correlate_bands_device:bands+bounds", lambda: eng.correlate_bands_device(64, 4, [[0.3, 0.1]], 128, 256, 512, lag_bounds=bad_lb)),
        ("caf:integrate+refine", lambda: eng.caf(iq, GRID_CPS, integrate=3, refine=3)),
        ("caf:integrate_none_refine", lambda: eng.caf(iq, GRID_CPS, integrate=None, refine=3)),
        ("caf:integrate_bool", lambda: eng.caf(iq, GRID_CPS, integrate=True)),
        ("caf:refine+pairs", lambda: eng.caf(iq, GRID_CPS, refine=3, pairs=[0, 1, 2])),
        ("caf:pairs+grid", lambda: eng.caf(iq, ["x"], pairs=[0, 1, 2])),
        ("caf:grid+bounds", lambda: eng.caf(iq, ["x"], lag_bounds=bad_lb)),
        ("caf:bounds+band", lambda: eng.caf(iq, GRID_CPS, lag_bounds=bad_lb, band=[0.3, 0.1])),
        ("caf:grid_2d", lambda: eng.caf(iq, [GRID_CPS, GRID_CPS])),
        ("caf_device:refine+integrate", lambda: eng.caf_device(64, 4, GRID_CPS, 1024, 128, 256, 512, refine=3, integrate=3)),
        ("caf_device:refine_false", lambda: eng.caf_device(64, 4, GRID_CPS, 1024, 128, 256, 512, refine=False)),
        ("caf_device:refine_false_with_bounds", lambda: eng.caf_device(64, 4, GRID_CPS, 1024, 128, 256, 512, refine=False, lag_bounds=lb)),
        ("caf_device:integrate_1", lambda: eng.caf_device(64, 4, GRID_CPS, 1024, 128, 256, 512, integrate=1)),
        ("caf_device:bounds+band", lambda: eng.caf_device(64, 4, GRID_CPS, 1024, 128, 256, 512, lag_bounds=bad_lb, band=[0.3, 0.1])),
        ("correlate_bands_device:quality_ptr_0", lambda: eng.correlate_bands_device(64, 4, bands, 128, 256, 512, quality_ptr=0)),
        ("correlate_device:integrate_true", lambda: eng.correlate_device(*dev, integrate=True)),
        ("correlate_device:refine_0.0", lambda: eng.correlate_device(*dev, refine=0.0)),
        ("correlate_device:whiten_0", lambda: eng.correlate_device(*dev, whiten=0)),
        ("caf_device:whiten_1", lambda: eng.caf_device(64, 4, GRID_CPS, 1024, 128, 256, 512, whiten=1)),
        # the defaults
        ("correlate:defaults", lambda: eng.correlate(iq)),
        ("correlate_device:defaults", lambda: eng.correlate_device(*dev)),
        ("correlate_bands:defaults", lambda: eng.correlate_bands(iq, bands)),
        ("correlate_bands_device:defaults", lambda: eng.correlate_bands_device(64, 4, bands, 128, 256, 512)),
        ("caf:defaults", lambda: eng.caf(iq, GRID_CPS)),
        ("caf_device:defaults", lambda: eng.caf_device(64, 4, GRID_CPS, 1024, 128, 256, 512)),
        # the empty batches: a host-array method makes no call, a device-pointer method does not short-circuit
        ("correlate:no_windows", lambda: eng.correlate(iq[:0], quality=True, lag_bounds=lb)),
        ("correlate:no_pairs", lambda: eng.correlate(iq, pairs=[], integrate=2)),
        ("correlate_bands:no_windows", lambda: eng.correlate_bands(iq[:0], bands, quality=True, refine=4)),
        ("correlate_bands:no_pairs", lambda: eng.correlate_bands(iq, bands, pairs=[], integrate=2)),
        ("caf:no_windows", lambda: eng.caf(iq[:0], GRID_CPS, fine=True, quality=True)),
        ("caf:no_pairs", lambda: eng.caf(iq, GRID_CPS, pairs=[], integrate=2)),
        ("correlate_device:no_windows", lambda: eng.correlate_device(64, 0, 128, 256, 512, lag_bounds=lb)),
        ("correlate_device:no_pairs", lambda: eng.correlate_device(*dev, pairs=[])),
        ("correlate_bands_device:no_windows", lambda: eng.correlate_bands_device(64, 0, bands, 128, 256, 512)),
        ("caf_device:no_windows", lambda: eng.caf_device(64, 0, GRID_CPS, 1024, 128, 256, 512)),
        ("caf_device:no_pairs", lambda: eng.caf_device(64, 4, GRID_CPS, 1024, 128, 256, 512, pairs=[], band=[-0.1, 0.1])),
    ]


# -- 3. the stub engine of MultiXcorrEngine and TDoACalculator -----------------------------------------------------------
SIGNATURES = {"correlate": ("iq", "pairs", "lag_bounds", "band", "whiten", "integrate", "refine", "quality"),
              "correlate_bands": ("iq", "bands", "pairs", "lag_bounds", "whiten", "refine", "quality", "integrate"),
              "caf": ("iq", "doppler_cps", "pairs", "lag_bounds", "band", "whiten", "fine", "refine", "quality", "integrate")}


class StubEngine:
    """records [device, method, [first window, windows], "the positional arguments behind iq|the keyword arguments"] and answers
    with lag_int = 1000 * (the group's first window) + pair, so that a gather in the wrong order shows"""
    arrays = None
    cap = None          # max_windows of every engine, whatever the factory is given

    def __init__(self, n_buoys=B, n_samples=N, max_windows=12, device=0):
        self.max_windows = StubEngine.cap or max_windows
        self.device, self.made, self.log = device, [n_buoys, n_samples, max_windows, device], []

    def _answer(self, method, a, kw):
        v = dict(zip(SIGNATURES[method], a))
        assert not set(v) & set(kw) and set(kw) <= set(SIGNATURES[method]), (method, kw)
        v.update(kw)
        iq = np.asarray(v["iq"])
        tags = np.abs(iq[:, 0, 0]).astype(np.int32)
        self.log.append((method, [int(tags[0]) if len(tags) else -1, len(tags)], a[1:], dict(kw)))
        K = v.get("integrate") or 1
        P = B * (B - 1) // 2 if v.get("pairs") is None else len(v["pairs"])
        mid = (np.asarray(v["bands"]).shape[-2],) if method == "correlate_bands" else ()
        shape = (len(tags) // K,) + mid + (P,)
        li = np.zeros(shape, np.int32)
        li += (1000 * tags[::K]).reshape((-1,) + (1,) * (len(shape) - 1)) + np.arange(P, dtype=np.int32)
        out = (li, np.zeros(shape, np.float32), np.ones(shape, np.float32))
        if method == "caf":
            out = (np.zeros(shape, np.int32),) + ((np.zeros(shape, np.float32),) if v.get("fine") else ()) + out
        return out + ((np.full(shape + (4,), 0.5, np.float32),) if v.get("quality") else ())

    def calls(self):
        """the log, written out (by the caller's thread, after the workers are done: the arrays' keys follow the order of
        the table, not of the threads)"""
        val = StubEngine.arrays.value
        return [c if isinstance(c, list) else
                [self.device, c[0], c[1], ",".join(str(val(x)) for x in c[2]) + "|" + ",".join(f"{k}={val(x)}" for k, x in sorted(c[3].items()))]
                for c in self.log]

    def correlate(self, *a, **kw):
        return self._answer("correlate", a, kw)

    def correlate_bands(self, *a, **kw):
        return self._answer("correlate_bands", a, kw)

    def caf(self, *a, **kw):
        return self._answer("caf", a, kw)

    def close(self):
        pass


def _gathered(out):
    """shapes and dtypes of a gathered result, and its int32 arrays' first pair (the order of the rows)"""
    return [[_shapes([a])] + ([StubEngine.arrays.key(a[(slice(None),) + (0,) * (a.ndim - 1)])] if a.dtype == np.int32 else [])
            for a in out]


def multi_combinations():
    for fam in "XBC":
        axes = [(0, 1, 2), (1, 2) if fam == "B" else (0, 1, 2), (0, 1), (1, 2, 3), (0, 4), (0, 1), (0, 1) if fam == "C" else (0,)]
        for combo in itertools.product(*axes):
            yield (fam, 0, 0) + combo
    for fam in "XBC":   # custom pairs, uint8 input, engines of two windows: the stepping loop under K = 2
        for custom, u8, cap in ((1, 0, 0), (0, 1, 0), (0, 0, 2), (1, 1, 2)):
            for K in (1, 2):
                yield (fam, custom + 2 * u8, cap, 2, 2, 1, K, 4, 1, 1 if fam == "C" else 0)


def multi_call(combo, W=12):
    """-> (the calls of the three engines in device order, the gathered result)"""
    sys.path.insert(0, ROOT)
    from radio_mapper_amd import multi
    fam, inp, cap, b, d, whiten, K, U, quality, fine = combo
    custom, u8 = inp & 1, inp >> 1
    StubEngine.cap = cap or None
    try:
        m = multi.MultiXcorrEngine(B, N, W, devices=[0, 1, 2], engine_factory=StubEngine)
    finally:
        StubEngine.cap = None
    pairs = PAIRS if custom else None
    kw = dict(pairs=pairs, lag_bounds=_bounds(b, W // K, 2 if custom else 3), whiten=bool(whiten), integrate=K, refine=U,
              quality=bool(quality))
    try:
        if fam == "X":
            out = m.correlate(_iq(W, u8), band=_band(d, W), **kw)
        elif fam == "B":
            out = m.correlate_bands(_iq(W, u8), _bands(d, W), **kw)
        else:
            out = m.caf(_iq(W, u8), GRID_CPS, band=_band(d, W), fine=bool(fine), **kw)
        return [c for e in m._engines for c in e.calls()], out
    finally:
        m.close()


def odd_multi_calls():
    sys.path.insert(0, ROOT)
    from radio_mapper_amd import multi

    def run(fn, W=12, cap=None):
        StubEngine.cap = cap
        try:
            m = multi.MultiXcorrEngine(B, N, W, devices=[0, 1, 2], engine_factory=StubEngine)
        finally:
            StubEngine.cap = None
        try:
            out = fn(m)
            return [c for e in m._engines for c in e.calls()], out
        finally:
            m.close()
    iq, bands, bad_lb = _iq(12, 0), _bands(1, 12), [[0, 1]]
    return [
        ("multi.correlate:defaults", lambda: run(lambda m: m.correlate(iq))),
        ("multi.correlate:whiten_1", lambda: run(lambda m: m.correlate(iq, whiten=1))),
        ("multi.correlate_bands:defaults", lambda: run(lambda m: m.correlate_bands(iq, bands))),
        ("multi.caf:defaults", lambda: run(lambda m: m.caf(iq, GRID_CPS))),
        ("multi.caf:integrate_1", lambda: run(lambda m: m.caf(iq, GRID_CPS, integrate=1))),
        ("multi.caf:integrate_2_only", lambda: run(lambda m: m.caf(iq, GRID_CPS, integrate=2))),
        ("multi.caf:fine_only", lambda: run(lambda m: m.caf(iq, GRID_CPS, fine=True))),
        ("multi.correlate:5_windows", lambda: run(lambda m: m.correlate(iq[:5], lag_bounds=_bounds(2, 5, 3)))),
        ("multi.correlate:2_windows", lambda: run(lambda m: m.correlate(iq[:2], band=_band(2, 2)))),
        ("multi.correlate:no_windows", lambda: run(lambda m: m.correlate(iq[:0], quality=True))),
        ("multi.correlate_bands:no_windows", lambda: run(lambda m: m.correlate_bands(iq[:0], bands, integrate=2))),
        ("multi.caf:no_windows", lambda: run(lambda m: m.caf(iq[:0], GRID_CPS, fine=True, quality=True))),
        ("multi.correlate:too_many_windows", lambda: run(lambda m: m.correlate(iq), W=8)),
        ("multi.correlate:iq+integrate", lambda: run(lambda m: m.correlate(iq[0], integrate=5))),
        ("multi.correlate:pairs+integrate", lambda: run(lambda m: m.correlate(iq, pairs=[0, 1, 2], integrate=5))),
        ("multi.correlate:integrate+refine", lambda: run(lambda m: m.correlate(iq, integrate=5, refine=3))),
        ("multi.correlate:refine+bounds", lambda: run(lambda m: m.correlate(iq, refine=3, lag_bounds=bad_lb))),
        ("multi.correlate:bounds+band", lambda: run(lambda m: m.correlate(iq, lag_bounds=bad_lb, band=[0.3, 0.1]))),
        ("multi.correlate:bounds+band_integrated", lambda: run(lambda m: m.correlate(iq, lag_bounds=bad_lb, band=[0.3, 0.1], integrate=2))),
        ("multi.correlate:group_larger_than_an_engine", lambda: run(lambda m: m.correlate(iq, integrate=3), cap=2)),
        ("multi.correlate_bands:integrate+bands", lambda: run(lambda m: m.correlate_bands(iq, None, integrate=5))),
        ("multi.correlate_bands:bands+bounds", lambda: run(lambda m: m.correlate_bands(iq, None, lag_bounds=bad_lb))),
        ("multi.correlate_bands:bounds+refine", lambda: run(lambda m: m.correlate_bands(iq, bands, lag_bounds=bad_lb, refine=3))),
        ("multi.correlate_bands:bands+refine", lambda: run(lambda m: m.correlate_bands(iq, None, refine=3))),
        ("multi.correlate_bands:group_larger_than_an_engine", lambda: run(lambda m: m.correlate_bands(iq, bands, integrate=3), cap=2)),
        ("multi.caf:integrate+refine", lambda: run(lambda m: m.caf(iq, GRID_CPS, integrate=5, refine=3))),
        ("multi.caf:integrate_none_refine", lambda: run(lambda m: m.caf(iq, GRID_CPS, refine=3, lag_bounds=bad_lb))),
        ("multi.caf:bounds+band", lambda: run(lambda m: m.caf(iq, GRID_CPS, lag_bounds=bad_lb, band=[0.3, 0.1]))),
        ("multi.caf:group_larger_than_an_engine", lambda: run(lambda m: m.caf(iq, GRID_CPS, integrate=3), cap=2)),
    ]


def calculator_combinations():
    for chan in (0, 1):
        for combo in itertools.product((0, 1, 2), (0, 1, 2), (0, 1), (1, 2), (0, 4), (0, 1)):
            yield ("lags", chan) + combo
        for combo in itertools.product((0, 1, 2), (0, 1, 2), (0, 1)):
            yield ("doppler", chan) + combo + (1, 0, 0)
        for combo in itertools.product((0, 1, 2), (0, 1)):
            yield ("lags_bands", chan, combo[0], 2, combo[1], 1, 0, 0)
        for combo in itertools.product((0, 1, 2), (0, 1), (1, 2), (0, 4), (0, 1)):
            yield ("band_lags", chan, combo[0], 2) + combo[1:]


def _calculator(eng):
    sys.path.insert(0, ROOT)
    from radio_mapper_amd import tdoa_processor as tp
    calc = tp.TDoACalculator()
    calc._engine = lambda b, n, w=1: eng.log.append(["_engine", b, n, w]) or eng
    return calc


def calculator_call(combo, C_=2, W=6):
    """-> (the engine's calls, the result); with a channel axis [C][W]... of 2 x 6 windows, else 6 windows"""
    kind, chan, b, d, whiten, K, U, quality = combo
    eng = StubEngine()
    calc = _calculator(eng)
    lead = (C_,) if chan else ()

    def fold(rows_of, value):   # a per-row option with the channel axis in front
        return None if value is None else (np.asarray(value).reshape(lead + (rows_of,) + np.asarray(value).shape[1:]) if chan else value)
    total = C_ * W if chan else W
    lb = _bounds(b, total // K, 3)
    lb = fold(W // K, lb) if b == 2 else lb
    iq = _iq(W, 0, lead)
    if kind == "band_lags" or kind == "lags_bands":
        bands = fold(W, _bands(2, total))
        if kind == "lags_bands":
            out = calc.measure_lags(iq, lag_bounds=lb, whiten=bool(whiten), bands=bands)
        else:
            out = calc.measure_band_lags(iq, bands, lag_bounds=lb, whiten=bool(whiten), refine=U, quality=bool(quality), integrate=K)
    else:
        band = _band(d, total)
        band = fold(W, band) if d == 2 else band
        more = {"doppler_cps": GRID_CPS} if kind == "doppler" else {"integrate": K, "refine": U, "quality": bool(quality)}
        out = calc.measure_lags(iq, lag_bounds=lb, band=band, whiten=bool(whiten), **more)
    return eng.calls(), out


def odd_calculator_calls():
    def run(fn):
        eng = StubEngine()
        out = fn(_calculator(eng))
        return eng.calls(), out
    iq, chan, bands = _iq(6, 0), _iq(6, 0, (2,)), _bands(2, 6)

    def seam(fn, **settings):   # _measure_groups / _measure_shared of a calculator with these settings, on two groups of 32 samples
        def call(c):
            for k, v in settings.items():
                setattr(c, k, v)
            out = fn(c, np.arange(2 * B * 32, dtype=np.complex64).reshape(2, B, 32))
            return (out,) if isinstance(out, np.ndarray) else out
        return lambda: run(call)
    glb, gband, gbands = np.asarray(_bounds(2, 2, 3)), np.asarray(_band(2, 2)), np.asarray(_bands(2, 2))
    return [
        ("calc._measure_groups:plain", seam(lambda c, x: c._measure_groups(x))),
        ("calc._measure_groups:bounds_band", seam(lambda c, x: c._measure_groups(x, glb, gband), whiten=True)),
        ("calc._measure_groups:integrate_2", seam(lambda c, x: c._measure_groups(x, glb, gband), integrate=2)),
        ("calc._measure_groups:integrate_2_refine_quality", seam(lambda c, x: c._measure_groups(x, None, gband, with_quality=True),
                                                                 integrate=2, refine=4, whiten=True)),
        ("calc._measure_groups:doppler", seam(lambda c, x: c._measure_groups(x, glb, None, fs=1e4), doppler_search_hz=(200.0, 100.0))),
        ("calc._measure_shared:plain", seam(lambda c, x: c._measure_shared(x, glb, gbands))),
        ("calc._measure_shared:refine", seam(lambda c, x: c._measure_shared(x, None, gbands), refine=4, whiten=True)),
        ("calc._measure_shared:integrate_2", seam(lambda c, x: c._measure_shared(x, glb, gbands), integrate=2)),
        ("calc._measure_shared:integrate_2_quality", seam(lambda c, x: c._measure_shared(x, glb, gbands, with_quality=True), integrate=2)),

        ("calc.measure_lags:defaults", lambda: run(lambda c: c.measure_lags(iq))),
        ("calc.measure_lags:pairs", lambda: run(lambda c: c.measure_lags(iq, PAIRS))),
        ("calc.measure_lags:uint8_channels", lambda: run(lambda c: c.measure_lags(_iq(6, 1, (2,)), PAIRS, whiten=1))),
        ("calc.measure_lags:bounds_only", lambda: run(lambda c: c.measure_lags(iq, lag_bounds=_bounds(1, 6, 3)))),
        ("calc.measure_band_lags:defaults", lambda: run(lambda c: c.measure_band_lags(iq, bands))),
        ("calc.measure_lags:no_windows", lambda: run(lambda c: c.measure_lags(iq[:0]))),
        ("calc.measure_lags:refine+bands", lambda: run(lambda c: c.measure_lags(iq, refine=3, bands=bands, band=[0.1, 0.2]))),
        ("calc.measure_lags:iq_2d", lambda: run(lambda c: c.measure_lags(iq[0], integrate=4))),
        ("calc.measure_lags:integrate_per_channel", lambda: run(lambda c: c.measure_lags(chan, integrate=4))),
        ("calc.measure_lags:bands_2d", lambda: run(lambda c: c.measure_lags(iq, bands=bands[0]))),
        ("calc.measure_band_lags:refine+iq", lambda: run(lambda c: c.measure_band_lags(iq[0], bands, refine=3))),
        ("calc.measure_band_lags:iq+integrate", lambda: run(lambda c: c.measure_band_lags(iq[0], bands, integrate=4))),
        ("calc.measure_band_lags:integrate_per_channel", lambda: run(lambda c: c.measure_band_lags(chan, _bands(2, 12), integrate=4))),
        ("calc.measure_band_lags:bands_2d", lambda: run(lambda c: c.measure_band_lags(iq, bands[0]))),
    ] + [("calc.measure_lags:bands+%s" % k, lambda kw=kw: run(lambda c: c.measure_lags(iq, bands=bands, **kw)))
         for k, kw in (("band", {"band": [0.1, 0.2]}), ("integrate", {"integrate": 2}), ("refine", {"refine": 4}),
                       ("quality", {"quality": True}), ("doppler_cps", {"doppler_cps": GRID_CPS}))] \
      + [("calc.measure_lags:doppler_cps+%s" % k, lambda kw=kw: run(lambda c: c.measure_lags(iq, doppler_cps=GRID_CPS, **kw)))
         for k, kw in (("integrate", {"integrate": 2}), ("refine", {"refine": 4}), ("quality", {"quality": True}))]


# -- the walk ------------------------------------------------------------------------------------------------------------
def names():
    """the rows of the table, in order"""
    out = ["".join(str(c) for c in combo) for combo in engine_combinations()]
    out += [n for n, _ in odd_engine_calls(None)]
    out += ["multi." + "".join(str(c) for c in combo) for combo in multi_combinations()]
    out += [n for n, _ in odd_multi_calls()]
    out += ["calc." + ".".join(str(c) for c in combo) for combo in calculator_combinations()]
    out += [n for n, _ in odd_calculator_calls()]
    assert len(set(out)) == len(out)
    return out


def walk():
    """-> {"name": NAME, "arrays": {key: [dtype, shape, values]}, "rows": [[name, [calls, returns] or {"error": ...}], ...]}"""
    arrays = Arrays()
    StubEngine.arrays = arrays
    lib = FakeLib(arrays)
    eng = make_engine(lib)
    rows = []
    for combo in engine_combinations():
        rows.append(["".join(str(c) for c in combo), _outcome(arrays, lib.calls, lambda: engine_call(eng, combo))])
    for name, fn in odd_engine_calls(eng):
        rows.append([name, _outcome(arrays, lib.calls, fn)])

    def stubbed(name, fn):
        try:
            calls, out = fn()
        except Exception as e:   # noqa: BLE001  (the table records it)
            return [name, {"error": [type(e).__name__, str(e)]}]
        return [name, [calls, _gathered(out)]]
    for combo in multi_combinations():
        rows.append(stubbed("multi." + "".join(str(c) for c in combo), lambda: multi_call(combo)))
    for name, fn in odd_multi_calls():
        rows.append(stubbed(name, fn))
    for combo in calculator_combinations():
        rows.append(stubbed("calc." + ".".join(str(c) for c in combo), lambda: calculator_call(combo)))
    for name, fn in odd_calculator_calls():
        rows.append(stubbed(name, fn))
    return {"name": NAME, "arrays": arrays.table, "rows": rows}


def _block(name):
    """the cross product a row belongs to, None for the rows that are written out"""
    return None if ":" in name else "multi" if name.startswith("multi.") else "calc" if name.startswith("calc.") else "engine"


def _digest(value, n=10):
    return hashlib.sha256(json.dumps(value, separators=(",", ":")).encode()).hexdigest()[:n]


def compact(table):
    """The table as it is stored.  The three cross products are thousands of rows that differ in one argument each: per
    cross product the number of rows, a digest of their names (so that none can drop out) and, in the order of names(), a
    10-digit SHA-256 digest of each row's outcome.  The rows a reader wants to read -- the wrong and doubly-wrong calls with
    their texts, the defaults, the empty batches, the seam -- are written out, and so is every array."""
    out = {"name": table["name"], "arrays": table["arrays"], "combinations": {}, "rows": []}
    for name, outcome in table["rows"]:
        if _block(name) is None:
            out["rows"].append([name, outcome])
        else:
            c = out["combinations"].setdefault(_block(name), {"names": [], "outcomes": []})
            c["names"].append(name)
            c["outcomes"].append(_digest(outcome))
    for c in out["combinations"].values():
        c["count"], c["names"] = len(c["names"]), _digest(c["names"], 16)
    return out


def main(out_path):
    if os.path.exists(out_path):
        sys.exit(f"{out_path} exists: a recorded table is not overwritten (move it away first)")
    table = walk()
    assert [r[0] for r in table["rows"]] == names()
    stored = compact(table)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write('{"name": %s,\n"arrays": {\n' % json.dumps(stored["name"]))
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in stored["arrays"].items()))
        f.write('\n},\n"combinations": {\n')
        blocks = []
        for k, c in stored["combinations"].items():   # 24 digests per line, as one string
            lines = [" ".join(c["outcomes"][i:i + 24]) for i in range(0, c["count"], 24)]
            blocks.append('%s: {"count": %d, "names": "%s", "outcomes": [\n%s\n]}'
                          % (json.dumps(k), c["count"], c["names"], ",\n".join(json.dumps(ln) for ln in lines)))
        f.write(",\n".join(blocks))
        f.write('\n},\n"rows": [\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in stored["rows"]))
        f.write("\n]}\n")
    errors = sum(isinstance(r[1], dict) for r in table["rows"])
    print(f"{len(table['rows'])} rows ({errors} of them exceptions), {len(table['arrays'])} arrays -> {out_path}", flush=True)
    return 0


def load(path=TABLE):
    """a stored table, the lines of digests split up again: the form compact() returns"""
    with open(path) as f:
        t = json.load(f)
    for c in t["combinations"].values():
        c["outcomes"] = [d for line in c["outcomes"] for d in line.split()]
    return t


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
