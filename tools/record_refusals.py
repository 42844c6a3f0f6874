"""GPU box: what the ten correlation and Doppler-search entries of the C ABI answer to bad, doubly bad and empty calls --
the behaviour pin of the checked request (radio-mapper_amd/csrc/host_request.hpp: check_request).  Runs a fixed list of at
most 200 small calls (3 buoys, N = 256, 4 windows) through ctypes and writes, per call, the arguments by name, rc, the full
rmx_last_error text of a refused call and whether the 77-filled outputs stayed untouched.  Per entry: one good control,
each single refusal, calls bad in two adjacent classes of the promised order (include/rmx.h: "Refusals ..., in this
order"), the empty batches.

usage: RMX_LIBRARY=<library of the commit the table pins> python tools/record_refusals.py OUT.json
       Record with the library of the commit BEFORE a change to the checks, never with the changed one; an existing
       OUT.json is not overwritten.  tests/test_gpu_request_refusals.py replays tests/golden/request_refusals.json on the
       tree's library."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "request_refusals.json")
B, N, W, M, P = 3, 256, 4, 3, 3
FILL = 77
SLOTS = W * M * P          # every output buffer holds the largest call's slots (quality: four times that)

BAND = [-0.2, 0.3]
SET = [[-0.5, 0.5], [0.0, 0.25], [-0.1, 0.1]]
LB = [[-30, 30]] * P
DOP = [-1e-4, 0.0, 1e-4]
# the arguments of each entry, in the order of include/rmx.h, with a good value each ("own": a buffer of its own)
COMMON = dict(iq="own", n_windows=W, pairs=None, n_pairs=P)
OUTS = dict(lag_int="own", lag_frac="own", peak="own")
WEIGHT = dict(band_cps=None, band_per_window=0, weighting=0, lag_bounds=None, bounds_per_window=0)
SETS = dict(band_cps=SET, n_bands=M, band_per_window=0, weighting=0, lag_bounds=None, bounds_per_window=0)
ENTRIES = {
    "rmx_xcorr_batch": {**COMMON, **OUTS},
    "rmx_xcorr_batch_bounded": {**COMMON, "lag_bounds": LB, "bounds_per_window": 0, **OUTS},
    "rmx_xcorr_batch_weighted": {**COMMON, **WEIGHT, "band_cps": BAND, "weighting": 1, **OUTS},
    "rmx_xcorr_batch_bands": {**COMMON, **SETS, **OUTS},
    "rmx_xcorr_batch_integrated": {**COMMON, "integrate": 2, **WEIGHT, **OUTS},
    "rmx_xcorr_batch_refined": {**COMMON, "integrate": 1, **WEIGHT, "refine": 4, **OUTS},
    "rmx_xcorr_batch_quality": {**COMMON, "integrate": 2, **WEIGHT, "weighting": 1, "refine": 4, **OUTS, "quality": "own"},
    "rmx_xcorr_batch_bands_quality": {**COMMON, **SETS, "refine": 4, **OUTS, "quality": "own"},
    "rmx_caf_batch": {**COMMON, "doppler_cps": DOP, "n_dopplers": 3, "dop_idx": "own", **OUTS},
    "rmx_caf_batch_request": {**COMMON, "doppler_cps": DOP, "n_dopplers": 3, **WEIGHT, "band_cps": BAND, "weighting": 1,
                              "lag_bounds": LB, "dop_idx": "own", "dop_frac": "own", **OUTS},
}
POINTERS = ("iq", "lag_int", "lag_frac", "peak", "quality", "dop_idx", "dop_frac")


def _per_window(rows, bad_at, bad):
    out = [list(r) if isinstance(r[0], (int, float)) else [list(x) for x in r] for r in rows]
    k = out
    for i in bad_at[:-1]:
        k = k[i]
    k[bad_at[-1]] = bad
    return out


def cases():
    out = []

    def add(entry, name, **change):
        args = dict(ENTRIES[entry])
        assert set(change) <= set(args), (entry, change)
        args.update(change)
        out.append(dict(name=f"{entry[4:]}:{name}", entry=entry, args=args))

    bad_lb = _per_window(LB, (1,), [7, 6])
    bad_lbw = _per_window([LB] * W, (1, 2), [0, N])
    bad_lbg = _per_window([LB] * 2, (1, 2), [-N, 0])
    nan_bands = _per_window([BAND] * W, (2,), ["nan", 0.1])
    bad_set = _per_window(SET, (1,), [0.3, -0.2])
    bad_setw = _per_window([SET] * W, (2, 1), [0.5, 0.5])
    one_pair = [[0, 2]]
    for e, good in ENTRIES.items():
        caf = "doppler_cps" in good
        banded = "n_bands" in good
        grouped = "integrate" in good
        weighted = "weighting" in good
        bounds = "lag_bounds" in good
        over = {"refine": 3, "quality": "on:peak:0"} if "quality" in good else {"refine": 3} if "refine" in good else {}
        add(e, "control")
        # ---- single refusals -------------------------------------------------------------------------------------------
        add(e, "iq_null", iq=None)
        if e in ("rmx_xcorr_batch", "rmx_caf_batch_request"):
            add(e, "peak_null", peak=None)
        add(e, "too_many_windows", n_windows=W + 1)
        add(e, "default_list_of_2", n_pairs=2)
        if e in ("rmx_xcorr_batch", "rmx_xcorr_batch_quality", "rmx_caf_batch"):
            add(e, "negative_pairs", pairs=one_pair, n_pairs=-1)
        if caf:
            add(e, "no_dopplers", n_dopplers=0)
        if e == "rmx_caf_batch":
            add(e, "dop_idx_null", dop_idx=None)
            add(e, "grid_null", doppler_cps=None)
            add(e, "pair_out_of_range", pairs=[[0, 3]], n_pairs=1)
            add(e, "no_dopplers+too_many_windows", n_dopplers=4097, n_windows=W + 1)
        if e == "rmx_xcorr_batch_bounded":
            add(e, "bounds_null", lag_bounds=None)
            add(e, "bounds_null+too_many_windows", lag_bounds=None, n_windows=W + 1)
        if grouped:
            add(e, "integrate_3", integrate=3)
            add(e, "integrate_3+iq_null", integrate=3, iq=None)
            add(e, "integrate_2_negative_pairs+iq_null", integrate=2, pairs=one_pair, n_pairs=-1, iq=None)
            if e == "rmx_xcorr_batch_integrated":
                add(e, "integrate_0", integrate=0)
                add(e, "integrate_1_negative_pairs+iq_null", integrate=1, pairs=one_pair, n_pairs=-1, iq=None)
        if banded:
            add(e, "n_bands_0", n_bands=0)
            if e == "rmx_xcorr_batch_bands":
                add(e, "bands_null", band_cps=None)
                add(e, "n_bands_65", n_bands=65)
                add(e, "one_band_bad", band_cps=[[1e-9, 2e-9]], n_bands=1)
            add(e, "bands_null+n_bands_0", band_cps=None, n_bands=0, **over)
            add(e, "n_bands_0+weighting", n_bands=0, weighting=7, **over)
            add(e, "bad_band_shared", band_cps=bad_set)
            add(e, "bad_band_per_window", band_cps=bad_setw, band_per_window=1)
            add(e, "one_band_bad_per_window", band_cps=[[b] for b in nan_bands], n_bands=1, band_per_window=1, **over)
            add(e, "weighting+bad_band", weighting=7, band_cps=bad_set, **over)
            add(e, "bad_band+default_list_of_2", band_cps=bad_set, n_pairs=2, **over)
        if weighted:
            add(e, "weighting_7", weighting=7)
            first = e in ("rmx_xcorr_batch_weighted", "rmx_caf_batch_request")   # (the entries behind take the same arguments)
            if first or banded:
                add(e, "weighting+too_many_windows", weighting=7, n_windows=W + 1)
            if not banded:
                add(e, "bad_band", band_cps=[0.3, -0.2])
                add(e, "weighting+bad_band", weighting=7, band_cps=[0.3, -0.2], lag_bounds=bad_lb)
                if first:
                    add(e, "thin_band", band_cps=[0.1 / N, 0.2 / N])
                    add(e, "nan_band_per_window", band_cps=nan_bands, band_per_window=1)
                    add(e, "too_many_windows+bad_band", n_windows=W + 1, band_cps=[0.3, -0.2])
                    add(e, "bad_band+bad_bounds", band_cps=[0.3, -0.2], lag_bounds=bad_lb)
                if e in ("rmx_xcorr_batch_weighted", "rmx_xcorr_batch_quality"):
                    add(e, "bad_band+default_list_of_2", band_cps=[0.3, -0.2], n_pairs=2)
        if bounds:
            add(e, "bad_bounds_shared", lag_bounds=bad_lb)
            if grouped and good["integrate"] > 1:
                add(e, "bad_bounds_per_group", lag_bounds=bad_lbg, bounds_per_window=1)
            else:
                add(e, "bad_bounds_per_window", lag_bounds=bad_lbw, bounds_per_window=1)
            if not caf:
                add(e, "default_list_of_2+bad_bounds", n_pairs=2, lag_bounds=bad_lb)
        if "refine" in good:
            add(e, "refine_3", refine=3)
            add(e, "bad_bounds+refine", lag_bounds=bad_lb, **over)
        if "quality" in good:
            for name in ("lag_int", "lag_frac", "peak"):
                add(e, f"quality_on_{name}", quality=f"on:{name}:0")
            add(e, "quality_on_the_last_of_peak", quality=f"on:peak:{(W // good.get('integrate', 1)) * (M if banded else 1) * P - 1}")
            add(e, "peak_on_the_last_of_quality", peak=f"on:quality:{4 * (W // good.get('integrate', 1)) * (M if banded else 1) * P - 1}")
            add(e, "refine+quality_on_peak", **over)
            add(e, "quality_null", quality=None)
        if "dop_frac" in good:
            add(e, "pair_out_of_range+weighting", pairs=[[0, 3]], n_pairs=1, weighting=7)
            add(e, "no_dopplers+weighting", n_dopplers=0, weighting=7)
            for name in ("dop_idx", "lag_int", "lag_frac", "peak"):
                add(e, f"dop_frac_on_{name}", dop_frac=f"on:{name}:0")
            add(e, "bad_bounds+dop_frac_on_peak", lag_bounds=bad_lb, dop_frac="on:peak:0")
            add(e, "dop_frac_null", dop_frac=None)
        # ---- the empty batches --------------------------------------------------------------------------------------------
        add(e, "no_windows", n_windows=0)
        add(e, "no_windows_default_list_of_2", n_windows=0, n_pairs=2)
        add(e, "no_pairs", pairs=one_pair, n_pairs=0)
    add("rmx_xcorr_batch_weighted", "full_band_no_windows_default_list_of_2", band_cps=[-0.5, 0.5], weighting=0, n_windows=0, n_pairs=2)
    add("rmx_xcorr_batch_bands", "one_full_band_no_windows_default_list_of_2", band_cps=[[-0.5, 0.5]], n_bands=1, n_windows=0, n_pairs=2)
    add("rmx_xcorr_batch_bands", "one_band_no_windows_default_list_of_2", band_cps=[BAND], n_bands=1, n_windows=0, n_pairs=2)
    add("rmx_xcorr_batch_bands_quality", "one_band_control", band_cps=[[b] for b in [BAND] * W], n_bands=1, band_per_window=1,
        lag_bounds=[LB] * W, bounds_per_window=1)
    add("rmx_xcorr_batch_bands_quality", "per_window_control", band_cps=[SET] * W, band_per_window=1, weighting=1,
        lag_bounds=[LB] * W, bounds_per_window=1)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names) and len(out) <= 200, len(out)
    return out


def _array(value, dtype):
    if value is None:
        return None
    a = np.array(value, dtype=object)
    a[a == "nan"] = np.nan
    return np.ascontiguousarray(a.astype(dtype))


_iq = {}


def run_case(eng, case):
    """One call on the loaded library -> {"rc": ..., "text": its rmx_last_error text ("" for RMX_OK), "untouched": ...}"""
    import radio_mapper_amd as rm
    from radio_mapper_amd import xcorr
    lib = xcorr.load_library()
    a = case["args"]
    if not _iq:
        _iq["iq"] = np.ascontiguousarray(rm.synth.make_windows(W, B, N, 10e6, seed=1)[0])
    bufs = {"iq": _iq["iq"], "lag_int": np.full(SLOTS, FILL, np.int32), "dop_idx": np.full(SLOTS, FILL, np.int32)}
    for k in ("lag_frac", "peak", "dop_frac"):
        bufs[k] = np.full(SLOTS, FILL, np.float32)
    bufs["quality"] = np.full(4 * SLOTS, FILL, np.float32)

    def pointer(spec):
        if spec is None:
            return None
        if spec == "own":
            return bufs[name].ctypes.data_as(C.c_void_p)
        _, on, off = spec.split(":")
        return C.c_void_p(bufs[on].ctypes.data + 4 * int(off))

    keep, argv = [], [eng._ctx]
    for name, v in a.items():
        if name in POINTERS:
            argv.append(pointer(v))
        elif name in ("pairs", "lag_bounds", "band_cps", "doppler_cps"):
            arr = _array(v, np.int32 if name in ("pairs", "lag_bounds") else np.float64)
            keep.append(arr)
            argv.append(None if arr is None else arr.ctypes.data_as(C.c_void_p))
        else:
            argv.append(int(v))
    rc = getattr(lib, case["entry"])(*argv, 0)
    text = lib.rmx_last_error(eng._ctx).decode() if rc != 0 else ""
    untouched = all(bool(np.all(bufs[k] == FILL)) for k in bufs if k != "iq")
    return {"rc": int(rc), "text": text, "untouched": untouched}


def engine():
    from radio_mapper_amd import xcorr
    return xcorr.XcorrEngine(B, N, W)


def main(out_path):
    if os.path.exists(out_path):
        sys.exit(f"{out_path} exists: a recorded table is not overwritten (move it away first)")
    sys.path.insert(0, ROOT)
    from radio_mapper_amd import xcorr
    rows = []
    with engine() as eng:
        for c in cases():
            row = dict(c, **run_case(eng, c))
            assert row["rc"] in (0, -1) and (row["rc"] == 0 or row["untouched"]), row
            rows.append(row)
            print("%-72s %2d %s" % (c["name"], row["rc"], row["text"] or ("wrote nothing" if row["untouched"] else "wrote")), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"library": xcorr.build_info().get("source_digest"), "cases": rows}, f, indent=1)
        f.write("\n")
    print(f"{len(rows)} calls -> {out_path}", flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
