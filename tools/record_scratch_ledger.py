"""GPU box: what rmx_scratch_bytes returns after rmx_create and after each call of a fixed script of small calls -- the
behaviour pin of the ledger that the ctx's buffers keep (radio-mapper_amd/csrc/dev_buf.hpp).  The script touches every
buffer that counts: the N = 4096 spectrum scratch and its growth, both stages (lag bounds, bands), the tables and the
persistent scratch of every whole-window length, the chunk-sized and the pair-dependent buffers of the four-step path,
and the rotated spectra of a Doppler search on a generic length.

usage: RMX_LIBRARY=<library of the commit the table pins> python tools/record_scratch_ledger.py OUT.json
       Record with the library of the commit BEFORE a change to the ownership of the buffers, never with the changed
       one; an existing OUT.json is not overwritten.  tests/test_gpu_scratch_ledger.py replays
       tests/golden/scratch_ledger.json on the tree's library."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "scratch_ledger.json")

BAND = [-0.2, 0.3]
DOP = [-1e-4, 0.0, 1e-4]


def script():
    """[(ctx name, (n_buoys, n_samples, max_windows), [(step name, call on (engine, iq))])]"""
    lb3 = [[-30, 30]] * 3
    two = [[0, 2], [1, 2]]
    return [
        ("n4096_b3_w8", (3, 4096, 8), [
            ("default_pairs", lambda e, iq: e.correlate(iq)),
            ("custom_pairs", lambda e, iq: e.correlate(iq, pairs=two)),
            ("bounded", lambda e, iq: e.correlate(iq, lag_bounds=lb3)),
            ("weighted", lambda e, iq: e.correlate(iq, band=BAND, whiten=True)),
            ("bounded_per_window", lambda e, iq: e.correlate(iq, lag_bounds=[lb3] * 8)),
        ]),
        # more windows than compute units: the per-transform routes need a slot per window of the chunk
        ("n4096_b3_w264", (3, 4096, 264), [
            ("default_pairs", lambda e, iq: e.correlate(iq)),
            ("custom_pairs", lambda e, iq: e.correlate(iq, pairs=two)),
        ]),
        ("n1024_b3_w8", (3, 1024, 8), [
            ("default_pairs", lambda e, iq: e.correlate(iq)),
            ("doppler", lambda e, iq: e.caf(iq, DOP)),
        ]),
        ("n8192_b3_w8", (3, 8192, 8), [("default_pairs", lambda e, iq: e.correlate(iq))]),
        ("n16384_b2_w8", (2, 16384, 8), [("default_pairs", lambda e, iq: e.correlate(iq))]),
        ("n65536_b3_w2", (3, 65536, 2), [
            ("one_pair", lambda e, iq: e.correlate(iq, pairs=[[0, 2]])),
            ("three_pairs", lambda e, iq: e.correlate(iq)),
            ("doppler", lambda e, iq: e.caf(iq[:1], DOP[:2], pairs=[[0, 1]])),
        ]),
    ]


def names():
    return [f"{ctx}:{step}" for ctx, _, steps in script() for step in ["create"] + [s for s, _ in steps]]


def run():
    """the script on the loaded library -> [{"name": ..., "scratch_bytes": ...}]"""
    import radio_mapper_amd as rm
    from radio_mapper_amd import xcorr
    rows = []
    for ctx, (B, N, W), steps in script():
        iq = np.ascontiguousarray(rm.synth.make_windows(W, B, N, 10e6, seed=1)[0])
        with xcorr.XcorrEngine(B, N, W) as eng:
            rows.append({"name": f"{ctx}:create", "scratch_bytes": eng.scratch_bytes()})
            for step, call in steps:
                call(eng, iq)
                rows.append({"name": f"{ctx}:{step}", "scratch_bytes": eng.scratch_bytes()})
    return rows


def main(out_path):
    if os.path.exists(out_path):
        sys.exit(f"{out_path} exists: a recorded table is not overwritten (move it away first)")
    sys.path.insert(0, ROOT)
    from radio_mapper_amd import xcorr
    rows = run()
    for r in rows:
        print("%-40s %14d" % (r["name"], r["scratch_bytes"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"library": xcorr.build_info().get("source_digest"), "steps": rows}, f, indent=1)
        f.write("\n")
    print(f"{len(rows)} readings -> {out_path}", flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
