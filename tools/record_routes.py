"""GPU box: which kernels every kind of correlation call launches, and what they compute -- the behaviour pin of the
route planner (host_plan.hpp: plan_route).  Runs a fixed list of small cases through the public Python API with
option timing = 1 and writes, per case, the parameters, last_timing_by_kernel() reduced to {family: launches} and a
SHA-256 over the bytes of every output array.  Each case runs twice; a case whose two digests differ gets digest null
and its first run's arrays instead (tests/test_gpu_routes.py then compares it by value; only small cases can be kept so).

usage: RMX_LIBRARY=<library of the commit the table pins> python tools/record_routes.py [--caf] OUT.json
       Record with the library of the commit BEFORE a change to the planner, never with the changed one; an existing
       OUT.json is not overwritten.  tests/test_gpu_routes.py replays tests/golden/route_table.json on the tree's library.
       --caf records caf_cases() instead of cases(): tests/golden/caf_route_table.json, the pin of the Doppler search's plan
       (host_plan.hpp: plan_caf), recorded with the library of the commit in front of it and replayed by the same test."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "route_table.json")
CAF_TABLE = os.path.join(ROOT, "tests", "golden", "caf_route_table.json")
FS = 10e6
MAX_KEPT = 4096   # elements of a not reproducible case's outputs that the table may carry


def case(name, B, N, W, **kw):
    c = dict(name=name, kind="xcorr", B=B, N=N, W=W, max_windows=W, defaults={}, options={}, pairs=None, u8=False,
             device=False, bounded=False, band=None, whiten=False, integrate=1, refine=0, quality=False, dopplers=None,
             seed=11)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def cases():
    out = []
    # ---- N = 4096: the cost model on a chip of 8 (or 6) CUs --------------------------------------------------------------
    for B in (3, 8):
        for W in (1, 2, 4, 8, 12):                                 # either side of the fused / per-transform crossover
            out.append(case(f"n4096_b{B}_w{W}", B, 4096, W, defaults={"ncus": 8}))
        for W in (9, 15, 17, 23):                                  # full rounds + a partial one that pays / does not
            out.append(case(f"n4096_b{B}_w{W}_tail", B, 4096, W, defaults={"ncus": 8}))
        # two chunks of 8 on 6 CUs: the first chunk's remainder (2) is larger than the last one's (1 / 0)
        out.append(case(f"n4096_b{B}_w15_chunk8_cu6", B, 4096, 15, defaults={"ncus": 6, "chunk_windows": 8}))
        out.append(case(f"n4096_b{B}_w14_chunk8_cu6", B, 4096, 14, defaults={"ncus": 6, "chunk_windows": 8}))
        out.append(case(f"n4096_b{B}_w17_rev", B, 4096, 17, defaults={"ncus": 8}, pairs="rev"))
        out.append(case(f"n4096_b{B}_w17_explicit_default", B, 4096, 17, defaults={"ncus": 8}, pairs="default"))
        out.append(case(f"n4096_b{B}_w4_sub", B, 4096, 4, defaults={"ncus": 8}, pairs="sub"))
        out.append(case(f"n4096_b{B}_w17_unfused", B, 4096, 17, defaults={"ncus": 8}, options={"fused": 0}))
        out.append(case(f"n4096_b{B}_w17_ppb3", B, 4096, 17, defaults={"ncus": 8}, options={"pairs_per_block": 3}))
        out.append(case(f"n4096_b{B}_w2_ppb3", B, 4096, 2, defaults={"ncus": 8}, options={"pairs_per_block": 3}))
        out.append(case(f"n4096_b{B}_w17_small0", B, 4096, 17, defaults={"ncus": 8, "small4096": 0}))
        out.append(case(f"n4096_b{B}_w2_small0", B, 4096, 2, defaults={"ncus": 8, "small4096": 0}))
        out.append(case(f"n4096_b{B}_w17_u8", B, 4096, 17, defaults={"ncus": 8}, u8=True))
        out.append(case(f"n4096_b{B}_w17_bounded", B, 4096, 17, defaults={"ncus": 8}, bounded=True))
    out.append(case("n4096_b2_w3", 2, 4096, 3, defaults={"ncus": 8}))                 # two buoys: outside the model
    out.append(case("n4096_b3_w521_host", 3, 4096, 521, defaults={"ncus": 8}))        # the pipelined host copy: no tail
    out.append(case("n4096_b3_w521_device", 3, 4096, 521, defaults={"ncus": 8}, device=True))
    out.append(case("n4096_b3_w4_generic", 3, 4096, 4, defaults={"ncus": 8, "generic4096": 1}))
    # ---- generic lengths, default pair list ------------------------------------------------------------------------------
    out.append(case("n1024_b3_w5", 3, 1024, 5, defaults={"ncus": 8}))                 # g_win_fused
    out.append(case("n1024_b3_w5_wfused0", 3, 1024, 5, defaults={"ncus": 8, "wfused": 0}))
    for W in (2, 24):                                                                   # g_win_scr below / above its fill
        out.append(case(f"n1024_b8_w{W}", 8, 1024, W, defaults={"ncus": 8}))
    out.append(case("n1024_b8_w2_wscr2", 8, 1024, 2, defaults={"ncus": 8, "wscr": 2}))
    out.append(case("n1024_b8_w24_wscr0", 8, 1024, 24, defaults={"ncus": 8, "wscr": 0}))
    for W in (1, 4, 9, 11):                                                             # k_win8kl: below 5/16, whole, tail, no tail
        out.append(case(f"n8192_b8_w{W}", 8, 8192, W, defaults={"ncus": 8}))
    out.append(case("n8192_b8_w9_wscr2", 8, 8192, 9, defaults={"ncus": 8, "wscr": 2}))
    out.append(case("n8192_b8_w1_wscr2", 8, 8192, 1, defaults={"ncus": 8, "wscr": 2}))
    out.append(case("n8192_b8_w9_bounded", 8, 8192, 9, defaults={"ncus": 8}, bounded=True))
    out.append(case("n8192_b8_w9_kwin8k0", 8, 8192, 9, defaults={"ncus": 8, "kwin8k": 0}))
    out.append(case("n8192_b3_w9", 3, 8192, 9, defaults={"ncus": 8}))
    out.append(case("n8192_b3_w4_long", 3, 8192, 4, defaults={"ncus": 8}, pairs="long"))
    out.append(case("n8192_b3_w4_long_bounded", 3, 8192, 4, defaults={"ncus": 8}, pairs="long", bounded=True))
    for W in (3, 4, 17):                                                                # k16 below / at its minimum, three chunks
        out.append(case(f"n16384_b3_w{W}_k16min4", 3, 16384, W, defaults={"ncus": 8, "k16_min_windows": 4}))
    out.append(case("n16384_b8_w1", 8, 16384, 1, defaults={"ncus": 8}))                # default minimum: 100 / 36 -> 3
    out.append(case("n16384_b8_w3", 8, 16384, 3, defaults={"ncus": 8}))
    out.append(case("n16384_b3_w2_kwin16k2", 3, 16384, 2, defaults={"ncus": 8, "kwin16k": 2}))
    out.append(case("n16384_b3_w9_wscr2", 3, 16384, 9, defaults={"ncus": 8, "wscr": 2}))
    out.append(case("n16384_b3_w4_bounded", 3, 16384, 4, defaults={"ncus": 8, "k16_min_windows": 4}, bounded=True))
    for W in (3, 8, 9, 14):                                                             # g_win_eo15: below 11/16, whole, tail, no tail
        out.append(case(f"n16384_b3_w{W}_kwin16k0", 3, 16384, W, defaults={"ncus": 8, "kwin16k": 0}))
    for W in (1, 2):                                                                    # g_rows_fused: too few units / enough
        out.append(case(f"n65536_b3_w{W}_cu32", 3, 65536, W, defaults={"ncus": 32}))
    out.append(case("n65536_b3_w1_fused2", 3, 65536, 1, defaults={"ncus": 32, "fused": 2}))
    out.append(case("n65536_b3_w2_fused0", 3, 65536, 2, defaults={"ncus": 32, "fused": 0}))
    out.append(case("n65536_b8_w2", 8, 65536, 2, defaults={"ncus": 8}))                # g_rows_anchor
    out.append(case("n65536_b5_w2", 5, 65536, 2, defaults={"ncus": 8}))                # g_rows_inv
    out.append(case("n65536_b8_w2_rev", 8, 65536, 2, defaults={"ncus": 8}, pairs="rev"))
    # ---- features, 3 buoys ------------------------------------------------------------------------------------------------
    band = [-0.2, 0.3]
    for N in (256, 4096, 8192, 65536):
        d = {"ncus": 8}
        f = lambda tag, W=6, **kw: out.append(case(f"n{N}_{tag}", 3, N, W, **{"defaults": d, **kw}))   # noqa: E731
        f("bounded", bounded=True)
        f("band_phat", band=band, whiten=True)
        f("integ2", integrate=2)
        f("refine4", refine=4)
        f("quality", quality=True)
        f("quality_band", quality=True, band=band)
        f("all", bounded=True, band=band, whiten=True, integrate=2, refine=4, quality=True)
        two = {"chunk_windows": 8} if N == 4096 else {"gen_chunk": 4}
        nw = 16 if N == 4096 else 8
        f("all_two_chunks", W=nw, defaults={**d, **two}, bounded=True, band=band, whiten=True, integrate=2, refine=4, quality=True)
        f("quality_two_chunks", W=nw, defaults={**d, **two}, quality=True)
        f("plain_two_chunks", W=nw, defaults={**d, **two})
        if N == 4096:                                              # (a chunk of N = 4096 holds at least 8 windows)
            f("integ16_chunk8", W=16, defaults={**d, "chunk_windows": 8}, integrate=16)
        else:
            f("integ2_chunk1", W=4, defaults={**d, "gen_chunk": 1}, integrate=2)
    out.append(case("n65536_integ2_cols64", 3, 65536, 4, defaults={"ncus": 8, "cols_threads": 64}, integrate=2))
    # ---- CAF ------------------------------------------------------------------------------------------------------------
    dop = [-1e-4, 0.0, 1e-4]
    out.append(case("caf_n1024_b3_w4", 3, 1024, 4, kind="caf", defaults={"ncus": 8}, dopplers=dop))
    out.append(case("caf_n4096_b3_w4", 3, 4096, 4, kind="caf", defaults={"ncus": 8}, dopplers=dop))
    out.append(case("caf_n4096_b3_w12_chunk8", 3, 4096, 12, kind="caf", defaults={"ncus": 8, "chunk_windows": 8}, dopplers=dop))
    out.append(case("caf_n4096_b8_w4_ppb3", 8, 4096, 4, kind="caf", defaults={"ncus": 8}, options={"pairs_per_block": 3}, dopplers=dop))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def caf_case(name, B, N, W, fine=False, **kw):
    c = case(name, B, N, W, kind="caf", **{"dopplers": [-1e-4, 0.0, 1e-4], "defaults": {"ncus": 8}, **kw})
    c["fine"] = fine
    return c


def caf_cases():
    """the Doppler search: every branch of the request on every route, 3 buoys and three hypotheses unless stated"""
    out = []
    band = [-0.2, 0.3]
    every = dict(fine=True, bounded=True, band=band, whiten=True, integrate=2, refine=4, quality=True)
    # small-L kernels / N = 4096 in one launch / N = 4096 per hypothesis, chunks of 8 + 4 / four-step
    for tag, N, W, d in (("n256", 256, 4, {}), ("n4096_one", 4096, 4, {}), ("n4096_per", 4096, 12, {"chunk_windows": 8}),
                         ("n8192", 8192, 4, {})):
        f = lambda t, W=W, d=d, **kw: out.append(caf_case(f"caf_{tag}_{t}", 3, N, W, defaults={"ncus": 8, **d}, **kw))   # noqa: E731
        f("fine", fine=True)
        f("bounded_band_phat", bounded=True, band=band, whiten=True)
        f("integ2", integrate=2)
        f("refine4_quality", refine=4, quality=True)
        f("all", **every)
        # two chunks: the second sweep over the hypotheses crosses a seam (N = 4096: more windows than a chunk is never
        # one launch, so the two N = 4096 rows are one)
        if tag != "n4096_one":
            two = {"chunk_windows": 8} if N == 4096 else {"gen_chunk": 4}
            f("all_two_chunks", W=16 if N == 4096 else 8, d=two, **every)
    f = lambda t, B=3, N=4096, W=4, **kw: out.append(caf_case(f"caf_{t}", B, N, W, **kw))   # noqa: E731
    f("n4096_single", dopplers=[1e-4])                              # one hypothesis: never one launch
    f("n4096_one_fine_device", fine=True, device=True)              # the two sides of the caf_nb rule
    f("n4096_per_fine_device", W=12, defaults={"ncus": 8, "chunk_windows": 8}, fine=True, device=True)
    f("n4096_u8", u8=True)
    f("n4096_generic", defaults={"ncus": 8, "generic4096": 1})
    f("n4096_rev", pairs="rev")
    f("n4096_b8_ppb3_integ2", B=8, options={"pairs_per_block": 3}, integrate=2)
    f("n4096_integ16_chunk8", W=16, defaults={"ncus": 8, "chunk_windows": 8}, integrate=16)
    f("n8192_integ2_chunk1", N=8192, defaults={"ncus": 8, "gen_chunk": 1}, integrate=2)
    f("n65536_integ2_cols64", N=65536, defaults={"ncus": 8, "cols_threads": 64}, integrate=2)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def _pairs(kind, B):
    from radio_mapper_amd import xcorr
    pl = xcorr.pair_list(B)
    if kind is None:
        return None
    if kind == "default":
        return pl
    if kind == "rev":
        return pl[::-1].copy()
    if kind == "sub":
        return pl[:-1].copy()
    if kind == "long":                                             # longer than the LDS copy of k_win8kl / k16_pairs (640)
        return np.tile(pl, (700 // len(pl) + 1, 1))[:700].copy()
    raise ValueError(kind)


_inputs = {}


def _windows(c):
    import radio_mapper_amd as rm
    key = (c["W"], c["B"], c["N"], c["seed"])
    if key not in _inputs:
        _inputs.clear()                                            # (cases of one shape follow each other)
        _inputs[key] = rm.synth.make_windows(c["W"], c["B"], c["N"], FS, seed=c["seed"], return_u8=True)
    iq, _, raw = _inputs[key]
    return raw if c["u8"] else iq


def run_case(c):
    """One case on the loaded library -> {"launches": {family: n}, "arrays": [...]} or {"error": text}"""
    from radio_mapper_amd import xcorr
    xcorr.clear_default_options()
    for k, v in c["defaults"].items():
        xcorr.set_default_option(k, v)
    try:
        iq = _windows(c)
        pairs = _pairs(c["pairs"], c["B"])
        P = len(pairs) if pairs is not None else c["B"] * (c["B"] - 1) // 2
        with xcorr.XcorrEngine(c["B"], c["N"], c["max_windows"]) as eng:
            for k, v in c["options"].items():
                eng.set_option(k, v)
            eng.set_option("timing", 1)
            try:
                kw = dict(pairs=pairs, band=c["band"], whiten=c["whiten"], integrate=c["integrate"], refine=c["refine"])
                if c["bounded"]:
                    kw["lag_bounds"] = np.tile(np.array([[-64, 64]], np.int32), (P, 1))
                if c["kind"] == "caf":
                    if c["integrate"] == 1:
                        kw["integrate"] = None                   # (the search per window, as the rows without the key)
                    if c["device"]:
                        arrays = _caf_device(eng, iq, P, c, kw)
                    else:
                        arrays = eng.caf(iq, c["dopplers"], fine=c.get("fine", False), quality=c["quality"], **kw)
                else:
                    if c["device"]:
                        arrays = _correlate_device(eng, iq, P, c, kw)
                    else:
                        arrays = eng.correlate(iq, quality=c["quality"], **kw)
            except xcorr.RmxError as e:
                return {"error": str(e)}
            launches = {k: v["launches"] for k, v in sorted(eng.last_timing_by_kernel().items())}
        return {"launches": launches, "arrays": [np.ascontiguousarray(a) for a in arrays]}
    finally:
        xcorr.clear_default_options()


def _correlate_device(eng, iq, P, c, kw):
    import torch
    W, K = c["W"], c["integrate"]
    dev = torch.device("cuda", 0)
    t_iq = torch.from_numpy(iq).to(dev)
    li = torch.zeros((W // K, P), dtype=torch.int32, device=dev)
    lf = torch.zeros((W // K, P), dtype=torch.float32, device=dev)
    pk = torch.zeros((W // K, P), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    eng.correlate_device(t_iq.data_ptr(), W, li.data_ptr(), lf.data_ptr(), pk.data_ptr(), u8=c["u8"], **kw)
    eng.synchronize()
    return li.cpu().numpy(), lf.cpu().numpy(), pk.cpu().numpy()


def _caf_device(eng, iq, P, c, kw):
    """caf_device with every output buffer [W // K][P] (quality [W // K][P][4]), in the order caf() returns them"""
    import torch
    W, G = c["W"], c["W"] // c["integrate"]
    dev = torch.device("cuda", 0)
    t_iq = torch.from_numpy(iq).to(dev)
    i32 = lambda: torch.zeros((G, P), dtype=torch.int32, device=dev)      # noqa: E731
    f32 = lambda *s: torch.zeros((G, P) + s, dtype=torch.float32, device=dev)   # noqa: E731
    dop, li, lf, pk = i32(), i32(), f32(), f32()
    df = f32() if c.get("fine", False) else None
    q = f32(4) if c["quality"] else None
    torch.cuda.synchronize()
    eng.caf_device(t_iq.data_ptr(), W, c["dopplers"], dop.data_ptr(), li.data_ptr(), lf.data_ptr(), pk.data_ptr(), u8=c["u8"],
                   dop_frac_ptr=df.data_ptr() if df is not None else 0, quality_ptr=q.data_ptr() if q is not None else 0, **kw)
    eng.synchronize()
    return tuple(t.cpu().numpy() for t in (dop, df, li, lf, pk, q) if t is not None)


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def record(c):
    """the table entry of one case: run twice, digest (or null + the first run's arrays when the two runs differ)"""
    a, b = run_case(c), run_case(c)
    row = dict(c)
    if "error" in a:
        assert a == b, (a, b)
        row["error"] = a["error"]
        return row
    assert a["launches"] == b["launches"], (c["name"], a["launches"], b["launches"])
    row["launches"] = a["launches"]
    da, db = digest(a["arrays"]), digest(b["arrays"])
    row["digest"] = da if da == db else None
    if da != db:
        assert sum(x.size for x in a["arrays"]) <= MAX_KEPT, f"{c['name']} is not reproducible and too large to keep by value"
        row["arrays"] = [x.tolist() for x in a["arrays"]]
    return row


def main(out_path, caf=False):
    if os.path.exists(out_path):
        sys.exit(f"{out_path} exists: a recorded table is not overwritten (move it away first)")
    sys.path.insert(0, ROOT)
    from radio_mapper_amd import xcorr
    rows = []
    for c in (caf_cases() if caf else cases()):
        row = record(c)
        rows.append(row)
        print("%-36s %s %s" % (c["name"], row.get("error") or row["launches"],
                               "" if "error" in row else (row["digest"] or "NOT REPRODUCIBLE")[:16]), flush=True)
    n_null = sum(1 for r in rows if "error" not in r and r["digest"] is None)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"library": xcorr.build_info().get("source_digest"), "cases": rows}, f, indent=1)
        f.write("\n")
    print(f"{len(rows)} cases, {n_null} not reproducible -> {out_path}", flush=True)
    return 0 if 10 * n_null <= len(rows) else 1


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--caf"]
    if len(args) != 1:
        sys.exit(__doc__)
    sys.exit(main(args[0], caf=len(args) < len(sys.argv) - 1))
