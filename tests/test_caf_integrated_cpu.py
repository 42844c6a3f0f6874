"""rmx_caf_batch_integrated without a GPU: tests/caf_integrated_ref.py pinned against the helpers it stacks (K = 1 is the
Doppler search's reference, the grid [0.0] is the integrated correlation's); the first-maximum and dop_frac rules on
integrated peaks; what the entry is for -- a weak emitter heard by free-running receivers, in counts from the reference
alone; the conditions on the inputs of every case tests/test_gpu_caf_integrated.py holds to the parity rule; the binding's
own side (the export, the header, caf's and MultiXcorrEngine.caf's forwarding of `integrate`); and every refusal of the
request in its order, through a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import caf_integrated_ref as ci
import caf_quality_ref as cq
import caf_ref as cr
import caf_request_ref as rq
import integrated_ref as ir
from radio_mapper_amd import multi, xcorr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement against the helpers it stacks ------------------------------------------------------------------------
@pytest.mark.parametrize("rid", ["phat", "band + bounds"])
def test_one_window_per_group_is_the_doppler_search(rid):
    W, B, N, D, U = 3, 4, 256, 5, 8
    iq, _, grid, _ = cr.scene(W, B, N, D, seed=300 + N + W)
    pairs = cr.CROSS_PAIRS
    lb = np.array([[-(N // 2), N // 3]] * len(pairs), np.int32)
    kw = dict(phat=True) if rid == "phat" else dict(band=np.array([-0.28, 0.31]), lag_bounds=lb)
    ref = ci.reference(iq, grid, 1, pairs, refine=U, **kw)
    base = cq.reference(iq, grid, pairs, refine=U, **kw)
    for k in ("dop", "dop_frac", "lag_int", "lag_frac", "peak", "bin_peak", "hyp_margin", "lag_margin", "flat_bound", "dop_frac_bound",
              "quality", "q_p0", "q_Et", "fine_int", "fine_frac", "fine_peak", "fine_bound", "full_max"):
        assert np.array_equal(ref[k], base[k]), k


@pytest.mark.parametrize("K", [2, 3])
def test_the_zero_hypothesis_alone_is_the_integrated_correlation(K):
    """grid = [0.0]: the table is exactly 1 + 0i and rot_mul leaves x_j's bits, so every figure is integrated_batch's"""
    W, B, N = 6, 3, 64
    iq = cr.scene(W, B, N, 3, seed=64 + K)[0]
    G = W // K
    lb = np.array([[[-20 - g, 17 + q] for q in range(3)] for g in range(G)], np.int32)
    band = rq.window_bands(W)
    ref = ci.reference(iq, [0.0], K, band=band, phat=True, lag_bounds=lb)
    li, lf, pk, mg, _ = ir.integrated_batch(iq, K, band, True, lb)
    assert np.array_equal(ref["dop"], np.zeros((G, 3), ref["dop"].dtype)) and np.array_equal(ref["dop_frac"], np.zeros((G, 3), np.float32))
    assert np.array_equal(ref["lag_int"], li) and np.array_equal(ref["lag_frac"], lf)
    assert np.array_equal(ref["peak"].astype(np.float64), pk) and np.array_equal(ref["lag_margin"], mg)
    assert np.array_equal(ref["q_p0"], pk)


def test_first_maximum_and_dop_frac_on_integrated_peaks():
    """A grid that names each hypothesis twice gives pairs of bit-identical integrated peaks: the d-major first maximum
    keeps the lower index.  dop_frac is the parabola through the INTEGRATED peaks of d* - 1, d*, d* + 1, 0 at the ends."""
    W, B, N, K = 4, 3, 64, 2
    iq, _, grid, _ = cr.scene(W, B, N, 5, seed=77)
    twice = np.repeat(grid, 2)
    r2 = ci.reference(iq, twice, K, phat=True)
    r1 = ci.reference(iq, grid, K, phat=True)
    assert np.array_equal(r2["bin_peak"][..., 0::2], r2["bin_peak"][..., 1::2])
    assert np.all(r2["dop"] % 2 == 0) and np.array_equal(r2["dop"] // 2, r1["dop"])
    assert np.array_equal(r2["lag_int"], r1["lag_int"]) and np.array_equal(r2["peak"], r1["peak"])
    pk, dop = r1["bin_peak"], r1["dop"]
    assert pk.shape == (W // K, 3, 5) and np.array_equal(dop, cr.first_max(pk))
    inner = (dop > 0) & (dop < 4)
    assert inner.any()
    for g, q in zip(*np.nonzero(inner)):
        a, b, c = (float(pk[g, q, dop[g, q] + k]) for k in (-1, 0, 1))
        assert a < b and c <= b
        assert r1["dop_frac"][g, q] == np.float32((a - c) / (2.0 * (a - 2.0 * b + c)))
        assert -0.5 < r1["dop_frac"][g, q] <= 0.5
    assert np.all(r1["dop_frac"][~inner] == 0)
    # the integrated peak of a hypothesis is the root-sum-square of sums over the group, not any single window's peak
    one = rq.reference(iq[:K], grid, phat=True)["bin_peak"]
    assert np.all(pk[0] >= one.max(axis=0) * (1 - 1e-6))


# ---- 2. what the entry is for ---------------------------------------------------------------------------------------------------
WEAK_SNR_DB = -9.0
WEAK_SEEDS = range(40)


def test_weak_emitter_with_free_running_receivers_needs_both():
    """3 buoys, one white emitter at -9 dB per receiver, delays (0, 7, -12), per-receiver offsets (0, +2, -3) grid steps of
    0.5 / N, N = 256, K = 16 windows, D = 13 hypotheses (-6 .. +6 steps), 40 seeds x 3 pairs = 120 integer lags.  On this
    float32 reference:
        integrate = 16 alone                                     3 of 120
        the Doppler search on the first window alone            13 of 120
        the search integrated over the 16 windows              120 of 120, the right hypothesis on all 120
    (the counts are printed; the first two are asserted below half, the last two at 120)"""
    alone, first, both, hyp = ci.weak_counts(WEAK_SEEDS, WEAK_SNR_DB)
    print("lags found of 120: integrate alone %d, search on one window %d, integrated search %d (hypotheses %d)" % (alone, first, both, hyp))
    assert both == 120 and hyp == 120
    assert alone < 60 and first < 60


# ---- 3. the conditions on the inputs of the GPU cases ------------------------------------------------------------------------------
@pytest.mark.parametrize("custom", [False, True], ids=["default", "custom"])
@pytest.mark.parametrize("name", sorted(ci.SCENES))
def test_every_gpu_case_needs_no_excuse_on_the_reference(name, custom):
    """dop_idx exact and lag_int exact are demanded wherever the reference's margins, on the integrated vectors, exceed
    1e-5: here every slot of every case clears that (and caf_ref.MARGIN_BAR between hypotheses), so no slot is excused"""
    ref = ci.case_reference(name, custom)
    print("hypothesis margin %.3e, lag margin %.3e" % (ref["hyp_margin"].min(), ref["lag_margin"].min()))
    excused = int((ref["hyp_margin"] <= cr.MARGIN_BAR).sum() + (ref["lag_margin"] <= rq.LAG_MARGIN_BAR).sum())
    assert excused == 0
    assert np.all(np.isfinite(ref["quality"])) and np.all(ref["q_p0"] > 0)
    assert np.array_equal(ref["q_p0"].astype(np.float32), ref["peak"])       # p0 IS the winner's coarse integrated peak
    assert np.all(np.abs(ref["fine_int"] - ref["lag_int"]) <= 1)


@pytest.mark.parametrize("name", ["one4", "chunk16k2", "chunk18k3", "n256k2", "seam8192"])
def test_winner_indexing_scenes_win_under_different_hypotheses(name):
    """the slots of a call win under different hypotheses: a slot that read another slot's winner, under the one-launch
    virtual group or across the second sweep, would miss the parity bars"""
    dop = ci.case_reference(name, False)["dop"]
    assert len(set(dop.ravel().tolist())) > 1, dop


# ---- 4. the binding -------------------------------------------------------------------------------------------------------------------
def test_export_and_header():
    assert "rmx_caf_batch_integrated" in xcorr.EXPORTS
    header = open(os.path.join(ROOT, "include", "rmx.h")).read()
    assert "int rmx_caf_batch_integrated(rmx_ctx* ctx" in header
    doc = header[header.index("The Doppler search integrated noncoherently"):header.index("int rmx_caf_batch_integrated(")]
    for said in ("integrate == 1 IS rmx_caf_batch_quality", "K^(1/4)", "never a silent", "[G][n_pairs]", "in window order",
                 "The winner is never", "Several bands under the search"):
        assert said in doc, said
    assert header.count("There is no integration here") >= 3                   # the two search entries still have none ...
    assert header.count("rmx_caf_batch_integrated") >= 3                       # ... and point here


class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def _engine(n_buoys, n_samples):
    eng = object.__new__(xcorr.XcorrEngine)
    eng._lib, eng._ctx = _FakeLib(), None
    eng.n_buoys, eng.n_samples, eng.max_windows, eng.device = n_buoys, n_samples, 64, 0
    return eng


def test_caf_forwards_integrate_to_the_new_entry_and_shapes_the_outputs_by_group():
    eng = _engine(3, 16)
    iq = np.zeros((6, 3, 16), np.complex64)
    out = eng.caf(iq, [0.0, 0.01], integrate=3, fine=True, refine=4, quality=True)
    name, args = eng._lib.calls[-1]
    assert name == "rmx_caf_batch_integrated" and args[2] == 6 and args[7] == 3 and args[13] == 4
    assert [a.shape for a in out] == [(2, 3)] * 5 + [(2, 3, 4)]
    lb = np.zeros((2, 3, 2), np.int32)
    eng.caf(iq, [0.0], integrate=3, lag_bounds=lb, band=np.tile([-0.2, 0.2], (6, 1)))
    name, args = eng._lib.calls[-1]
    assert name == "rmx_caf_batch_integrated" and args[9] == 1 and args[12] == 1     # bands per window, bounds per group
    with pytest.raises(ValueError, match="lag_bounds"):
        eng.caf(iq, [0.0], integrate=3, lag_bounds=np.zeros((6, 3, 2), np.int32))    # per WINDOW: refused
    with pytest.raises(ValueError, match="multiple of integrate"):
        eng.caf(iq, [0.0], integrate=4)
    with pytest.raises(ValueError, match="integrate"):
        eng.caf(iq, [0.0], integrate=0)
    # without it (or with 1) the entries are those of the search per window
    eng.caf(iq, [0.0, 0.01])
    assert eng._lib.calls[-1][0] == "rmx_caf_batch"
    eng.caf(iq, [0.0, 0.01], integrate=1, refine=2)
    assert eng._lib.calls[-1][0] == "rmx_caf_batch_quality"
    eng.caf_device(1 << 20, 6, [0.0], 2 << 20, 3 << 20, 4 << 20, 5 << 20, integrate=2)
    name, args = eng._lib.calls[-1]
    assert name == "rmx_caf_batch_integrated" and args[7] == 2
    eng.caf_device(1 << 20, 6, [0.0], 2 << 20, 3 << 20, 4 << 20, 5 << 20)
    assert eng._lib.calls[-1][0] == "rmx_caf_batch"


class _StubCaf:
    instances = []

    def __init__(self, n_buoys, n_samples, max_windows, device):
        self.n_buoys, self.max_windows, self.calls = n_buoys, max_windows, []
        _StubCaf.instances.append(self)

    def caf(self, iq, doppler_cps, pairs=None, **kw):
        K = kw.get("integrate", 1)
        self.calls.append(dict(kw, windows=iq.shape[0]))
        P = self.n_buoys * (self.n_buoys - 1) // 2
        tag = np.asarray(iq)[::K, 0, 0].real.astype(np.int32)[:, None] + np.zeros((1, P), np.int32)
        lb = kw.get("lag_bounds")
        lo = tag if lb is None or np.asarray(lb).ndim == 2 else np.asarray(lb)[:, :, 0]
        out = (tag, lo, tag.astype(np.float32), tag.astype(np.float32) + 0.5)
        if kw.get("fine"):
            out = (out[0], tag.astype(np.float32) / 100) + out[1:]
        if kw.get("quality"):
            out = out + (tag.astype(np.float32)[:, :, None] + np.arange(4, dtype=np.float32),)
        return out

    def close(self):
        pass


def test_multi_engine_caf_shards_whole_groups():
    _StubCaf.instances.clear()
    W, B, N, K = 14, 3, 16, 2
    G = W // K
    iq = np.zeros((W, B, N), np.complex64)
    iq[:, 0, 0] = np.arange(W)
    lb = np.zeros((G, 3, 2), np.int32)
    lb[:, :, 0] = 100 + np.arange(G)[:, None]
    band = np.tile([-0.2, 0.2], (W, 1))
    with multi.MultiXcorrEngine(B, N, W, devices=[0, 1, 2], engine_factory=_StubCaf) as eng:
        out = eng.caf(iq, [0.0, 0.01], lag_bounds=lb, band=band, whiten=True, fine=True, refine=4, quality=True, integrate=K)
        assert len(out) == 6 and all(a.shape[:2] == (G, 3) for a in out) and out[5].shape == (G, 3, 4)
        assert np.array_equal(out[0][:, 0], K * np.arange(G))                  # every group once, in order, from its first window
        assert np.array_equal(out[2][:, 0], 100 + np.arange(G))                # ... under its own group's bounds
        calls = [c for e in _StubCaf.instances for c in e.calls]
        assert sum(c["windows"] for c in calls) == W and all(c["windows"] % K == 0 for c in calls)
        assert all(c["integrate"] == K and c["refine"] == 4 and c["quality"] is True and c["fine"] is True for c in calls)
        assert all(c["band"].shape == (c["windows"], 2) and c["lag_bounds"].shape == (c["windows"] // K, 3, 2) for c in calls)
        with pytest.raises(ValueError, match="multiple of integrate"):
            eng.caf(iq, [0.0], integrate=4)
        # the call without it is the one it was
        for e in _StubCaf.instances:
            e.calls.clear()
        assert len(eng.caf(iq, [0.0, 0.01])) == 4
        assert all({k: v for k, v in e.calls[-1].items() if k != "windows"} == {} for e in _StubCaf.instances)
    _StubCaf.instances.clear()
    with multi.MultiXcorrEngine(B, N, 4, devices=[0, 1, 2], engine_factory=_StubCaf) as eng:     # engines of 2 windows each
        with pytest.raises(ValueError, match="more than one device's engine holds"):
            eng.caf(iq[:4], [0.0], integrate=4)


# ---- 5. every refusal of the request, in its order --------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_caf_integrated_request_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_caf_integrated_request")
    src = os.path.join(ROOT, "tests", "host", "test_caf_integrated_request.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-pthread", "-Wall", "-Wextra", "-Werror", "-o", exe, src]
    subprocess.run(cmd, check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "all checks passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
