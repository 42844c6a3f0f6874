"""rmx_caf_batch_quality without a GPU: tests/caf_quality_ref.py pinned against the three helpers it stacks, called by hand
on host-rotated windows; the conditions on the inputs of every case tests/test_gpu_caf_quality.py holds to the parity
rule; what the entry is for -- a threshold on psr separates emitter pairs from noise-only pairs under the Doppler search --
in numbers from the reference alone; and the binding's own side: the export, the header, MultiXcorrEngine.caf's gather."""
import os

import numpy as np
import pytest

import caf_quality_ref as cq
import caf_ref as cr
import caf_request_ref as rq
import quality_ref as qr
import refined_ref as rr
from radio_mapper_amd import multi, xcorr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement against its three helpers -------------------------------------------------------------------------
@pytest.mark.parametrize("rid", ["phat", "band + bounds"])
def test_reference_is_the_three_helpers_on_the_winners_rotated_pair(rid):
    """Buoys 2 and 3 rotated on the host, hypothesis by hypothesis, and CROSS_PAIRS ({0, 1} x {2, 3}: no buoy is both an i and
    a j): caf_request_ref's winner, then quality_ref and refined_ref on the rotated batch, taken at the winner, are
    reference()'s values exactly -- the same float64 arithmetic on the same float32 windows."""
    W, B, N, D, U = 3, 4, 256, 5, 8
    iq, _, grid, _ = cr.scene(W, B, N, D, seed=300 + N + W)
    pairs = cr.CROSS_PAIRS
    lb = np.array([[-(N // 2), N // 3]] * len(pairs), np.int32)
    kw = dict(phat=True) if rid == "phat" else dict(band=np.array([-0.28, 0.31]), lag_bounds=lb)
    ref = cq.reference(iq, grid, pairs, refine=U, **kw)
    base = rq.reference(iq, grid, pairs, **kw)
    for k in ("dop", "dop_frac", "lag_int", "lag_frac", "peak"):
        assert np.array_equal(ref[k], base[k]), k                  # the winner and the coarse outputs are the search's own
    assert len(set(ref["dop"].ravel().tolist())) > 1
    for d in sorted(set(ref["dop"].ravel().tolist())):
        x = iq.copy()
        x[:, 2:] = cr.rot_mul(iq[:, 2:], cr.libm_phasor(grid[d], N))
        qual, det = qr.quality_batch(x, 1, kw.get("band"), bool(kw.get("phat")), kw.get("lag_bounds"), pairs, detail=True)
        li, lf, pk, _, fm, fb = rr.refined_batch(x, U, 1, kw.get("band"), bool(kw.get("phat")), kw.get("lag_bounds"), pairs)
        won = ref["dop"] == d
        assert np.array_equal(ref["quality"][won], qual[won]) and np.array_equal(ref["q_p0"][won], det["p0"][won])
        assert np.array_equal(ref["q_p0"][won].astype(np.float32), ref["peak"][won])       # p0 IS the winner's coarse peak
        assert np.array_equal(det["lag_int"][won], ref["lag_int"][won])
        assert np.array_equal(ref["fine_int"][won], li[won]) and np.array_equal(ref["fine_frac"][won], lf[won])
        assert np.array_equal(ref["fine_peak"][won], pk[won]) and np.array_equal(ref["fine_bound"][won], fb[won])
    assert np.all(np.abs(ref["fine_int"] - ref["lag_int"]) <= 1)    # the fine rule stays within one sample of the coarse lag


# ---- 2. the conditions on the inputs of the GPU cases ----------------------------------------------------------------------
@pytest.mark.parametrize("custom", [False, True], ids=["default", "custom"])
@pytest.mark.parametrize("name", sorted(cq.SCENES))
def test_every_gpu_case_is_far_from_a_tie_on_the_reference(name, custom):
    """dop_idx exact and the coarse lag exact are fair demands only where the best hypothesis stands more than
    caf_ref.MARGIN_BAR above the second best and the winner's two largest magnitudes more than LAG_MARGIN_BAR apart."""
    ref = cq.case_reference(name, custom)
    print("hypothesis margin %.3e, lag margin %.3e" % (ref["hyp_margin"].min(), ref["lag_margin"].min()))
    assert ref["hyp_margin"].min() > cr.MARGIN_BAR
    assert ref["lag_margin"].min() > rq.LAG_MARGIN_BAR
    assert np.all(np.isfinite(ref["quality"])) and np.all(ref["q_p0"] > 0)


@pytest.mark.parametrize("name", ["one3", "seam256", "seam8192", "chunked12"])
def test_winner_indexing_scenes_win_under_different_hypotheses(name):
    """the pairs of one window win under different hypotheses, and so do the windows of one pair: a slot that read another
    slot's winner, under the one-launch virtual window or across the second sweep, would miss the parity bars"""
    dop = cq.case_reference(name, False)["dop"]
    assert any(len(set(row.tolist())) > 1 for row in dop), dop
    assert any(len(set(col.tolist())) > 1 for col in dop.T), dop


# ---- 3. what the entry is for -------------------------------------------------------------------------------------------------
def test_psr_threshold_separates_emitter_pairs_from_noise_pairs_under_the_search():
    """DESIGN.md section 5.5's DC-offset scene with a noise-only fourth buoy, PHAT and the Doppler search: every pair
    yields a lag and a hypothesis; the emitter pairs' psr clears psr_threshold(2N - 1, 1e-3), the noise-only pairs' does
    not.  N = 1024: at N = 256 the reference does not separate them -- pair (0, 2), whose windows overlap in 86 of 256
    samples, has psr 20.2 under a threshold of 26.3 (the others 127.8 and 170.6, the noise-only pairs 8.3 to 10.8)."""
    N = 1024
    iq, grid, emit, noise = cq.dc_noise_scene(N)
    ref = cq.reference(iq, grid, phat=True)
    psr = ref["quality"][0, :, qr.PSR]
    thr = xcorr.psr_threshold(2 * N - 1, 1e-3)
    print("threshold %.2f, emitter pairs %s, noise-only pairs %s" % (thr, np.round(psr[emit], 1), np.round(psr[noise], 2)))
    assert np.all(psr[emit] > thr) and np.all(psr[noise] < thr)
    assert np.all(ref["quality"][0, emit, qr.COHERENCE] > 3 * ref["quality"][0, noise, qr.COHERENCE].max())


# ---- 4. the binding ---------------------------------------------------------------------------------------------------------------
def test_export_and_header():
    assert "rmx_caf_batch_quality" in xcorr.EXPORTS
    header = open(os.path.join(ROOT, "include", "rmx.h")).read()
    assert "int rmx_caf_batch_quality(rmx_ctx* ctx" in header
    for gone in ("rmx_caf_batch is not refined", "rmx_caf_batch reports no quality", "is not refined and reports no quality"):
        assert gone not in header
    assert "There is no integration here" in header


class _StubCaf:
    instances = []

    def __init__(self, n_buoys, n_samples, max_windows, device):
        self.n_buoys, self.calls = n_buoys, []
        _StubCaf.instances.append(self)

    def caf(self, iq, doppler_cps, pairs=None, **kw):
        self.calls.append(kw)
        W, P = iq.shape[0], self.n_buoys * (self.n_buoys - 1) // 2
        tag = np.asarray(iq)[:, 0, 0].real.astype(np.int32)[:, None] + np.zeros((1, P), np.int32)
        out = (tag, tag + 1, tag.astype(np.float32), tag.astype(np.float32) + 0.5)
        if kw.get("fine"):
            out = (out[0], tag.astype(np.float32) / 100) + out[1:]
        if kw.get("quality"):
            out = out + (tag.astype(np.float32)[:, :, None] + np.arange(4, dtype=np.float32),)
        return out

    def close(self):
        pass


def test_multi_engine_caf_hands_refine_and_quality_to_every_shard():
    _StubCaf.instances.clear()
    W, B, N = 7, 3, 16
    iq = np.zeros((W, B, N), np.complex64)
    iq[:, 0, 0] = np.arange(W)
    with multi.MultiXcorrEngine(B, N, W, devices=[0, 1, 2], engine_factory=_StubCaf) as eng:
        out = eng.caf(iq, [0.0, 0.01], whiten=True, fine=True, refine=4, quality=True)
        assert len(out) == 6 and out[5].shape == (W, 3, 4) and out[5].dtype == np.float32
        assert np.array_equal(out[5][:, 1], np.arange(W)[:, None] + np.arange(4)) and np.array_equal(out[0][:, 0], np.arange(W))
        assert all(e.calls[-1]["refine"] == 4 and e.calls[-1]["quality"] is True for e in _StubCaf.instances)
        out = eng.caf(iq, [0.0, 0.01], quality=True)
        assert len(out) == 5 and out[4].shape == (W, 3, 4) and all(e.calls[-1]["refine"] == 0 for e in _StubCaf.instances)
        out = eng.caf(iq, [0.0, 0.01], refine=2)
        assert len(out) == 4 and all(e.calls[-1] == {"lag_bounds": None, "band": None, "whiten": False, "fine": False, "refine": 2}
                                     for e in _StubCaf.instances)
        assert len(eng.caf(iq, [0.0, 0.01])) == 4 and all(e.calls[-1] == {} for e in _StubCaf.instances)   # the plain call as before
        with pytest.raises(ValueError, match="refine"):
            eng.caf(iq, [0.0], refine=3)
