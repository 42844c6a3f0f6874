"""tests/large_batch_ref.py on the CPU: the boundary planner's arithmetic, the periodic index map, the base windows every
case of tests/test_gpu_large_batches.py runs (distinct, and no slot excused for its margin), and the proof that the
comparison has teeth: for every row of the matrix, what each of three narrow address rules would read, and that the
comparison reports it -- which it would not with a period that divides the wrap."""
import numpy as np
import pytest

import caf_ref as cr
import far_lag_ref as F
import integrated_ref as ir
import large_batch_ref as lb
import refined_ref as rr
import weighted_ref as wr
from oracle import xcorr_ref as orc

CASES = list(lb.CASES.values())
IDS = [c["id"] for c in CASES]


def test_boundary_plan_arithmetic():
    p = lb.boundary_plan(8 * 4096 * 8)
    assert p["windows"] == 16448 and p["first_beyond"] == 16384 and p["straddle32"] == [16383, 16384] and p["straddle31"] == [8191, 8192]
    assert p["elem31"] is None                                     # complex64 element 2^31 is byte 2^34
    p = lb.boundary_plan(8 * 8192, 1)                              # the uint8 door: byte = sample-part index
    assert p["windows"] == 65600 and p["elem31"] == 32768          # index 2^31 is the first byte of window 32768
    p = lb.boundary_plan(3 * 65536 * 8)                            # not a power of two: one window straddles
    assert p["windows"] == 2795 and p["straddle32"] == [2730] and p["straddle31"] == [1365] and p["first_beyond"] == 2731
    assert 2730 * 3 * 65536 * 8 < 1 << 32 < 2731 * 3 * 65536 * 8
    assert (p["windows"] - lb.TAIL) * p["bytes_per_window"] >= 1 << 32 > (p["windows"] - lb.TAIL - 1) * p["bytes_per_window"]
    # the shapes of the matrix: the planner's own count for the inputs ...
    want = {"I1": 16448, "I2": 65600, "I3": 8256, "I4": 4160, "I6": 32832, "I7": 2795, "I8": 16448, "I5-g_win_fused": 65600,
            "I5-g_win_scr": 16448, "I5-g_win_scr14": 8256, "I5-g_win_eo15": 4160}
    for c in CASES:
        if c["planned"]:
            assert c["W"] == want[c["id"]] == lb.boundary_plan(c["unit_bytes"], c["elem"])["windows"], c["id"]
        else:   # ... and the given shapes of the scratch rows cross with their last TAIL windows wholly beyond
            assert (c["W"] - lb.TAIL) * c["upw"] * c["unit_bytes"] >= 1 << 32, c["id"]
        assert c["T"] in (5, 7)
    assert "byte 2^32 in unit [2730]" in lb.describe(p)


def test_periodic_maps():
    assert lb.window_map(10, 7).tolist() == [0, 1, 2, 3, 4, 5, 6, 0, 1, 2]
    for T, K, W in ((7, 2, 4800), (5, 3, 300), (7, 4, 56)):
        m = lb.group_members(T, K)
        wm = lb.window_map(W, T).reshape(W // K, K)
        assert np.array_equal(wm, m[np.arange(W // K) % T])          # group g of the batch is reference group g % T
        assert len({tuple(r) for r in m.tolist()}) == T               # T distinct groups
    base = np.arange(7 * 2 * 3).reshape(7, 2, 3)
    g = lb.group_scene(base, 2)
    assert g.shape == (14, 2, 3) and np.array_equal(g[2 * 5 + 1], base[(2 * 5 + 1) % 7])
    a, b = lb.expand((np.arange(7), np.arange(14).reshape(7, 2)), 16, 7)
    assert a.tolist() == [0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3, 4, 5, 6, 0, 1] and b[15].tolist() == [2, 3]
    assert lb.expand({"x": np.arange(5)}, 7, 5)["x"].tolist() == [0, 1, 2, 3, 4, 0, 1]


def test_wrong_rule_on_a_small_buffer():
    """units of 2^30 bytes, 8-byte elements, six units: what each rule reads"""
    kind, src = lb.wrong_rule(lb.RULES[0], 1 << 30, 8, 6)
    assert kind.tolist() == [lb.RIGHT] * 4 + [lb.OTHER] * 2 and src.tolist() == [0, 1, 2, 3, 0, 1]
    kind, src = lb.wrong_rule(lb.RULES[1], 1 << 30, 8, 6)
    assert kind.tolist() == [lb.RIGHT] * 2 + [lb.OUTSIDE] * 2 + [lb.OTHER] * 2 and src.tolist() == [0, 1, -1, -1, 0, 1]
    kind, _ = lb.wrong_rule(lb.RULES[2], 1 << 30, 8, 6)
    assert kind.tolist() == [lb.RIGHT] * 6                            # element 2^31 is byte 2^34
    kind, src = lb.wrong_rule(lb.RULES[2], 1 << 30, 1, 6)
    assert kind.tolist() == [lb.RIGHT] * 2 + [lb.OUTSIDE] * 2 + [lb.OTHER] * 2
    kind, src = lb.wrong_rule(lb.RULES[0], 3 << 29, 8, 4)               # 1.5 GiB units: unit 2 holds byte 2^32 and is torn
    assert kind.tolist() == [lb.RIGHT, lb.RIGHT, lb.TORN, lb.TORN] and src[3] == 0


def _lags_of(c):
    """S4's units are product slots: the reference's integer lag of every (base window, pair)"""
    if c["upw"] == 1:
        return None
    iq, _, _ = lb.base_scene(c["N"], c["B"], c["T"])
    return wr.weighted_batch(iq, None, True)[0]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_comparison_reports_every_wrong_rule(c):
    """every row of the matrix x the three rules: each window of which a rule misreads a unit fails the comparison; the two
    byte rules misread the last TAIL windows of every row; and the rows' T is what makes it so"""
    W, T, upw = c["W"], c["T"], c["upw"]
    lags = _lags_of(c)
    for rule in lb.RULES:
        hit = lb.wrapped(rule, c["unit_bytes"], c["elem"], W, upw)
        seen = lb.reported(rule, c["unit_bytes"], c["elem"], W, T, upw, lags)
        assert np.array_equal(hit, seen), (c["id"], rule, int(hit.sum()), int(seen.sum()), np.flatnonzero(hit & ~seen)[:8])
        if rule != lb.RULES[2]:
            assert hit[-lb.TAIL:].all() and not hit[0], (c["id"], rule)
        elif c["elem"] == 1:
            assert hit[-lb.TAIL:].all()          # the uint8 door: element index 2^31 is byte 2^31
        else:
            assert not hit.any()                 # 8- and 16-byte elements: index 2^31 lies beyond every buffer of the matrix
    # a period that divides the wrap hides it: with T = 8 the uint32 rule passes unseen wherever the unit is a power of two
    bpu = c["unit_bytes"]
    if bpu & (bpu - 1) == 0 and upw == 1:
        shift = (1 << 32) // bpu
        assert shift % T != 0 and shift % 8 == 0
        assert not lb.reported(lb.RULES[0], bpu, c["elem"], W, 8, upw).any()
        assert lb.wrapped(lb.RULES[0], bpu, c["elem"], W, upw)[-lb.TAIL:].all()


SCENES = sorted({(c["N"], c["B"], c["T"]) for c in CASES} | {(1024, 8, 7), (1024, 10, 7)})   # (+ the grid-row cases)


@pytest.mark.parametrize("N,B,T", SCENES, ids=["N%d-B%d-T%d" % s for s in SCENES])
def test_base_windows_are_distinct_and_no_slot_is_excused(N, B, T):
    """any two base windows differ in the reference's integer lag on at least one pair, and every slot's top-two margin
    exceeds 1e-5: the GPU file compares every slot of every batch"""
    iq, raw, _ = lb.base_scene(N, B, T)
    assert np.array_equal(iq, ((raw[..., 0::2].astype(np.float32) - np.float32(127.5))
                               + 1j * (raw[..., 1::2].astype(np.float32) - np.float32(127.5))).astype(np.complex64))
    li, lf, pk, mg = F.ref64_batch(iq, orc.pair_list(B))
    assert lb.distinct(li) and mg.min() > 1e-5, (float(mg.min()))
    assert np.abs(li).max() > F.noise_top(N) // 2                     # the lags are spread over the range


def test_feature_references_excuse_no_slot():
    """the references of the weighted, refined, integrated and Doppler-search cases on their base windows"""
    iq, _, _ = lb.base_scene(4096, 20, 5)                              # S1
    ref = wr.weighted_batch(iq, None, True)
    assert ref[3].min() > 1e-5 and lb.distinct(ref[0])
    ref = rr.refined_batch(iq, 4)
    assert ref[3].min() > 1e-5 and lb.distinct(ref[0])
    iqd, _, k = lb.base_scene(4096, 20, 5, doppler=True)               # S2
    ref = cr.reference(iqd, lb.caf_grid(4096))
    pl = orc.pair_list(20)
    assert ref["hyp_margin"].min() > cr.MARGIN_BAR and ref["lag_margin"].min() > 1e-5 and lb.distinct(ref["lag_int"])
    assert np.array_equal(ref["dop"], k[:, pl[:, 1]] - k[:, pl[:, 0]] + 1)
    iq, _, _ = lb.base_scene(8192, 16, 7)                              # S4 / G1
    ref = wr.weighted_batch(iq, None, True)
    assert ref[3].min() > 1e-5 and lb.distinct(ref[0])
    for B in (8, 10):                                                  # G2, integrate = 2
        iq, _, _ = lb.base_scene(1024, B, 7)
        ref = ir.integrated_batch(lb.group_scene(iq, 2), 2)
        assert ref[0].shape == (7, B * (B - 1) // 2) and ref[3].min() > 1e-5 and lb.distinct(ref[0])
