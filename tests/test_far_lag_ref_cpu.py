"""The far-lag scenes and their float64 reference (tests/far_lag_ref.py) checked on the CPU, so that what
tests/test_gpu_far_lags.py holds the kernels to is itself held to something:

  * every lag of the target list is the float64 lag_int of a designed (window, pair) slot, and every designed slot --
    two-buoy, both orders; multi-buoy, every ordered pair; none left out -- has a relative top-two margin >= 1e-3, so the
    GPU test needs no near-tie excuse;
  * the impulse scene's analytic reference is what ref64 computes;
  * the float32 oracle (oracle.xcorr_batch_literal: scipy's correlate, pocketfft in single precision) meets the GPU test's
    bars against ref64 on the noise scenes: integer lags equal, lag_frac within 1e-5 ABSOLUTE, peak within 1e-5 relative.

Measured here (10 dB, two-buoy scenes, both orders of the pair; worst over the windows of a length):

      N     windows  int mismatches  |dfrac|   |dpeak|/peak  min margin  min |a-2b+c|/b
     256        77         0         2.3e-07     2.4e-07       0.0095        0.73
    1024       137         0         2.6e-07     2.8e-07       0.0040        0.78
    2048       143         0         2.8e-07     2.8e-07       0.0095        0.74
    4096       166         0         2.2e-07     3.2e-07       0.0118        0.80
    8192       208         0         3.0e-07     3.1e-07       0.0046        0.80
   16384       226         0         2.6e-07     3.6e-07       0.0154        0.80
   65536        85         0         1.7e-07     3.7e-07       0.0070        0.81
 1048576         2         0         6.1e-08     2.5e-07       0.2915        1.20

so the 1e-5 absolute bar on lag_frac has 33 x headroom or more over another float32 transform, at every lag."""
import numpy as np
import pytest

import far_lag_ref as F
from oracle import xcorr_ref as orc

LENGTHS = (256, 1024, 2048, 4096, 8192, 16384, 65536, 1 << 20)
MULTI = {256: (4, 5), 1024: (4, 5), 2048: (4, 5), 4096: (8,), 8192: (8,), 16384: (5,), 65536: (3, 8), 1 << 20: ()}


def test_target_list_holds_what_it_promises():
    for N in LENGTHS[:-1]:
        t = set(F.target_lags(N, 1).tolist())
        top = F.top_lag(N)
        assert top == N - N // 8 and {0, 1, -1, top, -top} <= t and max(abs(v) for v in t) == top
        k = 1
        while (1 << k) < top:
            assert {s * ((1 << k) + d) for s in (1, -1) for d in (-1, 0, 1)} <= t, (N, k)
            k += 1
        for m in range(1, 8):
            want = {s * (m * N // 8 + d) for s in (1, -1) for d in (-1, 0, 1)}
            assert {v for v in want if abs(v) <= top} <= t, (N, m)
        assert set(F.seam_lags(N, 1)) <= t
        for s in F.STRIDES[N]:                     # a seam of every stride in the far half, with the lag below it
            assert any(v % s == 0 and v > top // 2 and v - 1 in t for v in t), (N, s)
            assert any(v % s == 0 and v < -top // 2 and v - 1 in t for v in t), (N, s)
        other = set(F.target_lags(N, 2).tolist())
        assert 16 <= len(t ^ other) <= 2 * (32 + 6 * len(F.STRIDES[N]))   # the seeded part: 32 lags, one seam (x 6) per stride


def test_pack_places_every_window_at_a_designed_pair():
    x = np.arange(7 * 2 * 3).reshape(7, 2, 3)
    for B in (2, 3, 4, 5, 8):
        y, src = F.pack(x, B)
        des, cols = F.designed_pairs(B)
        assert y.shape[1] == B and set(src.ravel().tolist()) == set(range(7))
        dflt = orc.pair_list(B)
        for v in range(y.shape[0]):
            for g, (i, j) in enumerate(des):
                assert np.array_equal(y[v, i], x[src[v, g], 0]) and np.array_equal(y[v, j], x[src[v, g], 1])
                assert tuple(dflt[cols[g]]) == (i, j)


@pytest.mark.parametrize("N", LENGTHS)
def test_every_target_lag_is_designed_with_a_margin(N):
    s = F.two_buoy(N)
    assert np.array_equal(s["ref"][0], s["lags"]) and np.array_equal(s["rev"][0], -s["lags"])
    assert min(s["ref"][3].min(), s["rev"][3].min()) >= 1e-3
    assert np.all(np.abs(s["true"] - s["lags"]) < 0.5) and np.ptp(s["true"] - s["lags"]) > 0.8 or N == 1 << 20
    assert np.abs(s["ref"][1]).max() > 0.4 or N == 1 << 20          # lag_frac is exercised
    lags = F.impulse_lags(N)
    for B in (2, 5, 8):
        iq, pos, amp = F.impulse_scene(N, lags, B, 5)
        assert np.all((pos >= 0) & (pos < N)) and np.count_nonzero(iq) == pos.size
        got = set((pos[:, 1:] - pos[:, :1]).ravel().tolist())
        assert got == set(lags.tolist())
        pairs = F.mirrored(orc.pair_list(B))
        ai, ap = F.impulse_ref(pos, amp, pairs)
        for w in {0, len(iq) // 2, len(iq) - 1} if N <= 65536 else ():
            li, lf, pk, mg = F.ref64_batch(iq[w:w + 1], pairs)
            assert np.array_equal(li[0], ai[w]) and np.allclose(pk[0], ap[w], rtol=1e-6) and np.abs(lf).max() <= 1e-5
            assert mg.min() > 0.999
    found = set(s["ref"][0].tolist()) | set(s["rev"][0].tolist()) | set(lags.tolist())
    if N < 1 << 20:
        assert set(F.target_lags(N, F.SEED + N % 1009).tolist()) <= found
        assert {-(N - 1), -(N - 2), N - 2, N - 1} <= found
    for B in MULTI[N]:
        m = F.multi_buoy(N, B)
        assert m["ref"][3].min() >= 1e-3, (B, m["ref"][3].min())
        true = m["delays"][:, m["pairs"][:, 1]] - m["delays"][:, m["pairs"][:, 0]]
        assert np.abs(m["ref"][0] - true).max() < 1.0
        assert np.abs(m["ref"][0]).max() > 0.5 * F.noise_top(N)     # the pairs' lags do spread over the range


def test_exhaustive_impulse_scenes_hold_every_lag():
    for N, B in ((256, 4), (256, 5), (4096, 8)):
        iq, pos, amp = F.impulse_scene(N, np.arange(-(N - 1), N), B, 9)
        assert set((pos[:, 1:] - pos[:, :1]).ravel().tolist()) == set(range(-(N - 1), N))
        assert len(iq) == -(-(2 * N - 1) // (B - 1))


@pytest.mark.parametrize("N", LENGTHS)
def test_float32_oracle_meets_the_bars_against_ref64(N):
    """the figures of the module docstring: another float32 implementation against the float64 reference"""
    s = F.two_buoy(N)
    oi, of_, op = orc.xcorr_batch_literal(s["iq"], np.array([(0, 1), (1, 0)], np.int32))
    worst_f = worst_p = 0.0
    for col, ref in ((0, s["ref"]), (1, s["rev"])):
        assert np.array_equal(oi[:, col], ref[0])
        worst_f = max(worst_f, float(np.abs(of_[:, col] - ref[1]).max()))
        worst_p = max(worst_p, float((np.abs(op[:, col].astype(np.float64) - ref[2]) / ref[2]).max()))
        assert np.all(np.abs(of_[:, col] - ref[1]) <= 1e-5)
        assert np.all(np.abs(op[:, col].astype(np.float64) - ref[2]) <= 1e-5 * ref[2])
    curv = []
    for w in range(len(s["iq"])):
        m = np.abs(orc.xcorr_full_numpy(s["iq"][w, 0], s["iq"][w, 1])).astype(np.float64)
        k = int(s["ref"][0][w]) + N - 1
        curv.append(abs(m[k - 1] - 2 * m[k] + m[k + 1]) / m[k])
    print(f"N={N}: {len(s['iq'])} windows, 0 integer mismatches, worst |dfrac| {worst_f:.1e}, worst |dpeak|/peak {worst_p:.1e}, "
          f"min margin {min(s['ref'][3].min(), s['rev'][3].min()):.4f}, min curvature {min(curv):.2f}")
    for B in MULTI[N]:
        m = F.multi_buoy(N, B)
        oi, of_, op = orc.xcorr_batch_literal(m["iq"], m["pairs"])
        assert np.array_equal(oi, m["ref"][0])
        assert np.all(np.abs(of_ - m["ref"][1]) <= 1e-5) and np.all(np.abs(op - m["ref"][2]) <= 1e-5 * m["ref"][2])
