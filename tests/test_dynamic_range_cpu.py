"""The dynamic-range helpers (tests/dynamic_range_ref.py) checked on the CPU, so that what tests/test_gpu_dynamic_range.py
holds the kernels to is itself held to something:

  * exponents() holds the slots it promises: the two ends, the mixed pair, a loud window directly in front of a quiet one
    and the reverse, and an unscaled control window;
  * the float32 oracle (oracle.xcorr_batch_literal: scipy's correlate, pocketfft in single precision) meets the exact rule
    -- lag_int and lag_frac bit for bit those of the unscaled input, peak = ldexp(peak of the unscaled input, e_i + e_j)
    exactly -- under exponents() and under the uniform exponents -20, -7, +8 and +14, on every level, at every length:
    the rule is a property of IEEE arithmetic and the scenes stay inside float32's normal range;
  * every scene the GPU test uses has a relative top-two margin >= 1e-3 on every slot (the bar of
    test_far_lag_ref_cpu.py): no near-tie excuse on the GPU;
  * the unit and int16 levels do fill 24-bit mantissas, the uint8 grid has 8;
  * the analytic result of coherent_window is what the float64 reference computes."""
import numpy as np
import pytest

import dynamic_range_ref as D
import far_lag_ref as F
from oracle import xcorr_ref as orc
from test_gpu_far_lags import ROUTES

LENGTHS = (256, 1024, 2048, 4096, 8192, 16384, 65536, 1 << 20)
LAYOUT_SHAPES = [(4096, 3, 8), (256, 4, 8), (8192, 3, 4)]       # the stored-spectrum layouts of the GPU test
GPU_SHAPES = sorted({(r[1], r[2], D.windows_for(r[1])) for r in ROUTES} | set(LAYOUT_SHAPES))


def test_exponents_hold_the_forced_slots():
    for W, B in ((8, 2), (8, 3), (8, 8), (5, 4), (16, 5)):
        e = D.exponents(W, B, 3)
        assert e.shape == (W, B) and e.min() >= D.E_LO and e.max() <= D.E_HI
        assert not e[0].any()                                               # the unscaled control
        pairs = [(int(e[w, i]), int(e[w, j])) for w in range(W) for i in range(B) for j in range(i + 1, B)]
        assert {(D.E_LO, D.E_LO), (D.E_HI, D.E_HI), (D.E_LO, D.E_HI)} <= set(pairs)
        loud = [w for w in range(W) if np.all(e[w] == D.E_HI)]
        quiet = [w for w in range(W) if np.all(e[w] == D.E_LO)]
        assert any(w + 1 in quiet for w in loud) and any(w + 1 in loud for w in quiet)
        assert np.array_equal(e, D.exponents(W, B, 3))
        if W > 5:
            assert not np.array_equal(e[5:], D.exponents(W, B, 4)[5:])      # the rest is seeded
    e = D.exponents(4, 3, 1)                                                # what fits: four-step layout of the GPU test
    assert not e[0].any() and list(e[1]) == [D.E_LO, D.E_LO, D.E_HI] and np.all(e[2] == D.E_HI) and np.all(e[3] == D.E_LO)
    e = D.exponents(2, 3, 1)
    assert not e[0].any() and list(e[1]) == [D.E_LO, D.E_LO, D.E_HI]
    assert list(D.exponents(1, 2, 1)[0]) == [D.E_LO, D.E_HI]


def test_scaled_and_expect_peak_are_exact():
    iq = D.scene(256, 3, 8, "unit")["iq"]
    e = D.exponents(8, 3, 5)
    s = D.scaled(iq, e)
    assert s.dtype == np.complex64
    back = D.scaled(s, -e)
    assert back.tobytes() == iq.tobytes()                                   # nothing rounded, nothing subnormal
    assert np.array_equal(s[0], iq[0])
    pk = np.float32([[3.0, 5.0, 7.0]] * 8)
    pl = orc.pair_list(3)
    want = pk.astype(np.float64) * 2.0 ** (e[:, pl[:, 0]] + e[:, pl[:, 1]])
    assert np.array_equal(D.expect_peak(pk, e, pl).astype(np.float64), want)


def test_levels_fill_the_mantissas_they_promise():
    for N in (256, 4096):
        assert D.mantissa_bits(D.scene(N, 3, 8, "u8grid")["iq"]) == 8
        for level, top in (("unit", 1.0), ("int16", 32767.5)):
            iq = D.scene(N, 3, 8, level)["iq"]
            assert D.mantissa_bits(iq) == 24
            assert 0.05 * top < np.abs(iq.view(np.float32)).max() <= top


def _oracle_rule(iq, e, pairs, what):
    base = orc.xcorr_batch_literal(iq, pairs)
    got = orc.xcorr_batch_literal(D.scaled(iq, e), pairs)
    assert np.array_equal(got[0], base[0]), what
    assert np.asarray(got[1]).tobytes() == np.asarray(base[1]).tobytes(), what
    want = D.expect_peak(base[2], e, pairs)
    assert np.all(np.isfinite(want)) and np.all(want >= np.finfo(np.float32).tiny), what
    assert np.asarray(got[2], np.float32).tobytes() == want.tobytes(), what


@pytest.mark.parametrize("N", LENGTHS)
def test_float32_oracle_meets_the_exact_rule(N):
    B, W = (3, D.windows_for(N)) if N < 1 << 20 else (2, 1)
    for level in D.LEVELS:
        s = D.scene(N, B, W, level)
        _oracle_rule(s["iq"], D.exponents(W, B, N % 1009), s["pairs"], (N, level, "per buoy"))
        _oracle_rule(s["iq"], D.exponents(W, B, N % 1009 + 1), s["custom"], (N, level, "per buoy, custom list"))
        if N <= 4096 or level == "u8grid":
            for k in (-20, -7, 8, 14):
                _oracle_rule(s["iq"][:2], np.full((len(s["iq"][:2]), B), k), s["pairs"], (N, level, k))


@pytest.mark.parametrize("N,B,W", GPU_SHAPES, ids=["%d-%d-%d" % s for s in GPU_SHAPES])
def test_every_scene_has_a_margin(N, B, W):
    for level in D.LEVELS:
        s = D.scene(N, B, W, level)
        worst = min(s["ref"][3].min(), s["cref"][3].min())
        print("N = %d, B = %d, W = %d, %s: smallest top-two margin %.4f, |lag| up to %d" % (N, B, W, level, worst, np.abs(s["ref"][0]).max()))
        assert worst >= 1e-3, (N, B, W, level, worst)
        c = s["custom"]
        assert np.array_equal(s["cref"][0][:, 0], -s["cref"][0][:, 1]) and not s["cref"][0][:, 2].any()   # mirror, self pair


def test_coherent_window_is_analytic():
    for N, k in ((256, 0), (4096, 14), (1024, -20)):
        x, li, lf, pk = D.coherent_window(N, k)
        assert x.dtype == np.complex64 and np.all(x == x[0]) and x[0] == complex(127.5 * 2.0 ** k, 127.5 * 2.0 ** k)
        ri, rf, rp, mg = F.ref64(x, x)
        assert (ri, li, lf) == (0, 0, 0.0) and abs(rf) < 1e-9 and abs(rp - pk) <= 1e-12 * pk
        assert abs(mg - 1.0 / N) < 1e-9                                     # the triangle (N - |lag|) |a|^2
