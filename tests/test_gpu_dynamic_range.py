"""Every route across the input's dynamic range, per buoy and window.

Every other GPU test feeds the kernels rtl_sdr's level (+-127.5, 8 significant bits).  Each route carries its own
power-of-two scaling scheme, searches |c|^2 and not |c|, and resolves taps through sign sentinels and `> 0` branches: a
scale placed one step late, an epsilon, an absolute threshold, or state that leaks from a loud window into the next quiet one
on a persistent workgroup is invisible at one level.  Here (helpers and their CPU checks: tests/dynamic_range_ref.py,
tests/test_dynamic_range_cpu.py):

 a. every route of tests/test_gpu_far_lags.py, steered and asserted as there, runs a batch with every (window, buoy) scaled
    by its own 2^e, e in -20 ... +14 (the ends, the mixed pair, loud / quiet neighbours forced), default and custom pair
    list.  Scaling by a power of two commutes with every IEEE operation the kernels use, so against the call on the
    unscaled batch lag_int and lag_frac must be bit-identical and peak must equal ldexp(peak, e_i + e_j) exactly -- the
    float32 oracle meets that rule bit for bit (test_dynamic_range_cpu.py).  The unscaled call is held to the float64
    reference with the bars of test_gpu_far_lags._assert_bars.
 b. the request entries on the three stored-spectrum layouts under the same exponents: bounded, band, integrate = K (one
    exponent per group and buoy), refine = 8 and the Doppler search (fine = True too) by the same rule; quality = True: the
    four figures bit-identical (every sum scales by an exact power of two, every figure is a ratio); whiten = True: all
    three outputs bit-identical to the unscaled call; groups whose windows differ in level against tests/integrated_ref.py.
 c. full 24-bit mantissas (+-1 floats through a non-power-of-two normalisation, int16-scaled floats) on every route of (a)
    against the float64 reference with _assert_bars unchanged.
 d. the top of the range: a fully coherent full-scale window at the largest exponent each route's stored scales allow
    (TOP, derived below), and at +14, is finite and equals its analytic result.
 e. detect() on uniformly scaled batches (2^-7, 2^8) with the threshold moved by 20 log10(2^k).

Measured on an MI355X (every assertion of this file holds there):
  * (a), (b): no slot of any route or request deviates from the exact rule in a single bit.
  * whiten = True is bit-identical in lag_int, lag_frac and peak on all three layouts, with and without a band (v_rsq_f32
    returns the same mantissa when the exponent of its argument moves by an even number): that is what is asserted.
  * (c), worst over the 24 routes, default and custom list:   |dfrac|    |dpeak| / peak
        +-1 floats, 24-bit mantissas                            3.8e-07    4.8e-07     (both on 16384-g_win_eo15)
        int16-scaled floats, 24-bit mantissas                   3.6e-07    4.5e-07
        the uint8 grid at the same seeds (the control of (a))   3.6e-07    5.0e-07
    so the 1e-5 bars measured on 8-bit data hold unchanged on full mantissas.
  * (d): the peak of the coherent window is within 6.0e-8 of N |a|^2 on every route at every tested exponent; lag_frac is
    bounded by the flat-peak rule only (0.016 at N = 2^20, where one ulp on a tap of the triangle moves the vertex by 0.03).
  * what the file catches and the older suites do not (each tried once on a local build, test_gpu_parity.py and
    test_gpu_weighted.py passing): `m2 > 1e-12f` instead of `m2 > 0.0f` in xweight_apply fails the three whiten tests;
    `+ 1e-12f` on the two neighbour taps' squared magnitudes in k_win's resolve fails (a) on 4096-k_win.  `m2 > 1e-30f` is
    NOT caught, and is not wrong on this range: the smallest stored |X|^2 at 2^-20 is near 1e-12 (mean 1e-9), so a threshold
    of 1e-30 never fires above samples of 2^-55.  `+ 1e-12f` on the PEAK's squared magnitude is caught here and by
    test_gpu_parity.py's all-zero window alike.
"""
import numpy as np
import pytest

import caf_ref as cr
import dynamic_range_ref as D
import integrated_ref as ir
import quality_ref as qr
from oracle import xcorr_ref as orc
from test_gpu_far_lags import ROUTES, _assert_bars, _run, _windows_of

pytestmark = pytest.mark.gpu

TINY = np.finfo(np.float32).tiny


@pytest.fixture(scope="module")
def xc():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    assert xcorr.device_count() > 0, "no MI355X visible"
    return xcorr


@pytest.fixture
def opts(xc):
    xc.clear_default_options()
    yield xc.set_default_option
    xc.clear_default_options()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.int64)


def _assert_rule(got, base, e, pairs, what):
    """the exact rule: got = the call on scaled(iq, e), base = the call on iq; lag_int, lag_frac bit for bit, peak =
    ldexp(base peak, e_i + e_j) bit for bit.  Prints the count and the exponents of the first offenders first."""
    p = np.asarray(pairs).reshape(-1, 2)
    want = D.expect_peak(base[2], e, p)
    assert np.all(np.isfinite(want)) and np.all(want >= TINY), (what, "the expectation itself leaves float32's normal range")
    ei, ej = e[:, p[:, 0]], e[:, p[:, 1]]
    bad = [_bits(got[0]) != _bits(base[0]), _bits(got[1]) != _bits(base[1]), _bits(got[2]) != _bits(want)]
    print("%s: %d slots, differing lag_int %d, lag_frac %d, peak %d" % (what, want.size, *(int(b.sum()) for b in bad)))
    for name, b, g, w in zip(("lag_int", "lag_frac", "peak"), bad, got, (base[0], base[1], want)):
        if b.any():
            rows = ["(w %d, pair %s, e %d %d: got %r want %r)" % (r, tuple(p[c]), ei[r, c], ej[r, c], g[r, c], w[r, c])
                    for r, c in zip(*np.nonzero(b))][:6]
            print("  %s: %s" % (name, " ".join(rows)))
    for name, b in zip(("lag_int", "lag_frac", "peak"), bad):
        assert not b.any(), "%s: %s of %d slots is not that of the unscaled call" % (what, name, int(b.sum()))


def _steer(opts, dflt):
    for k, v in dflt.items():
        opts(k, v)


def _engine(xc, B, N, W, eopts=()):
    eng = xc.XcorrEngine(B, N, W)
    eng.set_option("timing", 1)
    for k, v in dict(eopts).items():
        eng.set_option(k, v)
    return eng


# ---- a. exact per-buoy equivariance on every route ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,B,dflt,eopts,fam,fam_custom,exhaustive", ROUTES, ids=[r[0] for r in ROUTES])
def test_route_is_equivariant_under_per_buoy_levels(xc, opts, name, N, B, dflt, eopts, fam, fam_custom, exhaustive):
    """one route: the smallest batch that reaches it (8 windows up to N = 16384, 2 at 65536, 1 at 2^20), default list and a
    custom list holding a pair, its mirror and a self pair"""
    _steer(opts, dflt)
    W = D.windows_for(N)
    s = D.scene(N, B, W)
    iq = s["iq"]
    with _engine(xc, B, N, W, eopts) as eng:
        for pairs, ref, arg, f, seed in ((s["pairs"], s["ref"], None, fam, 1), (s["custom"], s["cref"], s["custom"], fam_custom, 2)):
            what = "%s, %s list" % (name, "default" if arg is None else "custom")
            e = D.exponents(W, B, 31 * N % 1009 + seed)
            base = _run(eng, iq, arg, f, what)
            got = _run(eng, D.scaled(iq, e), arg, f, what + ", scaled")
            _assert_bars(base, ref[:3], _windows_of(iq, pairs), what + ", unscaled against float64")
            _assert_rule(got, base, e, pairs, what)


# ---- c. full mantissas -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,B,dflt,eopts,fam,fam_custom,exhaustive", ROUTES, ids=[r[0] for r in ROUTES])
def test_full_mantissas_against_float64(xc, opts, name, N, B, dflt, eopts, fam, fam_custom, exhaustive):
    """+-1 floats (a non-power-of-two normalisation) and int16-scaled floats: 24 significant bits in every sample, so no
    butterfly stage is exact; the header's bars unchanged"""
    _steer(opts, dflt)
    W = D.windows_for(N)
    with _engine(xc, B, N, W, eopts) as eng:
        for level in ("unit", "int16"):
            s = D.scene(N, B, W, level)
            got = _run(eng, s["iq"], None, fam, name + " " + level)
            _assert_bars(got, s["ref"][:3], _windows_of(s["iq"], s["pairs"]), "%s, %s, default list" % (name, level))
            got = _run(eng, s["iq"], s["custom"], fam_custom, name + " " + level + " custom")
            _assert_bars(got, s["cref"][:3], _windows_of(s["iq"], s["custom"]), "%s, %s, custom list" % (name, level))


# ---- d. the top of the range -----------------------------------------------------------------------------------------------------
# Every route computes c_s = c / out_scale, searches |c_s|^2 = re^2 + im^2 in float32 and returns sqrt(|c_s|^2) out_scale:
# the forward spectra carry 2^-u, the product 2^-2u, the unnormalised inverse transform multiplies by L (and, on the k_win
# network, by the TW1 table's 2^-6 once more), so out_scale = 2^s with
#     k_win, k_fwd + k_pair (N = 4096)   u = 6, L = 2^13: c_s = c 2^(13 - 18)             s = 3 x 6 - 13 = 5   (out_scale4096)
#     k_win8kl (N = 8192)                the same network, L = 2^14                        s = 3 x 6 - 14 = 4
#     k16_fwd + k16_pairs (N = 16384)    the same network, L = 2^15                        s = 3 x 6 - 15 = 3
#     every other kernel                 u = hs = floor(logL / 2): c_s = c 2^(logL - 2 hs)  s = -(logL - 2 hs) = 0 (logL even), -1 (odd)
# (the ldexp lines of rmx_hip.hip; g_rows_fused applies 2^-2hs to the product instead of 2^-hs to each spectrum).  Everything
# in front of the squares is linear in the samples or a product of two spectra, far below the square of the result.  For
# the fully coherent full-scale window a = (127.5 + 127.5j) 2^k the largest |c| is the self correlation at lag 0,
# c = N |a|^2 = N 32512.5 4^k, and all partial sums of the inverse transform are bounded by it (the cross-spectrum is
# |X|^2 >= 0).  |c_s|^2 stays finite while N 32512.5 4^k 2^-s < 2^64, i.e. |sample| < 2^32 sqrt(out_scale / N):
#     2 k < 64 - log2(32512.5) - log2 N + s = 49.011 - log2 N + s.
# k_quality forms EE = (A / L)(B / L) = (N |a|^2)^2 and sum |X_i|^2 |X_j|^2 >= (N |a| 2^-u)^4 in float32: both finite while
# N |a|^2 < 2^64 (the second because u = floor(logL / 2) or 6 at L = 2^13): 2 k < 49.011 - log2 N, TOP_Q.
TOP = {   # route -> (s, the largest k)
    "4096-k_win": (5, 21), "4096-k_fwd+k_pair": (5, 21), "4096-k_fwd+k_pair-fused0": (5, 21), "4096-g_small": (-1, 18),
    "256-g_win_fused": (-1, 20), "256-g_win_scr": (-1, 20), "256-g_small": (-1, 20),
    "1024-g_win_fused": (-1, 19), "1024-g_win_scr": (-1, 19), "1024-g_small": (-1, 19),
    "2048-g_win_fused": (0, 19), "2048-g_win_scr": (0, 19), "2048-g_small": (0, 19),
    "8192-k_win8kl": (4, 20), "8192-g_win_scr14": (0, 18), "8192-g_win_scr-1024thr": (0, 18), "8192-four-step": (0, 18),
    "16384-k16": (3, 19), "16384-g_win_eo15": (-1, 17), "16384-four-step": (-1, 17),
    "65536-g_rows_fused": (-1, 16), "65536-g_rows_fwd+inv": (-1, 16), "65536-g_rows_anchor": (-1, 16),
    "1048576-four-step": (-1, 14),
}
TOP_Q = {4096: 18, 256: 20, 8192: 18}


def _largest_k(N, s):
    k = 0
    while N * 32512.5 * 4.0 ** (k + 1) * 2.0 ** -s < 2.0 ** 64:
        k += 1
    return k


def test_the_table_is_the_derivation():
    assert set(TOP) == {r[0] for r in ROUTES}
    for name, N in ((r[0], r[1]) for r in ROUTES):
        s, k = TOP[name]
        logL = N.bit_length()                       # log2 (2 N)
        assert s == {"4096-k_win": 5, "4096-k_fwd+k_pair": 5, "4096-k_fwd+k_pair-fused0": 5, "8192-k_win8kl": 4,
                     "16384-k16": 3}.get(name, -(logL - 2 * (logL // 2))), name
        assert k == _largest_k(N, s) and k >= D.E_HI, (name, k)
    for N, k in TOP_Q.items():
        assert k == _largest_k(N, 0)


def _coherent_batch(N, B, ks):
    iq = np.empty((len(ks), B, N), np.complex64)
    peak = np.empty(len(ks))
    for w, k in enumerate(ks):
        iq[w], _, _, peak[w] = D.coherent_window(N, int(k))
    return iq, peak


@pytest.mark.parametrize("name,N,B,dflt,eopts,fam,fam_custom,exhaustive", ROUTES, ids=[r[0] for r in ROUTES])
def test_top_of_the_range(xc, opts, name, N, B, dflt, eopts, fam, fam_custom, exhaustive):
    """every buoy the constant window (127.5 + 127.5j) 2^k: windows alternate between k = TOP[route] and +14 (the header's
    4e6 at N = 4096).  Finite, lag 0, peak N |a|^2 within 1e-5 relative, lag_frac within the flat-peak bound (the triangle
    N - |lag| is flat: a - 2 b + c = -2 b / N)."""
    _steer(opts, dflt)
    W = D.windows_for(N)
    ks = np.where(np.arange(W) % 2 == 0, TOP[name][1], D.E_HI)
    iq, peak = _coherent_batch(N, B, ks)
    pairs = orc.pair_list(B)
    with _engine(xc, B, N, W, eopts) as eng:
        got = _run(eng, iq, None, fam, name + " coherent")
    assert np.all(np.isfinite(got[1])) and np.all(np.isfinite(got[2])), (name, got[2])
    shape = got[0].shape
    ref = (np.zeros(shape, np.int64), np.zeros(shape), np.broadcast_to(peak[:, None], shape))
    _assert_bars(got, ref, _windows_of(iq, pairs), "%s, coherent at 2^%s" % (name, sorted(set(ks.tolist()))))


# ---- b. the request entries on the three stored-spectrum layouts ----------------------------------------------------------------
LAYOUTS = [("k_fwd", 4096, 3, 8, 2), ("g_fwd_small", 256, 4, 8, 4), ("g_rows_fwd", 8192, 3, 4, 2)]   # (.., N, B, W, K)
layouts = pytest.mark.parametrize("fwd,N,B,W,K", LAYOUTS, ids=[l[0] for l in LAYOUTS])


def _both(xc, fwd, N, B, W, e, pairs=None, **kw):
    """the request on the unscaled scene and on the scaled one, through one engine -> (base, got, iq)"""
    iq = D.scene(N, B, W)["iq"]
    with _engine(xc, B, N, W) as eng:
        base = eng.correlate(iq, pairs, **kw)
        assert fwd in eng.last_timing_by_kernel(), (fwd, eng.last_timing_by_kernel())
        got = eng.correlate(D.scaled(iq, e), pairs, **kw)
        assert fwd in eng.last_timing_by_kernel()
    return base, got, iq


@layouts
def test_bounded_request(xc, opts, fwd, N, B, W, K):
    import test_gpu_weighted as tw
    P = B * (B - 1) // 2
    lb = tw._random_bounds(np.random.default_rng(N + 1), (W, P), N)
    e = D.exponents(W, B, N % 1009 + 3)
    base, got, _ = _both(xc, fwd, N, B, W, e, lag_bounds=lb)
    assert np.all((base[0] >= lb[..., 0]) & (base[0] <= lb[..., 1]))
    _assert_rule(got, base, e, orc.pair_list(B), "%s bounded" % fwd)


@layouts
def test_band_request(xc, opts, fwd, N, B, W, K):
    e = D.exponents(W, B, N % 1009 + 4)
    base, got, _ = _both(xc, fwd, N, B, W, e, band=(-0.31, 0.27))
    _assert_rule(got, base, e, orc.pair_list(B), "%s band" % fwd)
    cu = D.custom_pairs(B)
    base, got, _ = _both(xc, fwd, N, B, W, e, pairs=cu, band=(-0.31, 0.27))
    _assert_rule(got, base, e, cu, "%s band, custom list" % fwd)


@layouts
def test_integrated_request(xc, opts, fwd, N, B, W, K):
    """one exponent per (group, buoy), repeated over the group's K windows: the rule on [G][P]"""
    eg = D.exponents(W // K, B, N % 1009 + 5)
    base, got, _ = _both(xc, fwd, N, B, W, np.repeat(eg, K, axis=0), integrate=K)
    assert base[0].shape == (W // K, B * (B - 1) // 2)
    _assert_rule(got, base, eg, orc.pair_list(B), "%s integrate = %d" % (fwd, K))


@layouts
def test_integrated_groups_of_mixed_levels(xc, opts, fwd, N, B, W, K):
    """the windows of a group at different levels (0, +10, -7, +3 in turn; every buoy of a window alike): no exact rule --
    the loud window carries the sum --, so against tests/integrated_ref.py with the parity rule of test_gpu_integrated.py"""
    import test_gpu_integrated as ti
    iq = D.scene(N, B, W)["iq"]
    e = np.repeat(np.array([0, 10, -7, 3])[np.arange(W) % 4][:, None], B, axis=1)
    x = D.scaled(iq, e)
    with _engine(xc, B, N, W) as eng:
        got = eng.correlate(x, integrate=K)
        assert fwd in eng.last_timing_by_kernel()
    ti._assert_parity(*got, ir.integrated_batch(x, K, with_bound=True), "%s mixed-level groups, integrate = %d" % (fwd, K))


@layouts
def test_refined_request(xc, opts, fwd, N, B, W, K):
    e = D.exponents(W, B, N % 1009 + 6)
    base, got, _ = _both(xc, fwd, N, B, W, e, refine=8)
    _assert_rule(got, base, e, orc.pair_list(B), "%s refine = 8" % fwd)


@layouts
def test_quality_request(xc, opts, fwd, N, B, W, K):
    """the four figures bit for bit those of the unscaled call; the lag outputs by the rule"""
    e = D.exponents(W, B, N % 1009 + 7)
    base, got, _ = _both(xc, fwd, N, B, W, e, quality=True)
    _assert_rule(got, base, e, orc.pair_list(B), "%s quality" % fwd)
    diff = _bits(got[3]) != _bits(base[3])
    print("%s quality: figures that differ per column (coherence, psr, rms_bw, n_eff): %s of %d" % (
        fwd, diff.reshape(-1, 4).sum(axis=0), diff.size // 4))
    for r, c, q in list(zip(*np.nonzero(diff)))[:6]:
        print("  w %d pair %d figure %d: got %r want %r, e %s" % (r, c, q, got[3][r, c, q], base[3][r, c, q], e[r]))
    assert not diff.any()


@layouts
def test_quality_at_the_top_of_its_range(xc, opts, fwd, N, B, W, K):
    """the coherent full-scale window at TOP_Q (the fourth power and the energy product stay finite) and at +14"""
    import test_gpu_quality as tq
    ks = np.where(np.arange(W) % 2 == 0, TOP_Q[N], D.E_HI)
    iq, _ = _coherent_batch(N, B, ks)
    with _engine(xc, B, N, W) as eng:
        got = eng.correlate(iq, quality=True)
        assert "k_quality" in eng.last_timing_by_kernel()
    assert np.all(np.isfinite(got[2])) and not np.any(np.isnan(got[3]))
    tq._assert_quality(got[3], qr.quality_batch(iq), N, "%s coherent at 2^%d / 2^14" % (fwd, TOP_Q[N]))


@layouts
def test_whitened_request_is_invariant(xc, opts, fwd, N, B, W, K):
    """PHAT: lag_int, lag_frac and peak do not depend on the level at all.  m2 = |X|^2 moves by an even power of two, so
    v_rsq_f32 returns the same mantissa and x * rsq * unit the same bits: bit-identical on an MI355X (module docstring),
    which is what is asserted -- the entry's own parity bar (lag_int equal, lag_frac and peak within
    1e-5) is implied."""
    e = D.exponents(W, B, N % 1009 + 8)
    for kw in (dict(whiten=True), dict(whiten=True, band=(-0.31, 0.27))):
        base, got, _ = _both(xc, fwd, N, B, W, e, **kw)
        diff = [int((_bits(g) != _bits(b)).sum()) for g, b in zip(got, base)]
        dfr = float(np.abs(got[1] - base[1]).max())
        dpk = float((np.abs(got[2] - base[2]) / base[2]).max())
        print("%s %s: differing lag_int %d, lag_frac %d, peak %d of %d; worst |dfrac| %.2e, |dpeak| / peak %.2e" % (
            fwd, sorted(kw), *diff, got[0].size, dfr, dpk))
        assert np.array_equal(got[0], base[0]) and dfr <= 1e-5 and dpk <= 1e-5
        assert diff == [0, 0, 0]


CAF = [("one launch", 4096, 4, 8, 40), ("g_fwd_small", 1024, 3, 8, 1031)]


@pytest.mark.parametrize("what,N,B,W,seed", CAF, ids=[c[0] for c in CAF])
def test_doppler_search(xc, opts, what, N, B, W, seed):
    """caf() and the request with fine = True: 5 hypotheses 0.5 / N apart, a seeded on-grid offset per window and buoy.
    dop_idx, dop_frac, lag_int, lag_frac bit for bit; peak scaled exactly."""
    iq, _, grid, k = cr.scene(W, B, N, 5, seed)
    e = D.exponents(W, B, N % 1009 + 9)
    x = D.scaled(iq, e)
    pairs = orc.pair_list(B)
    with _engine(xc, B, N, W) as eng:
        base = eng.caf(iq, grid)
        launches = {n: v["launches"] for n, v in eng.last_timing_by_kernel().items()}
        got = eng.caf(x, grid)
        fbase = eng.caf(iq, grid, fine=True)
        fgot = eng.caf(x, grid, fine=True)
    if N == 4096:
        assert launches == {"k_fwd": 2, "k_win|k_pair": 1, "k_caf_select": 1}, launches       # all hypotheses in one launch
    assert np.array_equal(base[0], k[:, pairs[:, 1]] - k[:, pairs[:, 0]] + 2), "the scene's hypotheses are not found"
    assert np.array_equal(got[0], base[0]), "dop_idx moves with the level"
    _assert_rule(got[1:], base[1:], e, pairs, "caf %s" % what)
    assert np.array_equal(fgot[0], fbase[0])
    assert np.array_equal(_bits(fgot[1]), _bits(fbase[1])), "dop_frac moves with the level: %d of %d" % (
        int((_bits(fgot[1]) != _bits(fbase[1])).sum()), fgot[1].size)
    _assert_rule(fgot[2:], fbase[2:], e, pairs, "caf %s, fine" % what)


# ---- e. detection ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-7, 8])
def test_detect_on_a_scaled_batch(xc, k):
    """detect() on 2^k x (N = 1024, W = 6, complex64) with threshold_db moved by 20 log10(2^k): every local maximum against the
    float64 detector reference with the margin rule of tests/test_detect_exact.py, and the thresholded call's bins and
    count equal to the unscaled call's wherever neither that rule nor the float32 rounding of the dB values at the
    threshold gives an excuse (dB is a logarithm: the level is an offset, exact only up to float32 rounding; the 1e-12
    inside the logarithm is 2^-40 of these magnitudes)."""
    import test_detect_exact as te
    N, W, thr = 1024, 6, 60.0
    x0, _ = te.make_windows(W, N, seed=1700)
    x = D.scaled(x0[:, None, :], np.full((W, 1), k))[:, 0, :]
    shift = float(np.float32(20.0 * np.log10(2.0 ** k)))
    with xc.XcorrEngine(2, 4096, 1) as eng:
        A = eng.detect(x, threshold_db=-np.inf, distance=1, dc_exclude_bins=0.0, min_confidence=0.0, max_peaks=N // 2)
        cut0 = eng.detect(x0, threshold_db=thr, distance=1, max_peaks=N // 2)
        cut = eng.detect(x, threshold_db=float(np.float32(thr + shift)), distance=1, max_peaks=N // 2)
    for w in range(W):
        ab, ap, _, _, af = A[w]
        p_o, p64, tol = te._fft_tolerance_db(x[w])
        want = te._local_maxima_1d(p_o.astype(np.float64))[0]
        for b in np.setxor1d(ab, want):
            assert te._margin_ok(int(b), p64, tol), (k, w, int(b))
        common, ia, _ = np.intersect1d(ab, want, return_indices=True)
        dev = np.abs(ap[ia] - p_o[common].astype(np.float64))
        assert np.all((dev < 2e-4) | (dev <= tol[common])), (k, w, dev.max())
        rf, f64 = float(np.median(p_o)), float(np.median(p64))
        assert abs(af - rf) < 2e-4 or abs(af - rf) <= 4.0 * abs(rf - f64) + 1e-5, (k, w, af, rf, f64)
        # the thresholded calls (distance 1: every local maximum above the cuts): the same bins unless a candidate lies
        # within the tolerance of the threshold or of the confidence cut (snr = 20 min_confidence = 6 dB above the floor),
        # or is a local maximum by less than the two transforms agree on
        b0, p0, s0 = cut0[w][:3]
        b1, p1, s1 = cut[w][:3]
        edge = np.abs(p64 - (thr + shift)) <= tol + 2e-4
        edge |= np.abs(p64 - f64 - 6.0) <= tol + 4e-4
        print("k = %d window %d: %d / %d peaks, %d bins within the tolerance of a cut" % (k, w, len(b0), len(b1), int(edge.sum())))
        assert len(b0) > 0
        for b in np.setxor1d(b0, b1):
            assert edge[b] or te._margin_ok(int(b), p64, tol), (k, w, int(b))
        _, i0, i1 = np.intersect1d(b0, b1, return_indices=True)
        assert np.all(np.abs(p1[i1] - np.float32(shift) - p0[i0]) <= 4e-4) and np.all(np.abs(s1[i1] - s0[i0]) <= 8e-4), (k, w)
