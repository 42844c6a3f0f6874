"""Every route finds the peak wherever it lies in +-(N - 1), and gets lag_frac and peak right there.

The seeded generator keeps the winning lag inside the central +-800 of the range (tests/far_lag_ref.py), so a kernel that
dropped the lags of a far wave, fetched a parabola tap across a seam from the wrong place, or lost the winner in its last
cross-wave reduction passed every unbounded parity test.  Here each route -- steered as the other tests steer it, the
launched kernel families asserted -- runs

  * the impulse scene: every target lag, the seams of the route and the four lags at the two ends of the range as the
    single non-zero sample of a correlation; the reference is analytic (lag exact, peak |A C|, |lag_frac| <= 1e-5);
  * the two-buoy noise scene: one 10 dB window per target lag, true lag = target + u, |u| < 0.5, against ref64;
  * the multi-buoy noise scene where the route takes three buoys or more: every pair's lag anywhere in +-7/8 N;
  * complex64 and raw uint8 input of the noise scenes, bit-identical;
  * the default pair list, and a custom list holding each designed pair and its mirror (j, i): both signs of every lag.

Bars, against the float64 reference (or the analytic values): lag_int equal on every slot (every margin is >= 1e-3,
tests/test_far_lag_ref_cpu.py: no near-tie excuse); |lag_frac - ref| <= 1e-5 ABSOLUTE -- not scaled by |lag|: the header's
scaled bar allows 0.16 samples at lag 16000 -- or within four times what one float32 ulp on each of the oracle's taps moves
the parabola's vertex (the flat-peak bound of test_flat_peak_rule_on_short_noisy_windows); peak within 1e-5 relative.  The
float32 oracle holds 3e-7 on lag_frac on these inputs (test_far_lag_ref_cpu.py).

Seams per route (circular index m = lag mod 2N; a seam at every multiple of the stride, and the lag below it):
  k_win, k_fwd + k_pair     m mod 4096 = n: thread 2 (n mod 256) + half, register n / 256 -- wave every 32, register every 256,
                            the two lanes of a pair at -1 / 0; taps of lanes 0, 1, 62, 63 come from the halo rows
  k_win8kl                  the same network per bin-parity half: + halves at +-4096
  k16_fwd + k16_pairs       the same per residue quarter: + quarters at +-4096, +-8192, +-12288, two search phases per wave
  g_pair_small, g_win_fused, g_win_scr, g_win_scr14, the 1024-thread build, g_win_eo15
                            thread tid holds m = tid + e x threads: wave every 64, register every `threads` (L / 16 ... 1024),
                            taps by circular index out of LDS: the wrap 2N - 1 / 0 at lags -1 / 0; g_win_eo15's halves at +-8192
  four-step (g_final behind g_rows_fused / g_rows_inv / g_rows_anchor)
                            m = row x L2 + column, tiles of 8 ... 32 columns: tile seams every 8 / 16 / 32 lags (tap from the
                            neighbouring tile's halo), row seams every L2 = 1024 (N = 65536) ... 4096 lags (tap from the last
                            tile of the previous row), the wrap at -1 / 0
far_lag_ref.STRIDES lists these strides per length; target_lags puts a lag on the first, a middle, the last and a seeded
multiple of each, with both neighbours, on both sides of zero.

Exhaustive: N = 256 on its three routes and N = 4096 through k_win (1171 windows of 8 buoys, the fused route by itself)
make EVERY lag of +-(N - 1) the winning lag of an impulse slot."""
import numpy as np
import pytest

import caf_ref as cr
import far_lag_ref as F
import integrated_ref as ir
import quality_ref as qr
import radio_mapper_amd as rm
import refined_ref as rr
import weighted_ref as wr
from oracle import xcorr_ref as orc

pytestmark = pytest.mark.gpu

ABS = 1e-5


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


FOUR = {"g_cols_fwd", "g_cols_inv", "g_final"}
PER = {"k_fwd", "k_win|k_pair"}
SMALL = {"g_fwd_small", "g_pair_small"}
WIN = {"g_win_*"}
K16 = {"k16_fwd", "k16_pairs"}
TWO_PASS = FOUR | {"g_rows_fwd", "g_rows_inv"}
ANCHOR = FOUR | {"g_rows_fwd", "g_rows_anchor"}
RFUSED = FOUR | {"g_rows_fused"}

# (id, N, buoys, default options, engine options, families with the default list, families with a custom list, exhaustive)
ROUTES = [
    ("4096-k_win", 4096, 8, {"small4096": 0}, {}, {"k_win|k_pair"}, PER, False),
    ("4096-k_fwd+k_pair", 4096, 8, {}, {}, PER, PER, False),
    ("4096-k_fwd+k_pair-fused0", 4096, 2, {}, {"fused": 0}, PER, PER, False),
    ("4096-g_small", 4096, 8, {"generic4096": 1}, {}, SMALL, SMALL, False),
    ("256-g_win_fused", 256, 4, {}, {}, WIN, WIN, True),
    ("256-g_win_scr", 256, 5, {"wscr": 2}, {}, WIN, WIN, True),
    ("256-g_small", 256, 4, {"wfused": 0, "wscr": 0}, {}, SMALL, SMALL, True),
    ("1024-g_win_fused", 1024, 4, {}, {}, WIN, WIN, False),
    ("1024-g_win_scr", 1024, 5, {"wscr": 2}, {}, WIN, WIN, False),
    ("1024-g_small", 1024, 4, {"wfused": 0, "wscr": 0}, {}, SMALL, SMALL, False),
    ("2048-g_win_fused", 2048, 4, {}, {}, WIN, WIN, False),
    ("2048-g_win_scr", 2048, 5, {"wscr": 2}, {}, WIN, WIN, False),
    ("2048-g_small", 2048, 4, {"wfused": 0, "wscr": 0}, {}, SMALL, SMALL, False),
    ("8192-k_win8kl", 8192, 8, {"wscr": 2}, {}, WIN, WIN, False),
    ("8192-g_win_scr14", 8192, 8, {"wscr": 2, "kwin8k": 0}, {}, WIN, WIN, False),
    ("8192-g_win_scr-1024thr", 8192, 8, {"wscr": 2, "kwin8k": 0, "wscr14": 0}, {}, WIN, WIN, False),
    ("8192-four-step", 8192, 8, {}, {}, ANCHOR, TWO_PASS, False),
    ("16384-k16", 16384, 5, {"kwin16k": 2}, {}, K16, K16, False),
    ("16384-g_win_eo15", 16384, 5, {"kwin16k": 0, "wscr": 2}, {}, WIN, WIN, False),
    ("16384-four-step", 16384, 5, {"kwin16k": 0}, {}, TWO_PASS, TWO_PASS, False),
    ("65536-g_rows_fused", 65536, 3, {"fused": 2}, {}, RFUSED, RFUSED, False),
    ("65536-g_rows_fwd+inv", 65536, 3, {"fused": 0}, {}, TWO_PASS, TWO_PASS, False),
    ("65536-g_rows_anchor", 65536, 8, {}, {}, ANCHOR, TWO_PASS, False),
    ("1048576-four-step", 1 << 20, 2, {}, {}, RFUSED, RFUSED, False),
]


def _assert_bars(got, ref, xs, what):
    """got = (lag_int, lag_frac, peak) against ref = (lag_int, lag_frac, peak) of the same shape; xs(flat index) -> the two
    windows of that slot (for the flat-peak bound, computed only where the absolute bar is missed).  Prints the worst
    figures first."""
    li, lf, pk = (np.asarray(a) for a in got)
    ri, rf, rp = (np.asarray(a) for a in ref)
    assert li.shape == ri.shape, (what, li.shape, ri.shape)
    bad = li != ri
    d = np.abs(lf.astype(np.float64) - rf)
    dp = np.abs(pk.astype(np.float64) - rp) / rp
    print("%s: %d slots, %d integer lags differ, worst |dfrac| %.2e, worst |dpeak| / peak %.2e, |lag| up to %d"
          % (what, li.size, int(bad.sum()), float(d[~bad].max(initial=0.0)), float(dp[~bad].max(initial=0.0)), int(np.abs(ri).max())))
    assert not bad.any(), "%s: %d integer lags differ, e.g. got %s for %s" % (what, int(bad.sum()), li[bad][:8], ri[bad][:8])
    for k in np.flatnonzero(d.ravel() > ABS):
        x_i, x_j = xs(int(k))
        lag = float(ri.ravel()[k] + rf.ravel()[k])
        bound = 4.0 * orc.parabola_ulp_bound(x_i, x_j) * max(abs(lag), 1.0)
        assert d.ravel()[k] <= bound, "%s: lag_frac %.7f for %.7f at lag %d (four one-ulp bounds: %.2e)" % (
            what, lf.ravel()[k], rf.ravel()[k], ri.ravel()[k], bound)
    assert np.all(dp <= 1e-5), "%s: peak off by %.2e relative" % (what, float(dp.max()))


def _run(eng, iq, pairs, fam, what):
    got = eng.correlate(iq, pairs)
    launched = set(eng.last_timing_by_kernel())
    assert launched == fam, (what, launched, fam)
    return got


def _windows_of(iq, pairs):
    """flat slot index k = window x P + pair -> the pair's two windows (for _assert_bars)"""
    P = len(pairs)
    return lambda k: (iq[k // P, pairs[k % P, 0]], iq[k // P, pairs[k % P, 1]])


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("name,N,B,dflt,eopts,fam,fam_custom,exhaustive", ROUTES, ids=[r[0] for r in ROUTES])
def test_route_finds_the_peak_anywhere(xc, opts, name, N, B, dflt, eopts, fam, fam_custom, exhaustive):
    """one route: impulse, two-buoy and multi-buoy scenes, default and mirrored custom pair lists, complex64 and uint8 (module
    docstring; the seams of the route are listed there)"""
    for k, v in dflt.items():
        opts(k, v)
    dlist = orc.pair_list(B)
    both = F.mirrored(dlist)                                   # every pair of the default list followed by its mirror
    imp_iq, pos, amp = F.impulse_scene(N, F.impulse_lags(N), B, 11)
    two = F.two_buoy(N)
    t_iq, src = F.pack(two["iq"], B)
    t_raw, _ = F.pack(two["raw"], B)
    des, cols = F.designed_pairs(B)
    multi = F.multi_buoy(N, B) if B >= 3 else None
    W = max(len(imp_iq), len(t_iq), len(multi["iq"]) if multi else 0)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        for k, v in eopts.items():
            eng.set_option(k, v)
        # -- impulses: every ordered pair is analytic
        ai, ap = F.impulse_ref(pos, amp, both)
        got = _run(eng, imp_iq, None, fam, name + " impulses")
        _assert_bars(got, (ai[:, ::2], np.zeros(ai[:, ::2].shape), ap[:, ::2]), _windows_of(imp_iq, dlist), name + " impulses, default list")
        got = _run(eng, imp_iq, both, fam_custom, name + " impulses, mirrored list")
        _assert_bars(got, (ai, np.zeros(ai.shape), ap), _windows_of(imp_iq, both), name + " impulses, mirrored list")
        found = set(got[0].ravel().tolist())
        assert set(F.impulse_lags(N).tolist()) <= found
        # -- two-buoy noise windows, packed into windows of B buoys: designed pairs (2 g, 2 g + 1)
        ref = tuple(a[src] for a in two["ref"][:3])
        rev = tuple(a[src] for a in two["rev"][:3])
        G = src.shape[1]
        xs2 = lambda k: (two["iq"][src.ravel()[k], 0], two["iq"][src.ravel()[k], 1])   # noqa: E731
        got = _run(eng, t_iq, None, fam, name + " two-buoy")
        assert _same(got, eng.correlate(t_raw)), "uint8 input differs from complex64"
        _assert_bars(tuple(a[:, cols] for a in got), ref, xs2, name + " two-buoy noise, default list")
        mir = F.mirrored(des)
        got = _run(eng, t_iq, mir, fam_custom, name + " two-buoy, mirrored list")
        assert _same(got, eng.correlate(t_raw, mir)), "uint8 input differs from complex64 (custom list)"
        _assert_bars(tuple(a[:, 0::2] for a in got), ref, xs2, name + " two-buoy noise, designed pairs of the custom list")
        _assert_bars(tuple(a[:, 1::2] for a in got), rev, lambda k: xs2(k)[::-1], name + " two-buoy noise, mirror pairs")
        assert G == len(des)
        # -- multi-buoy noise windows: every pair's lag somewhere in +-7/8 N
        if multi is not None:
            m_iq, mref = multi["iq"], multi["ref"]
            got = _run(eng, m_iq, None, fam, name + " multi-buoy")
            assert _same(got, eng.correlate(multi["raw"]))
            _assert_bars(got, tuple(a[:, ::2] for a in mref[:3]), _windows_of(m_iq, dlist), name + " multi-buoy noise, default list")
            got = _run(eng, m_iq, both, fam_custom, name + " multi-buoy, mirrored list")
            assert _same(got, eng.correlate(multi["raw"], both))
            _assert_bars(got, mref[:3], _windows_of(m_iq, both), name + " multi-buoy noise, mirrored list")
        # -- every lag of +-(N - 1) as the winning lag of an impulse slot
        if exhaustive:
            e_iq, e_pos, e_amp = F.impulse_scene(N, np.arange(-(N - 1), N), B, 13)
            ei, ep = F.impulse_ref(e_pos, e_amp, both)
            with xc.XcorrEngine(B, N, len(e_iq)) as big:
                big.set_option("timing", 1)
                got = _run(big, e_iq, both, fam_custom, name + " every lag")
                _assert_bars(got, (ei, np.zeros(ei.shape), ep), _windows_of(e_iq, both), name + " every lag, mirrored list")
                gd = _run(big, e_iq, None, fam, name + " every lag, default list")
            _assert_bars(gd, (ei[:, ::2], np.zeros(ei[:, ::2].shape), ep[:, ::2]), _windows_of(e_iq, dlist), name + " every lag, default list")
            won = set(gd[0][:, :B - 1].ravel().tolist())
            assert won == set(range(-(N - 1), N)), "%d lags of +-(N - 1) never won" % (2 * N - 1 - len(won))
            print("%s: every lag of +-%d found (%d windows)" % (name, N - 1, len(e_iq)))


def test_every_lag_of_n4096_through_k_win(xc, opts):
    """8191 lags, seven designed pairs (0, b) per window of 8 buoys: 1171 windows (307 MB), which take the fused kernel
    by themselves; all 28 pairs of every window are analytic.  Every lag of +-4095 must be the winning lag of its slot."""
    N, B = 4096, 8
    iq, pos, amp = F.impulse_scene(N, np.arange(-(N - 1), N), B, 17)
    dlist = orc.pair_list(B)
    ai, ap = F.impulse_ref(pos, amp, dlist)
    assert len(iq) == 1171
    with xc.XcorrEngine(B, N, len(iq)) as eng:
        eng.set_option("timing", 1)
        got = _run(eng, iq, None, {"k_win|k_pair"}, "N = 4096 every lag")
    _assert_bars(got, (ai, np.zeros(ai.shape), ap), _windows_of(iq, dlist), "k_win, every lag of +-4095")
    won = set(got[0][:, :B - 1].ravel().tolist())
    assert won == set(range(-(N - 1), N)), "%d lags of +-4095 never won" % (2 * N - 1 - len(won))
    print("k_win: every lag of +-4095 found (%d windows)" % len(iq))


# ---- the feature kernels at far lags: one case per stored-spectrum layout ---------------------------------------------------
# (they read the spectra the per-transform forward kernels stored: k_fwd, g_fwd_small, the four-step rows)
LAYOUTS = [("k_fwd", 4096), ("g_fwd_small", 1024), ("g_rows_fwd", 65536)]


@pytest.fixture(scope="module")
def feature_scenes():
    """per layout: the two-buoy noise windows of ten lags spread over +-noise_top (both ends included) and the three-buoy
    scene (four lags and two windows at N = 65536); built once"""
    out = {}
    for _, N in LAYOUTS:
        two = F.two_buoy(N)
        n, w = (10, 8) if N < 65536 else (4, 2)       # (a refined reference costs 0.4 s per pair-window at N = 65536)
        sub = np.unique(np.linspace(0, len(two["lags"]) - 1, n).astype(int))
        m = F.multi_buoy(N, 3)
        out[N] = [("two-buoy", two["iq"][sub], two["raw"][sub]), ("multi-buoy", m["iq"][:w], m["raw"][:w])]
    return out


def _feature_engine(xc, iq):
    W, B, N = iq.shape
    eng = xc.XcorrEngine(B, N, W)
    eng.set_option("timing", 1)
    return eng


@pytest.mark.parametrize("fwd,N", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_weighted_at_far_lags(xc, opts, feature_scenes, fwd, N):
    """band [-0.3, 0.3] + PHAT against weighted_ref, with the bars of tests/test_gpu_weighted.py"""
    import test_gpu_weighted as tw
    for what, iq, raw in feature_scenes[N]:
        with _feature_engine(xc, iq) as eng:
            got = eng.correlate(iq, band=(-0.3, 0.3), whiten=True)
            assert fwd in eng.last_timing_by_kernel()
            assert _same(got, eng.correlate(raw, band=(-0.3, 0.3), whiten=True))
        ref = wr.weighted_batch(iq, band=(-0.3, 0.3), phat=True, with_bound=True)
        print(what, "N =", N, "|lag| up to", int(np.abs(ref[0]).max()), "smallest margin %.2e" % float(ref[3].min()))
        assert np.abs(ref[0]).max() > F.noise_top(N) // 2
        tw._assert_parity(*got, ref)


@pytest.mark.parametrize("fwd,N", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_integrated_at_far_lags(xc, opts, fwd, N):
    """K = 2, both windows of a group with the same delays (their own source and noise), against integrated_ref with the
    bars of tests/test_gpu_integrated.py"""
    import test_gpu_integrated as ti
    lags = F.scene_lags(N)
    lags = lags[np.unique(np.linspace(0, len(lags) - 1, 8).astype(int))]
    iq2, raw2, _ = F.noise_scene(N, lags, F.SEED + 77, repeat=2)
    half = F.noise_top(N) / 2.0
    d = np.repeat(np.random.default_rng(N).uniform(-half, half, size=(3, 3)), 2, axis=0)
    iq3, _, raw3 = rm.synth.make_windows(6, 3, N, F.FS, F.SEED + 78, max_delay=(N - 2) / 2.0, delays=d, return_u8=True)
    for what, iq, raw in (("two-buoy", iq2, raw2), ("multi-buoy", iq3, raw3)):
        with _feature_engine(xc, iq) as eng:
            got = eng.correlate(iq, integrate=2)
            assert fwd in eng.last_timing_by_kernel()
            assert _same(got, eng.correlate(raw, integrate=2))
        ref = ir.integrated_batch(iq, 2, with_bound=True)
        assert np.abs(ref[0]).max() > F.noise_top(N) // 2
        ti._assert_parity(*got, ref, "%s N = %d integrate = 2" % (what, N))


@pytest.mark.parametrize("U", [4, 16])
@pytest.mark.parametrize("fwd,N", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_refined_at_far_lags(xc, opts, feature_scenes, fwd, N, U):
    """refine = U against refined_ref with the bars of tests/test_gpu_refined.py"""
    import test_gpu_refined as tr
    for what, iq, raw in feature_scenes[N]:
        with _feature_engine(xc, iq) as eng:
            got = eng.correlate(iq, refine=U)
            tk = eng.last_timing_by_kernel()
            assert fwd in tk and "k_refine" in tk, tk
            assert _same(got, eng.correlate(raw, refine=U))
        ref = rr.refined_batch(iq, U)
        assert np.abs(ref[0]).max() > F.noise_top(N) // 2
        tr._assert_refined(got, ref, N, what="%s N = %d U = %d" % (what, N, U))


def test_refined_where_the_phase_index_wraps_32_bits(xc, opts):
    """N = 2^20, U = 2, two windows of two buoys, lags next to -+top (917 k): k_refine forms (k lag0) mod L in unsigned
    32-bit arithmetic, and k lag0 reaches 2^21 x 9e5 = 1.9e12 here -- it wraps 2^32 hundreds of times, which is exact only
    because L divides 2^32.  Against refined_ref (float64, the index reduced in Python integers)."""
    import test_gpu_refined as tr
    N = 1 << 20
    two = F.two_buoy(N)
    assert np.abs(two["lags"]).min() > 900000
    with xc.XcorrEngine(2, N, 2) as eng:
        eng.set_option("timing", 1)
        got = eng.correlate(two["iq"], refine=2)
        assert "k_refine" in eng.last_timing_by_kernel()
        rev = eng.correlate(two["iq"], np.array([(1, 0)], np.int32), refine=2)
    ref = rr.refined_batch(two["iq"], 2)
    assert np.all(np.abs(ref[0][:, 0] - two["lags"]) <= 1)
    tr._assert_refined(got, ref, N, what="N = 2^20 U = 2")
    tr._assert_refined(rev, rr.refined_batch(two["iq"], 2, pairs=[(1, 0)]), N, what="N = 2^20 U = 2, mirrored pair")


@pytest.mark.parametrize("fwd,N", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_quality_at_far_lags(xc, opts, feature_scenes, fwd, N):
    """the quality figures against quality_ref with the bars of tests/test_gpu_quality.py; the three lag outputs bit for bit
    those of the call without quality, and within this file's bars of ref64"""
    import test_gpu_quality as tq
    for what, iq, raw in feature_scenes[N]:
        with _feature_engine(xc, iq) as eng:
            got = eng.correlate(iq, quality=True)
            assert "k_quality" in eng.last_timing_by_kernel()
            plain = eng.correlate(iq)
        assert _same(got[:3], plain), "the lag outputs change with quality = True"
        tq._assert_quality(got[3], qr.quality_batch(iq), N, "%s N = %d" % (what, N))
        pl = orc.pair_list(iq.shape[1])
        ref = F.ref64_batch(iq, pl)
        _assert_bars(got[:3], ref[:3], _windows_of(iq, pl), "%s N = %d lag outputs of the quality call" % (what, N))


@pytest.mark.parametrize("fwd,N", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_doppler_search_at_far_lags(xc, opts, fwd, N):
    """rmx_caf_batch, five hypotheses 2 / N cycles per sample apart (a quarter turn over the N / 8 samples two windows at
    lag top still share: the hypotheses stay 1e-3 apart), every buoy's offset a whole multiple, so each pair's difference
    is a grid point: against caf_ref with the bars of tests/test_gpu_caf.py."""
    import test_gpu_caf as tc
    step = 2.0 / N
    grid = (np.arange(5) - 2) * step
    top = F.noise_top(N)
    lags = np.array([-(top - 1), -(N // 2) - 1, N // 4 + 1, top - 2])
    k2 = np.array([[0, 2], [2, 1], [1, 0], [2, 0]])
    iq2, raw2, _ = F.noise_scene(N, lags, F.SEED + 91, doppler_cps=k2 * step)
    k3 = np.array([[0, 1, 2], [2, 0, 1]])
    iq3, raw3, _ = F.multi_scene(N, 3, 2, F.SEED + 92, doppler_cps=k3 * step)
    for what, iq, raw, k in (("two-buoy", iq2, raw2, k2), ("multi-buoy", iq3, raw3, k3)):
        W, B, _ = iq.shape
        with xc.XcorrEngine(B, N, W) as eng:
            eng.set_option("timing", 1)
            got = eng.caf(iq, grid)
            assert "k_caf_select" in eng.last_timing_by_kernel()
            assert _same(got, eng.caf(raw, grid))
        ref = cr.reference(iq, grid)
        pl = orc.pair_list(B)
        assert np.array_equal(ref["dop"], k[:, pl[:, 1]] - k[:, pl[:, 0]] + 2), what
        print(what, "N =", N, "lags", ref["lag_int"].ravel())
        assert what != "two-buoy" or np.abs(ref["lag_int"]).max() >= top - 2
        tc._assert_parity(got, ref)
