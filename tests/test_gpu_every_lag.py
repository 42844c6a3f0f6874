"""Every lag of every bounded peak search: a one-lag interval [k, k] reads m[k] out of the correlation vector.

The sliced rule of include/rmx.h makes lag_bounds = [k, k] return lag_int = k, lag_frac = 0 and peak = m[k]: ONE element
of the 2N - 1, with both edges of lag_mask() (lag_bounds.hpp) decisive at that position.  The other bounded tests draw
random intervals some 2N / 3 lags long, where an off-by-one at an edge shows only if the wrongly kept or dropped lag
beats everything inside; here every lag (or, at the long lengths, every seam lag and 2048 seeded ones) is such an edge,
on each kernel that carries its own mask arithmetic, for a 10 dB emitter scene and a noise-only scene, against the
float64 vector of tests/full_vector_ref.py.  Which lag each output slot probes is full_vector_ref.lag_plan, whose
coverage tests/test_full_vector_cpu.py proves without a GPU.

Per slot: lag_int == k and lag_frac == 0 exactly; |peak - m64[k]| <= 1e-5 m64[k] + 1e-6 max(m64) -- the bar of a value
inside a vector (tests/test_gpu_lag_bounds.py: _assert_sliced; the weighted entry's parity statement in include/rmx.h);
uint8 input gives the same bytes.  The float32 oracle stays within 0.071 of that bar (test_full_vector_cpu.py).

Routes (steered as tests/test_gpu_far_lags.py steers them, the launched families asserted):
  k_win (bounded)                 N = 4096, 16 tiled buoys x 228 windows, default list, per-window bounds      exhaustive
  k_fwd + k_pair, resident / not  N = 4096, 2 windows, 16384 pairs alternating (0, 1) / (1, 0), shared bounds  exhaustive
  g_pair_small                    N = 16, 256, 2048, and 4096 with generic4096, the same                       exhaustive
  k_win8kl (wscr = 2)             N = 8192, 640 pairs (the kernel's LDS copy) x 27 windows                     exhaustive
  k16_fwd + k16_pairs             N = 16384, 640 pairs x 54 windows                                            exhaustive
  four-step behind g_rows_inv     N = 8192 exhaustive (512 pairs x 36 windows), N = 65536 sampled
  four-step behind g_rows_anchor  N = 8192, 6 tiled buoys x 168 windows, default list                          sampled
  four-step behind g_rows_fused   N = 65536, 4 tiled buoys, default list                                       sampled
A bounded call never runs g_win_fused, g_win_scr, g_win_scr14 or g_win_eo15 (host_plan.hpp: plan_route): they have no
bounded instantiation and are outside this probe.

Three further cases per stored-spectrum layout (k_fwd 4096, g_fwd_small 1024, g_rows_fwd 65536; sampled at the last):
integrate = 3 against the float64 root-sum-square, band [-0.3, 0.3] + PHAT through rmx_xcorr_batch_weighted, and the
Doppler search caf(lag_bounds = [k, k]) over five hypotheses 0.5 / N apart, whose dop_idx must be the float64 first
maximum over d of m_d[k] wherever the float64 gap between the two largest exceeds twice the bar of the larger; elsewhere
it must be one of those two (where more than two lie within that gap -- at lags +-(N - 1) one product is the whole sum
and every hypothesis has the same magnitude -- any of the tied ones), and at most 3 % of the slots may be such.

Measured on an MI355X (LABNOTES.md R14 has the table): worst |peak error| / bar over the bounded routes 0.032 on the
emitter scene and 0.146 on the noise scene (g_rows_fused at N = 65536); integrate = 3 0.045 / 0.077; band + PHAT 0.068 /
0.612 (noise at N = 65536); the Doppler search 0.101 / 0.106, its excused share 0.21 ... 0.82 % against the cap of 3 %,
dop_frac bit for bit the parabola over the engine's own per-hypothesis peaks.  The largest scratch is 579 MB."""
import numpy as np
import pytest

import caf_ref as cr
import caf_request_ref as rr
import full_vector_ref as V

pytestmark = pytest.mark.gpu


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
TWO_PASS = FOUR | {"g_rows_fwd", "g_rows_inv"}
NO_WIN = {"wfused": 0, "wscr": 0}

# (id, N, buoys, windows, custom list (pairs, every n-th the mirror) or None, bounds per window, default options, engine
# options, launched families, exhaustive, calls the windows are split over: the four-step product buffer grows with
# windows x pairs x L, the input with windows x buoys x N)
ROUTES = [
    ("4096-k_win", 4096, 16, 228, None, True, {"small4096": 0}, {}, {"k_win|k_pair"}, True, 1),
    ("4096-k_fwd+k_pair-resident", 4096, 2, 2, (16384, 2), False, {}, {"resident": 1}, PER, True, 1),
    ("4096-k_fwd+k_pair-streaming", 4096, 2, 2, (16384, 2), False, {}, {"resident": 0}, PER, True, 1),
    ("16-g_small", 16, 2, 2, (64, 2), False, NO_WIN, {}, SMALL, True, 1),
    ("256-g_small", 256, 2, 2, (1024, 2), False, NO_WIN, {}, SMALL, True, 1),
    ("2048-g_small", 2048, 2, 2, (8192, 2), False, NO_WIN, {}, SMALL, True, 1),
    ("4096-g_small", 4096, 2, 2, (16384, 2), False, {"generic4096": 1}, {}, SMALL, True, 1),
    ("8192-k_win8kl", 8192, 2, 27, (640, 32), True, {"wscr": 2}, {}, {"g_win_*"}, True, 1),
    ("16384-k16", 16384, 2, 54, (640, 32), True, {"kwin16k": 2}, {}, {"k16_fwd", "k16_pairs"}, True, 1),
    ("8192-g_rows_inv", 8192, 2, 36, (512, 16), True, {"fused": 0, "wscr": 0, "gen_chunk": 8}, {}, TWO_PASS, True, 1),
    ("65536-g_rows_inv", 65536, 2, 22, (128, 4), True, {"fused": 0, "gen_chunk": 4}, {}, TWO_PASS, False, 1),
    ("8192-g_rows_anchor", 8192, 6, 168, None, True, {"wscr": 0, "gen_chunk": 64}, {}, FOUR | {"g_rows_fwd", "g_rows_anchor"}, False, 1),
    ("65536-g_rows_fused", 65536, 4, 440, None, True, {"fused": 2, "gen_chunk": 32}, {}, FOUR | {"g_rows_fused"}, False, 4),
]


def plan_of(N, B, W, custom, per_window, exhaustive):
    """(pair list, pairs argument of the call, lags [W][P] or [1][P]) of a route"""
    pl = V.pair_list(*custom) if custom else np.array([(i, j) for i in range(B) for j in range(i + 1, B)], np.int32)
    kinds = V.kinds_of(pl, W if per_window else 1)
    return pl, (pl if custom else None), V.lag_plan(N, kinds, exhaustive).reshape(-1, len(pl)), kinds


def _bounds(lags, per_window):
    lb = np.stack([lags, lags], axis=-1).astype(np.int32)
    return lb if per_window else lb[0]


def _hold(name, got, lags, ref, vmax):
    """the per-slot assertions; returns the worst |peak error| / bar"""
    li, lf, pk = got
    lags = np.broadcast_to(lags, li.shape)
    assert np.array_equal(li, lags), "%s: %d slots returned another lag, e.g. %s for %s" % (
        name, int((li != lags).sum()), li[li != lags][:6], lags[li != lags][:6])
    assert not np.any(lf), "%s: lag_frac != 0 on %d one-lag intervals" % (name, int(np.count_nonzero(lf)))
    ratio = np.abs(pk.astype(np.float64) - ref) / V.bar(ref, vmax)
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print("%s: %d slots, worst |peak - m64[k]| / bar %.3f (lag %d, slot %s, m64 %.6g, got %.6g)" % (
        name, li.size, float(ratio.max()), int(lags[worst]), worst, float(ref[worst]), float(pk[worst])))
    assert ratio.max() <= 1.0, "%s: %d peaks outside the bar, worst %.2f of it at lag %d" % (
        name, int((ratio > 1).sum()), float(ratio.max()), int(lags[worst]))
    return float(ratio.max())


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("name,N,B,W,custom,per_window,dflt,eopts,fam,exhaustive,calls", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_lag_of_the_bounded_search(xc, opts, name, N, B, W, custom, per_window, dflt, eopts, fam, exhaustive, calls):
    """one route of the table in the module docstring, both scenes, complex64 and uint8"""
    for k, v in dflt.items():
        opts(k, v)
    pl, pairs, lags, kinds = plan_of(N, B, W, custom, per_window, exhaustive)
    probed = set(lags.ravel()[kinds == V.ORDER01].tolist())
    if exhaustive:
        assert probed == set(range(-(N - 1), N)), "%d lags of +-(N - 1) are not probed" % (2 * N - 1 - len(probed))
    else:
        assert set(V.sampled_lags(N).tolist()) <= probed and set(V.seeded_lags(N).tolist()) <= set(lags.ravel().tolist())
    assert set((V.mirror_lags(N) if exhaustive else V.sampled_lags(N)).tolist()) <= set(lags.ravel()[kinds == V.MIRROR10].tolist())
    lb = _bounds(lags, per_window)
    Wc = W // calls                                     # (even: every call sees the same tiled windows)
    assert Wc * calls == W and (Wc % 2 == 0 or calls == 1) and (per_window or calls == 1)
    with xc.XcorrEngine(B, N, Wc) as eng:
        eng.set_option("timing", 1)
        for k, v in eopts.items():
            eng.set_option(k, v)
        for scene in V.SCENES:
            iq, raw = (V.tile(a, Wc, B) for a in V.scenes(N)[scene])
            parts, parts8 = [], []
            for w0 in range(0, W, Wc):
                lbc = lb[w0:w0 + Wc] if per_window else lb
                parts.append(eng.correlate(iq, pairs, lag_bounds=lbc))
                launched = set(eng.last_timing_by_kernel())
                assert launched == fam, (name, scene, launched, fam)
                parts8.append(eng.correlate(raw, pairs, lag_bounds=lbc))
            got = tuple(np.concatenate(a) for a in zip(*parts))
            ref, vmax = V.slot_reference(V.vectors(N, scene), lags, pl, W)
            _hold("%s %s" % (name, scene), got, lags, ref, vmax)
            assert _same(got, tuple(np.concatenate(a) for a in zip(*parts8))), "uint8 input differs from complex64"
        print("%s: families %s, %d lags probed under (0, 1), scratch %d bytes" % (name, sorted(launched), len(probed), eng.scratch_bytes()))
        assert eng.scratch_bytes() <= 1 << 30


# ---- the feature kernels: one case per stored-spectrum layout ---------------------------------------------------------
# (forward family, N, windows or groups, custom list, bounds per window, default options, exhaustive)
LAYOUTS = [
    ("k_fwd", 4096, 2, (16384, 2), False, {}, True),
    ("g_fwd_small", 1024, 2, (4096, 2), False, {}, True),
    ("g_rows_fwd", 65536, 22, (128, 4), True, {"gen_chunk": 3}, False),
]
LAYOUT_IDS = [l[0] for l in LAYOUTS]


@pytest.mark.parametrize("fwd,N,G,custom,per_window,dflt,exhaustive", LAYOUTS, ids=LAYOUT_IDS)
def test_every_lag_of_the_integrated_sum(xc, opts, fwd, N, G, custom, per_window, dflt, exhaustive):
    """integrate = 3 over tiled windows: group g holds the distinct windows (g, g + 1, g) mod 2; m = the float64
    root-sum-square of their vectors"""
    for k, v in dflt.items():
        opts(k, v)
    K = 3
    pl, pairs, lags, kinds = plan_of(N, 2, G, custom, per_window, exhaustive)
    if exhaustive:
        assert set(lags.ravel()[kinds == V.ORDER01].tolist()) == set(range(-(N - 1), N))
    lb = _bounds(lags, per_window)
    with xc.XcorrEngine(2, N, K * G) as eng:
        eng.set_option("timing", 1)
        for scene in V.SCENES:
            iq, raw = (V.tile(a, K * G, 2) for a in V.scenes(N)[scene])
            got = eng.correlate(iq, pairs, lag_bounds=lb, integrate=K)
            launched = set(eng.last_timing_by_kernel())
            assert fwd in launched, launched
            assert _same(got, eng.correlate(raw, pairs, lag_bounds=lb, integrate=K)), "uint8 input differs from complex64"
            m = V.vectors(N, scene)
            # group parity p: windows p, 1 - p, p (K = 3 consecutive windows of the tiling, starting at window 3 g)
            mi = np.sqrt(np.stack([2.0 * m[p] ** 2 + m[1 - p] ** 2 for p in range(2)]))
            ref, vmax = V.slot_reference(mi, lags, pl, G)
            _hold("integrate = 3 %s N = %d %s" % (fwd, N, scene), got, lags, ref, vmax)
        print("integrate = 3 %s: families %s, scratch %d bytes" % (fwd, sorted(launched), eng.scratch_bytes()))


BAND = (-0.3, 0.3)


@pytest.mark.parametrize("fwd,N,W,custom,per_window,dflt,exhaustive", LAYOUTS, ids=LAYOUT_IDS)
def test_every_lag_of_the_weighted_correlation(xc, opts, fwd, N, W, custom, per_window, dflt, exhaustive):
    """band [-0.3, 0.3] + PHAT through rmx_xcorr_batch_weighted, against the weighted float64 vector"""
    for k, v in dflt.items():
        opts(k, v)
    pl, pairs, lags, kinds = plan_of(N, 2, W, custom, per_window, exhaustive)
    if exhaustive:
        assert set(lags.ravel()[kinds == V.ORDER01].tolist()) == set(range(-(N - 1), N))
    lb = _bounds(lags, per_window)
    with xc.XcorrEngine(2, N, W) as eng:
        eng.set_option("timing", 1)
        for scene in V.SCENES:
            iq, raw = (V.tile(a, W, 2) for a in V.scenes(N)[scene])
            got = eng.correlate(iq, pairs, lag_bounds=lb, band=BAND, whiten=True)
            launched = set(eng.last_timing_by_kernel())
            assert fwd in launched, launched
            assert _same(got, eng.correlate(raw, pairs, lag_bounds=lb, band=BAND, whiten=True)), "uint8 input differs from complex64"
            ref, vmax = V.slot_reference(V.vectors(N, scene, BAND, True), lags, pl, W)
            _hold("band + PHAT %s N = %d %s" % (fwd, N, scene), got, lags, ref, vmax)
        print("band + PHAT %s: families %s, scratch %d bytes" % (fwd, sorted(launched), eng.scratch_bytes()))


EXCUSED_SHARE = 0.03


@pytest.mark.parametrize("fwd,N,W,custom,per_window,dflt,exhaustive", LAYOUTS, ids=LAYOUT_IDS)
def test_every_lag_of_the_doppler_search(xc, opts, fwd, N, W, custom, per_window, dflt, exhaustive):
    """caf(lag_bounds = [k, k]) over five hypotheses 0.5 / N apart: the one-launch route (N = 4096), the small one and the
    four-step one.  m_d[k] in float64 per hypothesis; see the module docstring for the rule on dop_idx."""
    for k, v in dflt.items():
        opts(k, v)
    D = 5
    grid = (np.arange(D) - D // 2) * (0.5 / N)
    pl, pairs, lags, kinds = plan_of(N, 2, W, custom, per_window, exhaustive)
    if exhaustive:
        assert set(lags.ravel()[kinds == V.ORDER01].tolist()) == set(range(-(N - 1), N))
    lb = _bounds(lags, per_window)
    c = V.combo(pl)
    full = np.broadcast_to(lags, (W, len(pl)))
    tenth = np.random.default_rng(N + 5).random(full.shape) < 0.1
    with xc.XcorrEngine(2, N, W) as eng:
        eng.set_option("timing", 1)
        for scene in V.SCENES:
            iq2 = V.scenes(N)[scene][0]
            iq, raw = (V.tile(a, W, 2) for a in V.scenes(N)[scene])
            dop, dfrac, li, lf, pk = eng.caf(iq, grid, pairs, lag_bounds=lb, fine=True)
            launched = eng.last_timing_by_kernel()
            assert fwd in launched and "k_caf_select" in launched, launched
            if N == 4096:
                assert launched["k_win|k_pair"]["launches"] == 1, launched     # all hypotheses in one launch
            assert _same((dop, li, lf, pk), eng.caf(raw, grid, pairs, lag_bounds=lb)), "uint8 input differs from complex64"
            # m_d of the two distinct windows and the two orders, float64 [2][4][D][2N - 1] (the autocorrelations unused)
            md = np.zeros((2, 4, D, 2 * N - 1))
            for w in range(2):
                for cc in (1, 2):
                    for d in range(D):
                        md[w, cc, d] = V.derotated64(iq2[w, cc // 2], iq2[w, cc % 2], grid[d])
            wi = np.arange(W)[:, None] % 2
            vals = np.stack([md[wi, c[None, :], d, full + N - 1] for d in range(D)], axis=-1)         # [W][P][D]
            vmax = np.stack([md[:, :, d].max(axis=-1)[wi, c[None, :]] for d in range(D)], axis=-1)    # [W][P][D]
            bars = V.bar(vals, vmax)
            order = np.argsort(-vals, axis=-1, kind="stable")                                        # first maximum first
            d1, d2 = order[..., 0], order[..., 1]
            v1, v2 = cr.take(vals, d1), cr.take(vals, d2)
            decisive = (v1 - v2) > 2.0 * cr.take(bars, d1)
            what = "Doppler search %s N = %d %s" % (fwd, N, scene)
            assert np.array_equal(li, full) and not np.any(lf), what
            assert np.array_equal(dop[decisive], d1[decisive]), "%s: %d decisive slots chose another hypothesis" % (
                what, int((dop != d1)[decisive].sum()))
            # elsewhere: one of the two largest -- or, where more than two lie within that gap of the largest, any of those:
            # at lag +-(N - 1) ONE product x_j[n] conj(x_i[m]) is the whole sum and a rotation does not change its
            # magnitude (all five tie exactly), and over a short overlap N - |lag| the hypotheses hardly differ
            tied = (v1[..., None] - vals) <= 2.0 * cr.take(bars, d1)[..., None]
            assert np.all(cr.take(tied, dop)), "%s: %d slots chose a hypothesis below the float64 ties" % (what, int((~cr.take(tied, dop)).sum()))
            more = tied.sum(axis=-1) > 2
            assert np.all((dop == d1) | (dop == d2) | more), what
            print("%s: more than two hypotheses tie on %d slots, overlaps up to %d samples" % (
                what, int(more.sum()), int((N - np.abs(full[more])).max(initial=0))))
            err = np.abs(pk.astype(np.float64) - cr.take(vals, dop)) / cr.take(bars, dop)
            share = 1.0 - float(decisive.mean())
            print("%s: %d slots, worst |peak - m_d[k]| / bar %.3f, excused share %.4f" % (what, li.size, float(err.max()), share))
            assert err.max() <= 1.0, what
            assert share <= EXCUSED_SHARE, (what, share)
            # dop_frac on a seeded tenth: the parabola of caf_request_ref over the engine's own per-hypothesis peaks
            per = np.stack([eng.caf(iq, grid[d:d + 1], pairs, lag_bounds=lb)[3] for d in range(D)], axis=-1)   # [W][P][D]
            assert np.array_equal(cr.take(per, dop)[tenth], pk[tenth]), what
            want = rr.dop_parabola(per[tenth][None], dop[tenth][None])[0]
            bound = rr.dop_frac_bound(per[tenth][None], dop[tenth][None])[0]
            derr = np.abs(dfrac[tenth].astype(np.float64) - want.astype(np.float64))
            print("%s: dop_frac on %d slots, worst error %.3e" % (what, int(tenth.sum()), float(derr.max(initial=0.0))))
            assert np.all((derr <= 1e-5) | (derr <= bound)), (what, float(derr.max()))
        print("Doppler search %s: families %s, scratch %d bytes" % (fwd, sorted(launched), eng.scratch_bytes()))
