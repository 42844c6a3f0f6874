"""Every bin of every band consumer: a one-bin band [s / L, s / L] reads |X_j[s]| |X_i[s]| / L out of the cross-spectrum.

Each consumer of a band carries its own map from stored position to natural bin: the weighted forward epilogues of
k_fwd, g_fwd_small and the forward g_rows (xweight_apply with RMX_XBIN_KFWD, xbin_small, xbin_rows), the product-on-load
BandSet of the banded pair kernels, and the banded k_quality, which skips every 16-byte load whose bins the band drops.
The other tests probe 11 bins per route, through the banded entry only; from N = 2^16 on a wrong edge bin of a wide band
moves the peak by less than the 1e-5 bar.  Here every bin (a structured sample at N = 8192 and 65536 through the weighted
entry and at N = 65536 through the banded one: full_vector_ref.bin_plan, proven on the CPU in test_full_vector_cpu.py) is
the ONLY bin a band keeps, on a two-buoy 10 dB emitter scene, against the complex128 spectra of tests/full_vector_ref.py.

A one-bin correlation has the same magnitude at every lag: lag_int and lag_frac have no defined value and are not compared.
  weighted entry (store side)   per-window bands [W][2] over tiled windows; peak within 1e-5 of the product + 1e-6 of the
                                largest product of any bin; with PHAT, 1 / L under the same bar
  banded entry (product side)   64 one-bin bands per window, per-window band sets, the six routes of
                                test_gpu_bands.SINGLE and the four-step rows at N = 65536
  correlate_bands(quality=True) coherence = 1, Et / p0^2 = L, n_eff = 1, rms_bw = |s| / L at that entry's 1e-4 (rms_bw at
                                s = 0: 1e-7 absolute): rms_bw is the bin's frequency read back through k_quality's own map
  bounded + banded              a one-bin band with lag_bounds = [k, k] on 64 seeded (s, k): the same peak, lag_int = k,
                                lag_frac = 0

Measured on an MI355X (LABNOTES.md R14): worst |peak - product| / bar 0.033 over every route of the three entries, with
and without PHAT; coherence and n_eff within 1.2e-7 of 1, Et / p0^2 within 8.4e-7 of L, rms_bw within 7.9e-8 of |s| / L."""
import numpy as np
import pytest

import full_vector_ref as V
import quality_ref as qr

pytestmark = pytest.mark.gpu
QTOL = 1e-4     # the quality entry's bar (include/rmx.h; tests/test_gpu_bands_quality.py)


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


ROWS_FWD = {"g_cols_fwd", "g_rows_fwd"}
# (id, N, default options, engine options, forward families, exhaustive, layout of the structure sweep, windows per call)
WEIGHTED = [
    ("k_fwd 4096", 4096, {}, {}, {"k_fwd"}, True, None, 2048),
    ("g_fwd_small 16", 16, {}, {}, {"g_fwd_small"}, True, None, 32),
    ("g_fwd_small 256", 256, {}, {}, {"g_fwd_small"}, True, None, 512),
    ("g_rows_fwd 256", 256, {"small_maxl": 256}, {}, ROWS_FWD, True, None, 512),
    ("g_rows_fwd 8192", 8192, {}, {}, ROWS_FWD, False, ("rows", V.default_l1(8192)), 1024),
    ("g_rows_fwd 65536", 65536, {"gen_chunk": 64}, {}, ROWS_FWD, False, ("rows", V.default_l1(65536)), 128),
]
# the six routes of test_gpu_bands.SINGLE, and the four-step rows at N = 65536
BANDED = [
    ("k_pair_res", 4096, {}, {}, {"k_fwd"}, True, None, 128),
    ("k_pair_str", 4096, {}, {"resident": 0}, {"k_fwd"}, True, None, 128),
    ("g_pair_small", 256, {}, {}, {"g_fwd_small"}, True, None, 8),
    ("g_pair_small generic4096", 4096, {"generic4096": 1}, {}, {"g_fwd_small"}, True, None, 128),
    ("four-step rows", 8192, {"gen_chunk": 32}, {}, ROWS_FWD, True, None, 256),
    ("four-step rows N=256", 256, {"small_maxl": 256}, {}, ROWS_FWD, True, None, 8),
    ("four-step rows N=65536", 65536, {"gen_chunk": 8}, {}, ROWS_FWD, False, ("rows", V.default_l1(65536)), 16),
]
# the routes of test_gpu_bands_quality.ROUTES that differ in layout
QUALITY = [
    ("kRefKfwd", 4096, {}, {}, {"k_fwd"}, True, None, 128),
    ("kRefSmall", 256, {}, {}, {"g_fwd_small"}, True, None, 8),
    ("kRefRows N=256", 256, {"small_maxl": 256}, {}, ROWS_FWD, True, None, 8),
    ("kRefRows N=8192", 8192, {"gen_chunk": 32}, {}, ROWS_FWD, True, None, 256),
]
M = 64   # bands per window of the banded entries (the entry's limit)


def bin_rows():
    """(id, N, exhaustive, layout) of every sweep of this file (tests/test_full_vector_cpu.py checks the budgets)"""
    return [(kind + " " + r[0], r[1], r[5], r[6]) for kind, rows in (("weighted", WEIGHTED), ("banded", BANDED), ("quality", QUALITY))
            for r in rows]


def _scene(N):
    """(iq [2][2][N], the float64 products [2][L] of the two distinct windows over the natural bins, their largest)"""
    iq = V.scenes(N)["emitter"][0]
    X = V.spectra64(iq)                                      # [2][2][L]
    prod = np.abs(X[:, 1]) * np.abs(X[:, 0]) / (2 * N)
    assert np.all(np.abs(X) > 0)                             # (PHAT: every bin of both buoys is non-zero in float64)
    return iq, prod, prod.max(axis=-1)


def _padded(bins, multiple):
    """the bins, the last one repeated up to a multiple of `multiple` (whole calls of tiled windows)"""
    n = -(-len(bins) // multiple) * multiple
    return np.concatenate([bins, np.full(n - len(bins), bins[-1], bins.dtype)])


def _hold_peaks(what, pk, want, vmax):
    ratio = np.abs(pk.astype(np.float64) - want) / V.bar(want, vmax)
    k = int(np.argmax(ratio))
    print("%s: %d bins, worst |peak - product| / bar %.3f (got %.6g for %.6g)" % (what, ratio.size, float(ratio.max()), float(pk.ravel()[k]),
                                                                                float(np.ravel(want)[k])))
    assert ratio.max() <= 1.0, "%s: %d peaks outside the bar, worst %.2f of it" % (what, int((ratio > 1).sum()), float(ratio.max()))


def _complete(bins, N, exhaustive, layout):
    got = set(np.asarray(bins).tolist())
    if exhaustive:
        assert got == set(range(-N, N)), "%d bins are not probed" % (2 * N - len(got))
    else:
        assert set(V.bin_plan(N, False, layout).tolist()) <= got and set(V.rows_sweep(N, layout[1]).tolist()) <= got


@pytest.mark.parametrize("name,N,dflt,eopts,fwd,exhaustive,layout,Wc", WEIGHTED, ids=[r[0] for r in WEIGHTED])
def test_every_bin_through_the_weighted_entry(xc, opts, name, N, dflt, eopts, fwd, exhaustive, layout, Wc):
    """rmx_xcorr_batch_weighted, the store-side epilogue of each forward kernel: window w keeps bin s_w alone"""
    for k, v in dflt.items():
        opts(k, v)
    L = 2 * N
    iq2, prod, pmax = _scene(N)
    bins = _padded(V.bin_plan(N, exhaustive, layout), Wc)
    _complete(bins, N, exhaustive, layout)
    iq = V.tile(iq2, Wc, 2)
    w2 = np.arange(len(bins)) % 2                            # (Wc is even: window w of any call is distinct window w % 2)
    want, vmax = prod[w2, bins % L], pmax[w2]
    plain, phat = [], []
    with xc.XcorrEngine(2, N, Wc) as eng:
        eng.set_option("timing", 1)
        for k, v in eopts.items():
            eng.set_option(k, v)
        for w0 in range(0, len(bins), Wc):
            bd = V.one_bin_bands(bins[w0:w0 + Wc], N)
            plain.append(eng.correlate(iq, band=bd)[2][:, 0])
            launched = set(eng.last_timing_by_kernel())
            assert fwd <= launched and not any(f.startswith("g_win") or f == "g_rows_fused" for f in launched), launched
            phat.append(eng.correlate(iq, band=bd, whiten=True)[2][:, 0])
        print("%s: families %s, scratch %d bytes" % (name, sorted(launched), eng.scratch_bytes()))
        assert eng.scratch_bytes() <= 1 << 30
    _hold_peaks("weighted entry %s" % name, np.concatenate(plain), want, vmax)
    _hold_peaks("weighted entry %s PHAT" % name, np.concatenate(phat), np.full(len(bins), 1.0 / L), np.full(len(bins), 1.0 / L))


def _banded_calls(eng, iq, bins, Wc, N, fwd, **kw):
    """correlate_bands over per-window sets of M one-bin bands, Wc windows per call; window v of the sweep holds bins
    [M v, M v + M) -> the call's outputs concatenated, [V][M]..."""
    out = []
    for w0 in range(0, len(bins) // M, Wc):
        bd = V.one_bin_bands(bins[M * w0:M * (w0 + Wc)].reshape(Wc, M), N)
        got = eng.correlate_bands(iq, bd, **kw)
        launched = set(eng.last_timing_by_kernel())
        assert fwd <= launched and not any(f.startswith("g_win") or f in ("g_rows_fused", "g_rows_anchor") for f in launched), launched
        out.append(got)
    return tuple(np.concatenate(a) for a in zip(*out)), launched


@pytest.mark.parametrize("name,N,dflt,eopts,fwd,exhaustive,layout,Wc", BANDED, ids=[r[0] for r in BANDED])
def test_every_bin_through_the_banded_entry(xc, opts, name, N, dflt, eopts, fwd, exhaustive, layout, Wc):
    """rmx_xcorr_batch_bands, the product-on-load BandSet of each pair kernel: 64 one-bin bands per window"""
    for k, v in dflt.items():
        opts(k, v)
    L = 2 * N
    iq2, prod, pmax = _scene(N)
    bins = _padded(V.bin_plan(N, exhaustive, layout), M * Wc)
    _complete(bins, N, exhaustive, layout)
    iq = V.tile(iq2, Wc, 2)
    w2 = (np.arange(len(bins)) // M) % 2
    with xc.XcorrEngine(2, N, Wc) as eng:
        eng.set_option("timing", 1)
        for k, v in eopts.items():
            eng.set_option(k, v)
        (_, _, pk), launched = _banded_calls(eng, iq, bins, Wc, N, fwd)
        (_, _, pw), _ = _banded_calls(eng, iq, bins, Wc, N, fwd, whiten=True)
        print("%s: families %s, scratch %d bytes" % (name, sorted(launched), eng.scratch_bytes()))
        assert eng.scratch_bytes() <= 1 << 30
    assert pk.shape == (len(bins) // M, M, 1)
    _hold_peaks("banded entry %s" % name, pk.ravel(), prod[w2, bins % L], pmax[w2])
    _hold_peaks("banded entry %s PHAT" % name, pw.ravel(), np.full(len(bins), 1.0 / L), np.full(len(bins), 1.0 / L))


@pytest.mark.parametrize("name,N,dflt,eopts,fwd,exhaustive,layout,Wc", QUALITY, ids=[r[0] for r in QUALITY])
def test_every_bin_through_the_banded_quality(xc, opts, name, N, dflt, eopts, fwd, exhaustive, layout, Wc):
    """correlate_bands(quality=True): the four figures of a one-bin band are analytic (module docstring)"""
    for k, v in dflt.items():
        opts(k, v)
    L = 2 * N
    iq2, prod, pmax = _scene(N)
    bins = _padded(V.bin_plan(N, exhaustive, layout), M * Wc)
    _complete(bins, N, exhaustive, layout)
    iq = V.tile(iq2, Wc, 2)
    w2 = (np.arange(len(bins)) // M) % 2
    with xc.XcorrEngine(2, N, Wc) as eng:
        eng.set_option("timing", 1)
        for k, v in eopts.items():
            eng.set_option(k, v)
        (_, _, pk, ql), launched = _banded_calls(eng, iq, bins, Wc, N, fwd, quality=True)
        assert "k_quality" in launched, launched
        print("%s: families %s, scratch %d bytes" % (name, sorted(launched), eng.scratch_bytes()))
    _hold_peaks("banded quality %s" % name, pk.ravel(), prod[w2, bins % L], pmax[w2])
    q = ql.reshape(-1, 4).astype(np.float64)
    assert np.all(np.isfinite(q)), name
    f = np.abs(bins) / float(L)
    dev = {"coherence": np.abs(q[:, qr.COHERENCE] - 1.0).max(), "n_eff": np.abs(q[:, qr.NEFF] - 1.0).max(),
           "Et/p0^2": (np.abs(qr.et_over_p2(q, N) - L) / L).max(),
           "rms_bw": (np.abs(q[:, qr.RMS_BW] - f)[bins != 0] / f[bins != 0]).max(),
           "rms_bw at bin 0": np.abs(q[:, qr.RMS_BW][bins == 0]).max()}
    print("%s: %d bins, worst deviation %s" % (name, len(bins), ", ".join("%s %.2e" % kv for kv in dev.items())))
    for key, d in dev.items():
        assert d <= (1e-7 if key == "rms_bw at bin 0" else QTOL), (name, key, d)
    assert np.all(q[:, qr.COHERENCE] <= 1.0)
    # every bin is told apart from its neighbours: the frequencies of adjacent bins differ by 1 / L, the bar allows 1e-4 |s| / L
    assert np.all(np.abs(q[:, qr.RMS_BW] * L - np.abs(bins)) < 0.5)


# ---- a one-bin band inside a one-lag interval, per stored-spectrum layout ---------------------------------------------
MIX = [("k_fwd", 4096, {}), ("g_fwd_small", 1024, {}), ("g_rows_fwd", 65536, {})]


@pytest.mark.parametrize("fwd,N,dflt", MIX, ids=[m[0] for m in MIX])
def test_one_bin_band_inside_a_one_lag_interval(xc, opts, fwd, N, dflt):
    """64 seeded (s, k): lag_bounds = [k, k] gives the flat correlation a defined peak -- lag_int = k, lag_frac = 0, the
    peak unchanged -- through the weighted entry and through the banded one"""
    for k, v in dflt.items():
        opts(k, v)
    L = 2 * N
    W = 64
    rng = np.random.default_rng(N + 64)
    bins = np.concatenate([[-N, N - 1, 0, -1], rng.integers(-N, N, size=W - 4)])
    lags = np.concatenate([[N - 1, -(N - 1), 0, 1], rng.integers(-(N - 1), N, size=W - 4)])
    iq2, prod, pmax = _scene(N)
    iq = V.tile(iq2, W, 2)
    w2 = np.arange(W) % 2
    want, vmax = prod[w2, bins % L], pmax[w2]
    lb = np.stack([lags, lags], axis=-1).astype(np.int32)[:, None, :]
    bd = V.one_bin_bands(bins, N)
    with xc.XcorrEngine(2, N, W) as eng:
        eng.set_option("timing", 1)
        li, lf, pk = eng.correlate(iq, band=bd, lag_bounds=lb)
        assert fwd in eng.last_timing_by_kernel()
        bi, bf, bp = eng.correlate_bands(iq, bd[:, None, :], lag_bounds=lb)
        assert fwd in eng.last_timing_by_kernel()
        free = eng.correlate(iq, band=bd)[2]
    for what, a, b, c in (("weighted", li[:, 0], lf[:, 0], pk[:, 0]), ("banded", bi[:, 0, 0], bf[:, 0, 0], bp[:, 0, 0])):
        assert np.array_equal(a, lags) and not np.any(b), (fwd, what)
        _hold_peaks("one bin, one lag: %s entry %s N = %d" % (what, fwd, N), c, want, vmax)
    _hold_peaks("one bin, no bounds: weighted entry %s N = %d" % (fwd, N), free[:, 0], want, vmax)
