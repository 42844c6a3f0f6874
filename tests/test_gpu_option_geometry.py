"""The four-step options that change the generic path's geometry -- col_logt, rows_tpr, logl1, cols_threads -- on the
GPU.  Each of them changes thread counts and the dynamic-LDS layout of the column or row kernels (gen_geometry.hpp:
make_geometry, cols_layout, rows_layout) and selects the run-time-length instantiations; tests/host/test_gen_geometry.cpp
holds those layouts to used <= bytes <= 160 KiB for exactly these cases before they run here.

Every case: 3 buoys x 5 windows through the four-step kernels (small_maxl = 256 sends N = 256 and N = 2048 there), the
default pair list and a custom one, plain and bounded.  Plain outputs against the float64 oracle under the bars of
tests/test_gpu_parity.py (integer lag bit-exact -- but for the oracle's own near ties, excused only where the GPU's lag is
the oracle's second candidate --, lag within 1e-5 * max(|lag|, 1), peak rtol 1e-5); bounded outputs against the sliced
reference under the bars of tests/test_gpu_lag_bounds.py.  The kernel families that ran are asserted."""
import functools

import numpy as np
import pytest

import radio_mapper_amd as rm
from lag_bounds_ref import bounded_batch
from oracle import xcorr_ref as orc

pytestmark = pytest.mark.gpu
TOL = 1e-5
B, W = 3, 5
CUSTOM = np.array([(2, 0), (0, 1), (1, 1)], np.int32)      # reversed, plain, autocorrelation
FOUR_STEP = {"g_cols_fwd", "g_rows_fwd", "g_rows_inv", "g_cols_inv", "g_final"}

# (N, option, value)
CASES = [(256, "col_logt", 3), (256, "rows_tpr", 4), (256, "logl1", 4),
         (2048, "col_logt", 5), (2048, "rows_tpr", 64), (2048, "cols_threads", 128)]


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


def _random_bounds(rng, shape, N):
    a = rng.integers(-(N - 1), N, size=shape + (2,))
    lo, hi = np.minimum(a[..., 0], a[..., 1]), np.maximum(a[..., 0], a[..., 1])
    return np.stack([lo, hi], -1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _reference(N):
    """the windows of length N and every reference the cases of that length share (computed once, never written to)"""
    iq, _ = rm.synth.make_windows(W, B, N, 2.4e6, seed=2000 + N)
    rng = np.random.default_rng(N)
    ref = {"iq": iq}
    for name, pairs in (("default", None), ("custom", CUSTOM)):
        plist = orc.pair_list(B) if pairs is None else pairs
        margin = np.zeros((W, len(plist)))
        second = np.zeros((W, len(plist)), np.int64)
        for w in range(W):
            for q, (i, j) in enumerate(plist):
                margin[w, q], _, second[w, q] = orc.peak_top2(iq[w, i], iq[w, j])
        lb = _random_bounds(rng, (W, len(plist)), N)
        plain = orc.xcorr_batch_literal(iq) if pairs is None else orc.xcorr_batch_literal(iq, pairs)
        ref[name] = dict(plain=plain, margin=margin, second=second, lb=lb, bounded=bounded_batch(iq, lb, pairs))
    return ref


def _assert_parity(li, lf, pk, ri, rf, rp, margin, second):
    """tests/test_gpu_parity.py: _assert_parity"""
    ref = ri + rf
    got = li + lf.astype(np.float64)
    bad = li != ri
    excused = bad & (margin <= TOL) & (li == second)
    assert not np.any(bad & ~excused), f"{int(np.sum(bad & ~excused))} integer lags differ"
    ok = ~bad
    assert np.all(np.abs(got[ok] - ref[ok]) <= TOL * np.maximum(np.abs(ref[ok]), 1.0)), \
        "fractional lag outside 1e-5: max %.3e" % np.abs(got[ok] - ref[ok]).max()
    assert np.allclose(pk[ok], rp[ok], rtol=1e-5, atol=0)


def _assert_sliced(li, lf, pk, ref):
    """tests/test_gpu_lag_bounds.py: _assert_sliced"""
    ri, rf, rp, mg, fm = ref
    ok = mg > TOL                                      # the parity rule: bit-exact where the slice's top two differ
    assert np.array_equal(li[ok], ri[ok]), "integer lags differ from the sliced reference: %d" % int((li != ri)[ok].sum())
    got, want = li[ok] + lf[ok].astype(np.float64), ri[ok] + rf[ok]
    assert np.all(np.abs(got - want) <= TOL * np.maximum(np.abs(want), 1.0)), np.abs(got - want).max()
    assert np.all(np.abs(pk[ok] - rp[ok]) <= 1e-5 * rp[ok] + 1e-6 * fm[ok])


@pytest.mark.parametrize("N,key,value", CASES, ids=["N%d-%s=%d" % c for c in CASES])
def test_option_geometry_four_step(xc, opts, N, key, value):
    ref = _reference(N)
    iq = ref["iq"]
    opts("small_maxl", 256)
    opts(key, value)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        for name, pairs in (("default", None), ("custom", CUSTOM)):
            r = ref[name]
            li, lf, pk = eng.correlate(iq, pairs)
            assert set(eng.last_timing_by_kernel()) == FOUR_STEP, (name, eng.last_timing_by_kernel())
            _assert_parity(li, lf, pk, *r["plain"], r["margin"], r["second"])
            li, lf, pk = eng.correlate(iq, pairs, lag_bounds=r["lb"])
            assert set(eng.last_timing_by_kernel()) == FOUR_STEP, (name, "bounded", eng.last_timing_by_kernel())
            assert np.all((li >= r["lb"][..., 0]) & (li <= r["lb"][..., 1]))
            _assert_sliced(li, lf, pk, r["bounded"])
