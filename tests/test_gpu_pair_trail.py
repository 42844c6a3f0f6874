"""The fused N = 4096 kernel walks the pairs among buoys 1 .. B-1 in a host-planned order (host::plan_pair_trail: runs
that hand the anchor over): the spectrum two consecutive pairs share stays in its register array, and each pair requests
one spectrum into the other array, which is sa or sb.  Buoy counts: 2 (no step), 3 (one step, nothing requested), 4 (the
smallest with a handover and with requests into both arrays), 5 (odd: an Eulerian trail would have to reload here, this
order does not), 8 (the benchmark's shape), 9, 16 (runs of 14 ... 1 pairs).  Each through the engine with the fused route
forced, against the oracle with the bars of tests/test_gpu_parity.py, against the per-transform kernels of the same build
(integer lags exactly), for complex64 and uint8 windows, and through the bounded kernel (k_win_lb) at 4 and 8 buoys.  Two
persistent workgroups (option ncus): one of them runs a second window behind its first, so the tables and rings carry
over.  The half-order option `stag` changes scheduling only: its former default 1 gives the default's bytes."""
import functools

import numpy as np
import pytest

import radio_mapper_amd as rm
from oracle import xcorr_ref as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 4096
CASES = [(2, 3), (3, 3), (4, 3), (5, 3), (8, 3), (9, 3), (16, 2)]   # (buoys, windows)


@pytest.fixture(scope="module")
def xc():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    assert xcorr.device_count() > 0, "no MI355X visible"
    return xcorr


@pytest.fixture
def opts(xc):
    yield xc.set_default_option
    xc.clear_default_options()


@functools.lru_cache(maxsize=None)
def _scene(B, W):
    """windows, their uint8 form, the oracle's result and its top-two margins: computed once per buoy count"""
    iq, _, raw = rm.synth.make_windows(W, B, N, 10e6, seed=900 + B, return_u8=True)
    ri, rf, rp = orc.xcorr_batch_fast(iq, workers=4)
    plist = orc.pair_list(B)
    margin = np.zeros((W, len(plist)))
    second = np.zeros((W, len(plist)), np.int64)
    for w in range(W):
        for q, (i, j) in enumerate(plist):
            margin[w, q], _, second[w, q] = orc.peak_top2(iq[w, i], iq[w, j])
    for a in (iq, raw, ri, rf, rp, margin, second):
        a.setflags(write=False)
    return iq, raw, ri, rf, rp, margin, second


def _run(xc, B, W, x, fused, lb=None):
    """one call on a two-workgroup engine; fused: k_win / k_win_lb alone, else the per-transform kernels"""
    with xc.XcorrEngine(B, N, W) as eng:
        if fused:
            eng.set_option("small4096", 0)
        else:
            eng.set_option("fused", 0)
        eng.set_option("timing", 1)
        out = eng.correlate(x, lag_bounds=lb)
        t = eng.last_timing()
    assert t["pair_launches"] >= 1
    assert (t["fwd_launches"] == 0) == fused, t   # the fused kernel has no forward launch of its own
    return out


def _assert_parity(li, lf, pk, ri, rf, rp, margin, second):
    """tests/test_gpu_parity.py: integer lags bit-exact unless the oracle's own two largest magnitudes are within 1e-5
    and the GPU took the second; |lag - ref| <= 1e-5 max(|ref|, 1); peak rtol 1e-5"""
    ref = ri + rf
    got = li + lf.astype(np.float64)
    bad = li != ri
    excused = bad & (margin <= TOL) & (li == second)
    assert not np.any(bad & ~excused), f"{int(np.sum(bad & ~excused))} integer lags differ"
    ok = ~bad
    assert np.all(np.abs(got[ok] - ref[ok]) <= TOL * np.maximum(np.abs(ref[ok]), 1.0)), \
        "fractional lag outside 1e-5: max %.3e" % np.abs(got[ok] - ref[ok]).max()
    assert np.allclose(pk[ok], rp[ok], rtol=1e-5, atol=0)


@pytest.mark.parametrize("B,W", CASES)
def test_trail_against_oracle_and_per_transform_route(xc, opts, B, W):
    iq, raw, ri, rf, rp, margin, second = _scene(B, W)
    opts("ncus", 2)
    li, lf, pk = _run(xc, B, W, iq, fused=True)
    assert li.shape == (W, B * (B - 1) // 2)
    _assert_parity(li, lf, pk, ri, rf, rp, margin, second)
    # uint8 windows decode to exactly these samples: the same bytes out
    l8, f8, p8 = _run(xc, B, W, raw, fused=True)
    assert np.array_equal(li, l8) and np.array_equal(lf, f8) and np.array_equal(pk, p8)
    # k_fwd + the pair kernels of the same build
    ui, uf, up = _run(xc, B, W, iq, fused=False)
    assert np.array_equal(li, ui)
    assert np.all(np.abs(lf - uf) <= TOL) and np.allclose(pk, up, rtol=1e-5, atol=0)
    u8i, _, _ = _run(xc, B, W, raw, fused=False)
    assert np.array_equal(l8, u8i)


@pytest.mark.parametrize("B,W", [(4, 3), (8, 3)])
def test_trail_in_the_bounded_kernel(xc, opts, B, W):
    """k_win_lb shares the body: a lag window per pair that holds every true peak leaves the oracle's answer"""
    iq, raw, ri, rf, rp, margin, second = _scene(B, W)
    P = B * (B - 1) // 2
    half = int(np.abs(ri).max()) + 8
    assert half < N - 1                      # a proper sub-interval: the bounded kernel, not the full-range shortcut
    lb = np.empty((P, 2), np.int32)
    lb[:, 0], lb[:, 1] = -half, half
    opts("ncus", 2)
    li, lf, pk = _run(xc, B, W, iq, fused=True, lb=lb)
    _assert_parity(li, lf, pk, ri, rf, rp, margin, second)
    l8, f8, p8 = _run(xc, B, W, raw, fused=True, lb=lb)
    assert np.array_equal(li, l8) and np.array_equal(lf, f8) and np.array_equal(pk, p8)
    ui, uf, up = _run(xc, B, W, iq, fused=False, lb=lb)
    assert np.array_equal(li, ui)
    assert np.all(np.abs(lf - uf) <= TOL) and np.allclose(pk, up, rtol=1e-5, atol=0)


def test_half_order_one_gives_the_default_bytes(xc, opts):
    """`stag` 0 is the default since h1 stands once between two copies of h2; tests/test_gpu_parity.py sets 0 and 2 ... 5
    against the default, this one 1, which some waves run through the second copy of h2"""
    B, W = 8, 3
    iq = _scene(B, W)[0]
    opts("ncus", 2)
    base = _run(xc, B, W, iq, fused=True)
    opts("stag", 1)
    got = _run(xc, B, W, iq, fused=True)
    for a, b in zip(base, got):
        assert np.array_equal(a, b)
