"""Phase 1 of the fused N = 4096 kernel stores X_1 .. X_{B-2} and not X_{B-1}: the last buoy's spectrum stays in registers
as the first anchor of phase 2, the pair table never requests it (tests/test_trail_last_buoy_sanitized.py), and its slot of
the workgroup's scratch is allocated but never written.  Buoy counts: 2 (nothing stored, no phase 2), 3 (one table step, the
dummy request right behind it), 5 and 8 (odd and even).  Every case runs six windows on a grid of two persistent workgroups
(option `ncus`), so each workgroup takes three windows one after the other through the same scratch slots, the unwritten one
included; six is the smallest count that gives both workgroups three windows, and with two CUs host::plan_route sends all six
through the fused kernel (no few-window route, no partial round), which the per-kernel timing confirms.  Bars against the
oracle: those of tests/test_gpu_parity.py for N = 4096."""
import functools

import numpy as np
import pytest

import radio_mapper_amd as rm
from oracle import xcorr_ref as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 4096
NCUS = 2
W = 3 * NCUS
BUOYS = [2, 3, 5, 8]


@pytest.fixture(scope="module")
def xc():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    assert xcorr.device_count() > 0, "no MI355X visible"
    return xcorr


@pytest.fixture
def opts(xc):
    xc.set_default_option("ncus", NCUS)
    yield xc.set_default_option
    xc.clear_default_options()


@functools.lru_cache(maxsize=None)
def _scene(B, seed=0):
    """windows, their uint8 form, the oracle's result and its top-two margins: computed once per buoy count and seed"""
    iq, _, raw = rm.synth.make_windows(W, B, N, 10e6, seed=1200 + 10 * B + seed, return_u8=True)
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


def _fused(eng, x, lb=None):
    """one call that must have run the fused kernel alone, in one launch"""
    eng.set_option("timing", 1)
    out = eng.correlate(x, lag_bounds=lb)
    t, fam = eng.last_timing(), eng.last_timing_by_kernel()
    assert set(fam) == {"k_win|k_pair"} and fam["k_win|k_pair"]["launches"] == 1, fam   # no k_fwd: the family's k_win
    assert t["fwd_launches"] == 0 and t["pair_launches"] == 1, t
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


def _same(a, b):
    return all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))


@pytest.mark.parametrize("B", BUOYS)
def test_against_the_oracle(xc, opts, B):
    iq, raw, ri, rf, rp, margin, second = _scene(B)
    with xc.XcorrEngine(B, N, W) as eng:
        li, lf, pk = _fused(eng, iq)
    assert li.shape == (W, B * (B - 1) // 2)
    _assert_parity(li, lf, pk, ri, rf, rp, margin, second)


@pytest.mark.parametrize("B", BUOYS)
def test_stale_scratch_cannot_leak(xc, opts, B):
    """batch A, then batch B on the same engine: every scratch slot holds A's spectra (the last buoy's slot whatever an
    earlier launch left there) when B starts, and B's outputs are those of an engine that never saw A"""
    a, b = _scene(B, 1)[0], _scene(B, 2)[0]
    assert not np.array_equal(a, b)
    with xc.XcorrEngine(B, N, W) as eng:
        first = _fused(eng, a)
        after = _fused(eng, b)
    with xc.XcorrEngine(B, N, W) as eng:
        fresh = _fused(eng, b)
    assert _same(after, fresh)
    assert not _same(first, fresh)            # (the two batches do differ in their results)
    iq, raw, ri, rf, rp, margin, second = _scene(B, 2)
    _assert_parity(*fresh, ri, rf, rp, margin, second)


@pytest.mark.parametrize("B", BUOYS)
def test_other_routes_agree_byte_for_byte(xc, opts, B):
    iq, raw = _scene(B)[:2]
    P = B * (B - 1) // 2
    with xc.XcorrEngine(B, N, W) as eng:
        base = _fused(eng, iq)
        # raw uint8 windows decode to exactly these samples
        assert _same(base, _fused(eng, raw))
        # k_win_lb: every interval the full one but pair 0's, which ends one lag short of it (all of them full would be the
        # unbounded call again, host::check_bounds); no peak of these scenes sits at lag N - 1
        assert int(np.abs(base[0]).max()) < N - 2
        lb = np.tile(np.array([[-(N - 1), N - 1]], np.int32), (P, 1))
        lb[0, 1] = N - 2
        assert _same(base, _fused(eng, iq, lb))
        assert _same(base, _fused(eng, raw, lb))
    # the half-order option changes scheduling only
    opts("stag", 1)
    with xc.XcorrEngine(B, N, W) as eng:
        one = _fused(eng, iq)
    opts("stag", 0)
    with xc.XcorrEngine(B, N, W) as eng:
        zero = _fused(eng, iq)
    assert _same(base, one) and _same(base, zero)
