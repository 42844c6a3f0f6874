"""The forward transform of the fused N = 4096 kernel exchanges through an image of its own, [k0][n1][n0 >> 3][p][n0 & 7]
(fft_r16.hpp: role A's stores without the bank conflict, role B's reads as sixteen ds_read_b64 of one asm statement), while
the 28 inverse transforms of a window keep [k0][n1][p][n0].  A wrong index on either side of that image would hand a thread
another thread's value, so every check here is on data that differs in every row and lane of the image: noise windows
(every sample distinct) and impulses (every bin a different phase), the latter with peaks at the ends of the lag range.

Option `small4096` = 0 sends these few windows through the fused kernel, option `ncus` sets its grid: one window on one
workgroup, three windows on three workgroups, and three windows on ONE workgroup (one after the other through the same
exchange images and the same spectrum scratch).  The per-kernel timing confirms the route.  2, 3, 5 and 8 buoys: no phase
2, one table step, odd and even.  Four kernels: k_win and k_win_lb, each for complex64 and for raw uint8 windows.

Bars against oracle.xcorr_ref.xcorr_batch_fast: those of tests/test_gpu_parity.py for this route (integer lags bit-exact
unless the oracle's own two largest magnitudes are within 1e-5 and the GPU took the second; |lag - ref| <= 1e-5 max(|ref|,
1); peak rtol 1e-5).  The four kernels agree byte for byte."""
import functools

import numpy as np
import pytest

import far_lag_ref as F
import radio_mapper_amd as rm
from oracle import xcorr_ref as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 4096
BUOYS = [2, 3, 5, 8]
GRIDS = [(1, 1), (3, 3), (3, 1)]          # (windows, persistent workgroups)
# impulse lags: both ends of the range (-(N - 1) itself; the last two lags of the other end are left free for pair 0's
# shortened window below, whose edge lag would lose its fractional part), the seams of the wave / slot / half split of the
# peak search, and lags in between
IMPULSE_LAGS = [-(N - 1), -(N - 2), -2049, -2048, -257, -33, -1, 0, 1, 31, 32, 255, 256, 1023, 2047, 3000, N - 4, N - 3]


@pytest.fixture(scope="module")
def xc():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    assert xcorr.device_count() > 0, "no MI355X visible"
    return xcorr


@pytest.fixture
def opts(xc):
    xc.set_default_option("small4096", 0)
    yield xc.set_default_option
    xc.clear_default_options()


@functools.lru_cache(maxsize=None)
def _noise(B):
    """three windows, their uint8 form, the oracle's result and its top-two margins: once per buoy count"""
    iq, _, raw = rm.synth.make_windows(3, B, N, 10e6, seed=1700 + 10 * B, return_u8=True)
    ri, rf, rp = orc.xcorr_batch_fast(iq, workers=4)
    plist = orc.pair_list(B)
    margin = np.zeros((3, len(plist)))
    second = np.zeros((3, len(plist)), np.int64)
    for w in range(3):
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
    assert set(fam) == {"k_win|k_pair"} and fam["k_win|k_pair"]["launches"] == 1, fam
    assert t["fwd_launches"] == 0 and t["pair_launches"] == 1, t
    return out


def _assert_parity(li, lf, pk, ri, rf, rp, margin, second):
    ref = ri + rf
    got = li + lf.astype(np.float64)
    bad = li != ri
    excused = bad & (margin <= TOL) & (li == second)
    assert not np.any(bad & ~excused), f"{int(np.sum(bad & ~excused))} integer lags differ"
    ok = ~bad
    err = np.abs(got[ok] - ref[ok])
    print("max |dlag| %.3e, max peak rel %.3e" % (err.max(), np.abs(pk[ok] / rp[ok] - 1.0).max()))
    assert np.all(err <= TOL * np.maximum(np.abs(ref[ok]), 1.0)), "fractional lag outside 1e-5: max %.3e" % err.max()
    assert np.allclose(pk[ok], rp[ok], rtol=1e-5, atol=0)


def _same(a, b):
    return all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))


def _full_window(B, base_li):
    """k_win_lb's widest request: every interval the full one but pair 0's, which ends one lag short of the range on a side
    where none of its peaks sits (all of them full would be the unbounded call again, host::check_bounds)"""
    lb = np.tile(np.array([[-(N - 1), N - 1]], np.int32), (B * (B - 1) // 2, 1))
    if not np.any(base_li[:, 0] >= N - 2):
        lb[0, 1] = N - 2
    else:
        assert not np.any(base_li[:, 0] <= -(N - 2))
        lb[0, 0] = -(N - 2)
    return lb


@pytest.mark.parametrize("W,ncus", GRIDS)
@pytest.mark.parametrize("B", BUOYS)
def test_noise_windows_through_all_four_kernels(xc, opts, B, W, ncus):
    iq, raw, ri, rf, rp, margin, second = (a[:W] for a in _noise(B))
    opts("ncus", ncus)
    with xc.XcorrEngine(B, N, W) as eng:
        base = _fused(eng, iq)
        lb = _full_window(B, base[0])
        others = [_fused(eng, raw), _fused(eng, iq, lb), _fused(eng, raw, lb)]
    assert base[0].shape == (W, B * (B - 1) // 2)
    _assert_parity(*base, ri, rf, rp, margin, second)
    for k, o in enumerate(others):
        assert _same(base, o), ("k_win uint8", "k_win_lb complex64", "k_win_lb uint8")[k]


@pytest.mark.parametrize("B", BUOYS)
def test_impulses_with_peaks_at_the_ends_of_the_range(xc, opts, B):
    """x_b = C_b d[p_b]: every pair's correlation is one sample at lag p_j - p_i, from -(N - 1) to N - 2, and every spectrum
    a pure phase ramp (no two bins alike); two workgroups share the windows"""
    # (pairs among buoys 1 .. B-1 reach lags beyond the list's, up to +-(N - 1), whenever a window holds both signs)
    iq, pos, amp = F.impulse_scene(N, IMPULSE_LAGS, B, 1700 + B)
    W = len(iq)
    ri, rf, rp = orc.xcorr_batch_fast(iq, workers=4)
    ai, ap = F.impulse_ref(pos, amp, orc.pair_list(B))
    assert np.array_equal(ri, ai) and np.allclose(rp, ap, rtol=1e-5)      # the oracle finds what the scene was built with
    assert ri.min() == -(N - 1) and ri.max() >= N - 3
    opts("ncus", 2)
    with xc.XcorrEngine(B, N, W) as eng:
        li, lf, pk = base = _fused(eng, iq)
        bounded = _fused(eng, iq, _full_window(B, li))
    assert np.array_equal(li, ri), f"{int(np.sum(li != ri))} integer lags differ"
    ref = ri + rf
    err = np.abs(li + lf.astype(np.float64) - ref)
    print("max |dlag| %.3e, max peak rel %.3e" % (err.max(), np.abs(pk / rp - 1.0).max()))
    assert np.all(err <= TOL * np.maximum(np.abs(ref), 1.0))
    assert np.allclose(pk, rp, rtol=1e-5, atol=0)
    assert _same(base, bounded)
