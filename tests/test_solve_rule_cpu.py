"""rmx_solve_batch without a GPU: the kernel-order restatement of k_solve (tests/solve_kernel_ref.py) against the oracle it
must agree with where the oracle is well conditioned, the properties of the documented Levenberg-Marquardt rule pinned on
the restatement (tests/test_gpu_solve_exact.py then holds the kernel to the restatement bit for bit), the give-up on
degenerate input, and the shape checks of XcorrEngine.solve before any C call."""
import ctypes as C

import numpy as np
import pytest

import solve_kernel_ref as kr
from oracle import solve_ref as sr
from radio_mapper_amd import tdoa_processor as tp
from radio_mapper_amd import xcorr
from test_solve import scenario


def _eq(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# -- the restatement against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_buoys,noise_m", [(4, 0.0), (5, 3.0), (8, 10.0), (16, 5.0)])
def test_restatement_meets_the_oracle_bars(n_buoys, noise_m):
    """the scenarios and the bars of test_solve.test_gpu_solve_matches_oracle, with the restatement in the kernel's place"""
    W = 300
    buoys, tx, pairs, li, lf, fs = scenario(n_buoys, W, seed=10 + n_buoys, noise_m=noise_m)
    wgt = (1.0 / (np.random.default_rng(3).uniform(0.2, 1.0, li.shape) + 0.1)).astype(np.float32)
    rpos, rf, rit = sr.solve_batch(buoys, pairs, sr.lags_to_dist(li, lf, fs), wgt)
    pos, f, it = kr.solve_kernel_order(buoys, pairs, li, lf, wgt, kr.metres_per_sample(fs))
    P = len(pairs)
    good = rf < 20.0 * wgt.max() * P * max(noise_m, 0.02) ** 2
    print("good share %.3f, cost rel %.2e, pos %.2e m, median iters %g / %g" % (
        good.mean(), (np.abs(f - rf)[good] / np.maximum(rf[good], 1e-6)).max(),
        np.linalg.norm(pos - rpos, axis=1)[good].max(), np.median(it[good]), np.median(rit[good])))
    assert good.mean() > 0.9
    assert np.all(np.abs(f - rf)[good] <= 1e-6 * np.maximum(rf[good], 1e-6))
    good_k = f < 20.0 * wgt.max() * P * max(noise_m, 0.02) ** 2
    assert abs(good_k.mean() - good.mean()) < 0.03
    assert np.linalg.norm(pos - rpos, axis=1)[good].max() < 1e-3
    assert abs(np.median(it[good]) - np.median(rit[good])) <= 2 and it.max() <= 60


# -- properties of the rule ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk():
    """a case with everything in it: windows that converge early, windows on the cap of 60, rejected steps"""
    buoys, tx, pairs, li, lf, fs = scenario(4, 70, seed=14, noise_m=5.0)
    wgt = (1.0 / (np.random.default_rng(3).uniform(0.2, 1.0, li.shape) + 0.1)).astype(np.float32)
    mps = kr.metres_per_sample(fs)
    full = kr.solve_kernel_order(buoys, pairs, li, lf, wgt, mps)
    assert full[2].min() < 10 and full[2].max() == 60        # the case is what the docstring says
    return buoys, pairs, li, lf, wgt, mps, full


def test_max_iter_cuts_the_same_walk(walk):
    buoys, pairs, li, lf, wgt, mps, (pos, cost, it) = walk
    prev = None
    for k in (1, 2, 7):
        pk, ck, ik = kr.solve_kernel_order(buoys, pairs, li, lf, wgt, mps, max_iter=k)
        assert np.array_equal(ik, np.minimum(it, k))
        assert np.all(ck >= cost)
        assert prev is None or np.all(ck <= prev)
        done = it <= k                                       # finished within k iterations: the final result already
        assert np.array_equal(pk[done], pos[done]) and np.array_equal(ck[done], cost[done])
        prev = ck
    # the cap of 60 is a cap: with 200 the windows that sat on it move on, the others keep their bits
    p2, c2, i2 = kr.solve_kernel_order(buoys, pairs, li, lf, wgt, mps, max_iter=200)
    capped = it == 60
    assert np.all(i2[capped] >= 60) and (i2[capped] > 60).any() and np.all(c2 <= cost)
    assert np.array_equal(p2[~capped], pos[~capped]) and np.array_equal(i2[~capped], it[~capped])


def test_swapping_every_pair_and_negating_the_lags_changes_no_bit(walk):
    """(j, i) with -lag is the same measurement: n1 and n2 trade places, r and every Jacobian entry change sign exactly"""
    buoys, pairs, li, lf, wgt, mps, full = walk
    assert _eq(kr.solve_kernel_order(buoys, pairs[:, ::-1], -li, -lf, wgt, mps), full)


def test_unit_weights_are_no_weights(walk):
    buoys, pairs, li, lf, _, mps, _ = walk
    a = kr.solve_kernel_order(buoys, pairs, li, lf, None, mps)
    assert _eq(kr.solve_kernel_order(buoys, pairs, li, lf, np.ones(li.shape, np.float32), mps), a)


def test_windows_are_independent(walk):
    buoys, pairs, li, lf, wgt, mps, full = walk
    perm = np.random.default_rng(8).permutation(li.shape[0])
    got = kr.solve_kernel_order(buoys, pairs, li[perm], lf[perm], wgt[perm], mps)
    assert _eq(got, [a[perm] for a in full])
    one = kr.solve_kernel_order(buoys, pairs, li[5:6], lf[5:6], wgt[5:6], mps)
    assert _eq(one, [a[5:6] for a in full])


# -- degenerate inputs: finite outputs and the documented give-up ----------------------------------------------------------
def _centroid(buoys):
    c = np.zeros(3)
    for b in buoys:
        c = c + b
    return c / len(buoys)


def test_all_zero_weights_give_up_at_the_start_point():
    buoys, tx, pairs, li, lf, fs = scenario(5, 7, seed=15, noise_m=3.0)
    pos, cost, it = kr.solve_kernel_order(buoys, pairs, li, lf, np.zeros(li.shape, np.float32), kr.metres_per_sample(fs))
    assert np.all(it == 25) and np.all(cost == 0.0) and np.all(pos == _centroid(buoys))
    pos, cost, it = kr.solve_kernel_order(buoys, pairs, li, lf, np.zeros(li.shape, np.float32), kr.metres_per_sample(fs), 7)
    assert np.all(it == 7) and np.all(cost == 0.0) and np.all(pos == _centroid(buoys))


@pytest.mark.parametrize("ks,on_buoy", [((1, 0, -1), 1), ((-3, -1, 0.5, 2, 4), 2)])
def test_a_centroid_on_a_buoy_rejects_every_step(ks, on_buoy):
    """0 / 0 in every Jacobian entry of the pairs with that buoy: A is NaN, `d00 > 0` is false, 25 rejections take lambda
    from 1e-3 past 1e12 (4^25 e-3 = 1.13e12, 4^24 e-3 = 2.8e11)"""
    buoys = kr.line_of_buoys(ks)
    assert np.array_equal(_centroid(buoys), buoys[on_buoy])
    pairs = kr.all_pairs(len(ks))
    li, lf = kr.seeded_lags(4, len(pairs), seed=5)
    pos, cost, it = kr.solve_kernel_order(buoys, pairs, li, lf, None, kr.metres_per_sample(10e6))
    assert np.all(it == 25) and np.all(pos == buoys[on_buoy]) and np.all(np.isfinite(cost)) and np.all(cost > 0)


def test_the_give_up_count_follows_from_the_constants():
    lam, n = 1e-3, 0
    while True:
        n += 1
        lam *= 4.0
        if lam > 1e12:
            break
    assert n == 25


# -- the binding: shapes are checked before the library reads W * P elements -------------------------------------------------
class _NoCall(xcorr.XcorrEngine):
    def __init__(self):   # no library, no ctx: a C call would fail with AttributeError, not ValueError
        self.n_buoys, self.n_samples = 3, 16

    def __del__(self):
        pass


def _args(W=4, B=4):
    P = B * (B - 1) // 2
    return dict(buoy_xyz=np.arange(3.0 * B).reshape(B, 3), lag_int=np.zeros((W, P), np.int32),
                lag_frac=np.zeros((W, P), np.float32), sample_rate_hz=10e6)


_BAD = {
    "lag_int 1-D": (dict(lag_int=np.zeros(6, np.int32), lag_frac=np.zeros(6, np.float32)), "lag_int"),
    "lag_int 3-D": (dict(lag_int=np.zeros((2, 2, 6), np.int32)), "lag_int"),
    "lag_frac one row": (dict(lag_frac=np.zeros(6, np.float32)), "lag_frac"),
    "lag_frac transposed": (dict(lag_frac=np.zeros((6, 4), np.float32)), "lag_frac"),
    "lag_frac fewer windows": (dict(lag_frac=np.zeros((3, 6), np.float32)), "lag_frac"),
    "weight of length W": (dict(weight=np.ones(4, np.float32)), "weight"),
    "weight [1][P]": (dict(weight=np.ones((1, 6), np.float32)), "weight"),
    "weight transposed": (dict(weight=np.ones((6, 4), np.float32)), "weight"),
    "weight scalar": (dict(weight=1.0), "weight"),
    "one buoy": (dict(buoy_xyz=np.zeros((1, 3))), "buoy_xyz"),
    "65 buoys": (dict(buoy_xyz=np.zeros((65, 3))), "buoy_xyz"),
    "buoys not [B][3]": (dict(buoy_xyz=np.zeros((4, 2))), "buoy_xyz"),
    "pairs of another length": (dict(pairs=np.zeros((5, 2), np.int32)), "pairs"),
    "pairs odd": (dict(pairs=np.zeros(11, np.int32)), "pairs"),
    "no pairs, P != B(B-1)/2": (dict(lag_int=np.zeros((4, 5), np.int32), lag_frac=np.zeros((4, 5), np.float32)), "pairs"),
    "max_iter 0": (dict(max_iter=0), "max_iter"),
    "max_iter -3": (dict(max_iter=-3), "max_iter"),
    "fs 0": (dict(sample_rate_hz=0.0), "sample_rate_hz"),
    "fs negative": (dict(sample_rate_hz=-1.0), "sample_rate_hz"),
    "fs NaN": (dict(sample_rate_hz=float("nan")), "sample_rate_hz"),
}


@pytest.mark.parametrize("case", sorted(_BAD))
def test_solve_refuses_before_any_call(case):
    change, name = _BAD[case]
    with pytest.raises(ValueError, match=name):
        _NoCall().solve(**{**_args(), **change})


@pytest.mark.parametrize("change", [
    {}, dict(weight=np.ones((4, 6))), dict(weight=np.ones(6)), dict(pairs=np.zeros((6, 2), np.int32)),
    dict(pairs=np.zeros(12, np.int64)), dict(max_iter=1), dict(buoy_xyz=np.zeros(12)),
    dict(lag_int=np.zeros((4, 2), np.int32), lag_frac=np.zeros((4, 2), np.float32), pairs=[[0, 1], [1, 1]]),
], ids=["plain", "weight [W][P]", "weight [P]", "pairs [P][2]", "pairs flat", "max_iter 1", "buoys flat", "custom P"])
def test_an_accepted_solve_reaches_the_library(change):
    """the checks pass and the call goes to the C entry: without a library that is an AttributeError, not a ValueError"""
    with pytest.raises(AttributeError):
        _NoCall().solve(**{**_args(), **change})


def test_no_windows_is_no_call():
    pos, cost, it = _NoCall().solve(np.zeros((4, 3)), np.zeros((0, 6), np.int32), np.zeros((0, 6), np.float32), 10e6)
    assert pos.shape == (0, 3) and cost.shape == (0,) and it.shape == (0,)


class _Recorder:
    """stands in for the loaded library: keeps what rmx_solve_batch would have read through each pointer"""

    def __init__(self):
        self.seen = None

    def rmx_solve_batch(self, ctx, bx, B, pp, P, li, lf, wp, fs, W, max_iter, pos, cost, iters, flags):
        def read(p, ctype, n):
            return None if p is None else np.array((ctype * n).from_address(p.value))
        self.seen = dict(B=B, P=P, W=W, fs=fs, max_iter=max_iter, flags=flags, buoys=read(bx, C.c_double, 3 * B),
                         pairs=read(pp, C.c_int32, 2 * P), li=read(li, C.c_int32, W * P), lf=read(lf, C.c_float, W * P),
                         weight=read(wp, C.c_float, W * P))
        return 0


class _Recording(_NoCall):
    def __init__(self):
        super().__init__()
        self._lib, self._ctx = _Recorder(), None


def test_one_weight_row_is_broadcast_to_every_window():
    """the library reads W * P floats through the weight pointer: a row of P is handed over as W copies of itself"""
    a = _args(W=5)
    row = np.linspace(0.5, 3.0, 6)
    eng = _Recording()
    eng.solve(**a, weight=row)
    assert eng._lib.seen["W"] == 5 and eng._lib.seen["P"] == 6
    assert np.array_equal(eng._lib.seen["weight"].reshape(5, 6), np.tile(row.astype(np.float32), (5, 1)))
    eng.solve(**a, weight=np.tile(row, (5, 1)))
    assert np.array_equal(eng._lib.seen["weight"].reshape(5, 6), np.tile(row.astype(np.float32), (5, 1)))
    eng.solve(**a)
    assert eng._lib.seen["weight"] is None and eng._lib.seen["pairs"] is None and eng._lib.seen["flags"] == 0


def test_triangulate_batch_takes_one_confidence_row():
    """HyperbolicPositioning.triangulate_batch(confidence = one row of P): weight = 1 / (confidence + 0.1) for all windows"""
    buoys = [tp.BuoyPosition("b%d" % i, 51.5 + 0.01 * i, -0.1 + 0.02 * (i % 2), 10.0 * i) for i in range(4)]
    li, lf = np.zeros((5, 6), np.int32), np.zeros((5, 6), np.float32)
    conf = np.linspace(0.3, 0.9, 6)
    eng = _Recording()
    out = tp.HyperbolicPositioning().triangulate_batch(eng, buoys, li, lf, 10e6, confidence=conf)
    assert len(out) == 5
    want = (1.0 / (conf + 0.1)).astype(np.float32)
    assert np.array_equal(eng._lib.seen["weight"].reshape(5, 6), np.tile(want, (5, 1)))
    with pytest.raises(ValueError, match="weight"):
        tp.HyperbolicPositioning().triangulate_batch(eng, buoys, li, lf, 10e6, confidence=np.ones(5))
    with pytest.raises(ValueError, match="lag_frac"):
        tp.HyperbolicPositioning().triangulate_batch(eng, buoys, li, lf[0], 10e6)
