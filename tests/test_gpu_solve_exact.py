"""k_solve through rmx_solve_batch against its kernel-order restatement (tests/solve_kernel_ref.py): pos, cost and iters
equal bit for bit (np.array_equal) for EVERY window -- no mask of converged windows, no tolerance, no excused share.
tests/test_solve.py compares with oracle/solve_ref.py, which sums in numpy's order and can therefore only be held to the
windows that reach the global minimum; a wrong constant of the rule, a wrong index in the tail of the last block or in a
window that does not converge, more than 16 buoys, custom pair lists, the pointer flags, ctx reuse and the refusals of
the entry are all invisible there.  The restatement itself is held to the oracle and to the rule in
tests/test_solve_rule_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import radio_mapper_amd as rm
import solve_kernel_ref as kr
from oracle import solve_ref as sr
from test_solve import scenario

pytestmark = pytest.mark.gpu

FS = 10e6
MPS = kr.metres_per_sample(FS)
RMX_E_INVAL = -1


@pytest.fixture(scope="module")
def xc():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    assert xcorr.device_count() > 0, "no MI355X visible"
    return xcorr


def _engine(xc):
    # the solve entry uses nothing of the ctx but its stream and its solve buffers: any engine will do
    return xc.XcorrEngine(3, 256, 2)


def _weights(shape):
    """float32 weights drawn as test_solve.test_gpu_solve_matches_oracle draws them: 1 / (confidence + 0.1)"""
    return (1.0 / (np.random.default_rng(3).uniform(0.2, 1.0, shape) + 0.1)).astype(np.float32)


_REF = {}


def _ref(key, buoys, pairs, li, lf, wgt, max_iter=60):
    """the restatement's result, computed once per case and shared read-only"""
    if key not in _REF:
        out = kr.solve_kernel_order(buoys, pairs, li, lf, wgt, MPS, max_iter)
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _assert_exact(got, ref, what):
    (pos, cost, it), (rpos, rcost, rit) = got, ref
    bad = np.any(pos != rpos, axis=1) | (cost != rcost) | (it != rit)
    with np.errstate(all="ignore"):
        msg = "%s: %d of %d windows differ (first %s); max |dpos| %.3e m, max |dcost| %.3e relative, %d iteration counts" % (
            what, bad.sum(), len(bad), np.flatnonzero(bad)[:5], np.abs(pos - rpos).max(initial=0.0),
            (np.abs(cost - rcost) / np.maximum(np.abs(rcost), 1e-300)).max(initial=0.0), (it != rit).sum())
    print(msg)
    assert np.array_equal(pos, rpos) and np.array_equal(cost, rcost) and np.array_equal(it, rit), msg


def _lags_for(buoys, tx, pairs, noise_m, seed):
    """physical lags of an arbitrary pair list (test_solve.scenario only makes them for all i < j)"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    dist = np.linalg.norm(tx[:, None, :] - buoys[None, :, :], axis=2)
    dd = dist[:, pairs[:, 1]] - dist[:, pairs[:, 0]]
    dd = dd + np.random.default_rng(seed).normal(0.0, noise_m, dd.shape)
    lag = dd / sr.SPEED_OF_LIGHT * FS
    li = np.round(lag).astype(np.int32)
    return li, (lag - li).astype(np.float32)


# -- by buoy count and block tail ---------------------------------------------------------------------------------------------
# 64 threads a block: 70 and 130 leave a tail of 6 and 2, 65 of 1, 63 is one short, 64 exact; 33 and 64 buoys are 528 and
# 2016 pairs, beyond anything the oracle tests reach; (5, 1) is one window alone
CASES = [(2, 70, 1), (3, 130, 0), (4, 130, 0), (4, 130, 5), (5, 65, 3), (8, 64, 10), (16, 63, 5), (33, 20, 5), (64, 6, 5),
         (5, 1, 3)]


def _case(B, W, noise_m):
    buoys, tx, pairs, li, lf, fs = scenario(B, W, seed=10 + B, noise_m=float(noise_m))
    assert fs == FS
    return buoys, tx, pairs, li, lf


@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "no_weights"])
@pytest.mark.parametrize("B,W,noise_m", CASES)
def test_every_window_bit_for_bit(xc, B, W, noise_m, weighted):
    buoys, tx, pairs, li, lf = _case(B, W, noise_m)
    wgt = _weights(li.shape) if weighted else None
    ref = _ref(("case", B, W, noise_m, weighted), buoys, pairs, li, lf, wgt)
    with _engine(xc) as eng:
        got = eng.solve(buoys, li, lf, FS, weight=wgt)
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    _assert_exact(got, ref, "B %d W %d noise %g" % (B, W, noise_m))


def test_one_weight_row_for_all_windows_and_unit_weights(xc):
    """the binding broadcasts a 1-D weight of length P to [W][P]; a row of ones is the call without weights, bit for bit"""
    buoys, tx, pairs, li, lf = _case(5, 65, 3)
    row = _weights(li.shape)[0]
    with _engine(xc) as eng:
        a = eng.solve(buoys, li, lf, FS, weight=row)
        b = eng.solve(buoys, li, lf, FS, weight=np.tile(row, (li.shape[0], 1)))
        ones_row = eng.solve(buoys, li, lf, FS, weight=np.ones(li.shape[1]))
        ones = eng.solve(buoys, li, lf, FS, weight=np.ones(li.shape, np.float32))
        none = eng.solve(buoys, li, lf, FS)
        with pytest.raises(ValueError, match="lag_frac"):
            eng.solve(buoys, li, lf[0], FS)
    _assert_exact(a, b, "one row against the tiled array")
    _assert_exact(a, _ref(("row", 5, 65), buoys, pairs, li, lf, np.tile(row, (li.shape[0], 1))), "one row")
    _assert_exact(ones_row, ones, "a row of ones against an array of ones")
    _assert_exact(ones, none, "ones against no weights")
    _assert_exact(none, _ref(("case", 5, 65, 3, False), buoys, pairs, li, lf, None), "no weights")


# -- custom pair lists --------------------------------------------------------------------------------------------------------
CUSTOM5 = np.array([[0, 1], [0, 1], [2, 2], [4, 0], [3, 1], [0, 2], [0, 3], [0, 4]], np.int32)   # a repeat, (i, i), reversed, a star


def _custom64():
    p = np.random.default_rng(64).integers(0, 64, (200, 2)).astype(np.int32)
    p[0], p[1], p[199] = (63, 0), (5, 63), (63, 62)
    return p


def _custom_case(name):
    if name == "b5":
        buoys, tx, *_ = _case(5, 65, 3)
        pairs = CUSTOM5
    else:
        buoys, tx, *_ = _case(64, 6, 5)
        pairs = _custom64()
    li, lf = _lags_for(buoys, tx, pairs, 3.0, seed=77)
    return buoys, pairs, li, lf, _weights(li.shape)


@pytest.mark.parametrize("name", ["b5", "b64"])
def test_custom_pair_lists(xc, name):
    buoys, pairs, li, lf, wgt = _custom_case(name)
    assert pairs.max() == len(buoys) - 1
    ref = _ref(("custom", name), buoys, pairs, li, lf, wgt)
    perm = np.random.default_rng(9).permutation(li.shape[0])
    with _engine(xc) as eng:
        got = eng.solve(buoys, li, lf, FS, weight=wgt, pairs=pairs)
        swapped = eng.solve(buoys, -li, -lf, FS, weight=wgt, pairs=np.ascontiguousarray(pairs[:, ::-1]))
        permuted = eng.solve(buoys, li[perm], lf[perm], FS, weight=wgt[perm], pairs=pairs)
    _assert_exact(got, ref, "custom list " + name)
    _assert_exact(swapped, got, "every pair swapped and every lag negated, GPU against GPU")
    _assert_exact(permuted, [a[perm] for a in got], "windows permuted, GPU against GPU")


def test_swap_and_permutation_on_all_pairs(xc):
    buoys, tx, pairs, li, lf = _case(8, 64, 10)
    wgt = _weights(li.shape)
    perm = np.random.default_rng(10).permutation(li.shape[0])
    with _engine(xc) as eng:
        got = eng.solve(buoys, li, lf, FS, weight=wgt)
        swapped = eng.solve(buoys, -li, -lf, FS, weight=wgt, pairs=np.ascontiguousarray(pairs[:, ::-1]))
        permuted = eng.solve(buoys, li[perm], lf[perm], FS, weight=wgt[perm])
        listed = eng.solve(buoys, li, lf, FS, weight=wgt, pairs=pairs)
    _assert_exact(swapped, got, "swapped")
    _assert_exact(permuted, [a[perm] for a in got], "permuted")
    _assert_exact(listed, got, "pairs == NULL against the same list given")


# -- max_iter -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 7, 200])
def test_max_iter(xc, k):
    buoys, tx, pairs, li, lf = _case(4, 130, 5)
    wgt = _weights(li.shape)
    ref60 = _ref(("case", 4, 130, 5, True), buoys, pairs, li, lf, wgt)
    ref = _ref(("max_iter", k), buoys, pairs, li, lf, wgt, max_iter=k)
    with _engine(xc) as eng:
        got = eng.solve(buoys, li, lf, FS, weight=wgt, max_iter=k)
    _assert_exact(got, ref, "max_iter %d" % k)
    if k < 60:
        assert np.array_equal(got[2], np.minimum(ref60[2], k))
    else:
        capped = ref60[2] == 60
        assert capped.any() and (got[2][capped] > 60).any()       # the windows on the cap of 60 move on


# -- degenerate and unphysical inputs ---------------------------------------------------------------------------------------------
def _degenerate(name):
    """(buoys, pairs, lag_int, lag_frac, weight or None, pinned: None or (iters, pos, cost or None))"""
    if name in ("zero_weights", "some_zero_weights"):
        buoys, tx, pairs, li, lf = _case(5, 65, 3)
        if name == "zero_weights":
            c = np.zeros(3)
            for b in buoys:
                c = c + b
            return buoys, pairs, li, lf, np.zeros(li.shape, np.float32), (25, c / 5, 0.0)
        wgt = _weights(li.shape)
        wgt[np.random.default_rng(4).random(li.shape) < 0.4] = 0.0
        wgt[7] = 0.0                                   # one window with nothing to go on among windows that have
        wgt[11, 1:] = 0.0                              # and one with a single measurement: a rank-1 normal matrix
        return buoys, pairs, li, lf, wgt, None
    if name in ("centroid_on_a_buoy", "collinear"):
        ks, on = ((1, 0, -1), 1) if name == "centroid_on_a_buoy" else ((-3, -1, 0.5, 2, 4), 2)
        buoys = kr.line_of_buoys(ks)
        pairs = kr.all_pairs(len(ks))
        li, lf = kr.seeded_lags(70, len(pairs), seed=5)
        return buoys, pairs, li, lf, None, (25, buoys[on], None)
    assert name == "unphysical_lags"                  # no position has these lags: a chaotic walk, the same bits
    buoys, tx, pairs, li, lf = _case(5, 65, 3)
    li, lf = kr.seeded_lags(70, len(pairs), seed=6, span=4_000_000)
    return buoys, pairs, li, lf, _weights(li.shape), None


@pytest.mark.parametrize("name", ["zero_weights", "centroid_on_a_buoy", "collinear", "some_zero_weights", "unphysical_lags"])
def test_degenerate_inputs_stay_finite_and_exact(xc, name):
    buoys, pairs, li, lf, wgt, pinned = _degenerate(name)
    ref = _ref(("degenerate", name), buoys, pairs, li, lf, wgt)
    with _engine(xc) as eng:
        pos, cost, it = got = eng.solve(buoys, li, lf, FS, weight=wgt)
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(cost))
    if pinned is not None:
        n, p, c = pinned
        assert np.all(it == n) and np.all(pos == p) and (c is None or np.all(cost == c))
    _assert_exact(got, ref, name)


# -- pointer flags through the raw ABI --------------------------------------------------------------------------------------------
def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _tp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "no_weights"])
def test_pointer_flags_through_the_raw_abi(xc, weighted):
    """RMX_IN_DEVICE and RMX_OUT_DEVICE, alone and together (XcorrEngine.solve only ever passes 0): the same bits"""
    import torch
    buoys, tx, pairs, li, lf, _ = scenario(8, 130, seed=18, noise_m=10.0)
    wgt = _weights(li.shape) if weighted else None
    W, P = li.shape
    ref = _ref(("flags", weighted), buoys, pairs, li, lf, wgt)
    lib = xc.load_library()
    dev = torch.device("cuda", 0)
    ins_d = [torch.from_numpy(li).to(dev), torch.from_numpy(lf).to(dev), None if wgt is None else torch.from_numpy(wgt).to(dev)]
    got = {}
    with _engine(xc) as eng:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        for flags in (0, xc.RMX_IN_DEVICE, xc.RMX_OUT_DEVICE, xc.RMX_IN_DEVICE | xc.RMX_OUT_DEVICE):
            ins = [_tp(t) for t in ins_d] if flags & xc.RMX_IN_DEVICE else [_vp(li), _vp(lf), _vp(wgt)]
            if flags & xc.RMX_OUT_DEVICE:
                o = [torch.full((W, 3), -77.0, dtype=torch.float64, device=dev),
                     torch.full((W,), -77.0, dtype=torch.float64, device=dev),
                     torch.full((W,), -77, dtype=torch.int32, device=dev)]
                outs = [_tp(t) for t in o]
            else:
                o = [np.full((W, 3), -77.0), np.full(W, -77.0), np.full(W, -77, np.int32)]
                outs = [_vp(a) for a in o]
            torch.cuda.synchronize()
            rc = lib.rmx_solve_batch(eng._ctx, _vp(buoys), 8, None, P, *ins, FS, W, 60, *outs, flags)
            assert rc == 0, (flags, lib.rmx_last_error(eng._ctx))
            assert lib.rmx_synchronize(eng._ctx) == 0
            got[flags] = [t.cpu().numpy() if flags & xc.RMX_OUT_DEVICE else t for t in o]
    for flags in (0, 1, 2, 3):
        _assert_exact(got[flags], ref, "flags %d" % flags)


def test_correlate_to_solve_chain_on_the_device(xc):
    """the chain of the header: rmx_xcorr_batch with RMX_OUT_DEVICE, then rmx_solve_batch with RMX_IN_DEVICE on the same ctx,
    no host round trip between them, against the host path on the same IQ (the shapes of test_gpu_iq_to_position_chain)"""
    import torch
    B, W, N = 5, 24, 4096
    buoys, tx, pairs, _, _, _ = scenario(B, W, seed=31, fs=FS)
    dist = np.linalg.norm(tx[:, None, :] - buoys[None, :, :], axis=2)
    delays = (dist - dist.mean(axis=1, keepdims=True)) / sr.SPEED_OF_LIGHT * FS
    iq, _ = rm.synth.make_windows(W, B, N, FS, seed=32, snr_db=20.0, delays=delays)
    iq = np.ascontiguousarray(iq, dtype=np.complex64)
    P = len(pairs)
    lib = xc.load_library()
    dev = torch.device("cuda", 0)
    with xc.XcorrEngine(B, N, W) as eng:
        li, lf, pk = eng.correlate(iq)
        host = eng.solve(buoys, li, lf, FS)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        lag_d = torch.full((W, P), -77, dtype=torch.int32, device=dev)
        frac_d = torch.full((W, P), -77.0, dtype=torch.float32, device=dev)
        peak_d = torch.full((W, P), -77.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        pos, cost, it = np.full((W, 3), -77.0), np.full(W, -77.0), np.full(W, -77, np.int32)
        rc = lib.rmx_xcorr_batch(eng._ctx, _vp(iq), W, None, 0, _tp(lag_d), _tp(frac_d), _tp(peak_d), xc.RMX_OUT_DEVICE)
        assert rc == 0, lib.rmx_last_error(eng._ctx)
        rc = lib.rmx_solve_batch(eng._ctx, _vp(buoys), B, None, 0, _tp(lag_d), _tp(frac_d), None, FS, W, 60,
                                 _vp(pos), _vp(cost), _vp(it), xc.RMX_IN_DEVICE)
        assert rc == 0, lib.rmx_last_error(eng._ctx)
        assert lib.rmx_synchronize(eng._ctx) == 0
    assert np.array_equal(lag_d.cpu().numpy(), li) and np.array_equal(frac_d.cpu().numpy(), lf)
    _assert_exact((pos, cost, it), host, "device chain against the host path")
    _assert_exact(host, _ref("chain", buoys, pairs, li, lf, None), "host path")


# -- one ctx, many calls ------------------------------------------------------------------------------------------------------------
def test_one_ctx_through_growing_and_shrinking_calls(xc):
    """sv_in / sv_out / sv_pairs grow, are reused by smaller calls and by a custom list, with a correlation and a refused
    solve between: every result is a fresh engine's and the restatement's"""
    steps = []
    for B, W, noise_m in [(5, 3, 3), (16, 130, 5), (3, 1, 0)]:
        buoys, tx, pairs, li, lf, _ = scenario(B, W, seed=40 + B, noise_m=float(noise_m))
        steps.append((("ctx", B, W), buoys, None, pairs, li, lf, _weights(li.shape)))
    buoys, pairs, li, lf, wgt = _custom_case("b64")
    steps.append((("custom", "b64"), buoys, pairs, pairs, li, lf, wgt))
    steps.append(steps[1])
    iq, _ = rm.synth.make_windows(2, 3, 256, FS, seed=3, max_delay=20)
    lib = xc.load_library()
    with _engine(xc) as eng:
        first = eng.correlate(iq)
        for n, (key, buoys, given, pairs, li, lf, wgt) in enumerate(steps):
            got = eng.solve(buoys, li, lf, FS, weight=wgt, pairs=given)
            with _engine(xc) as fresh:
                alone = fresh.solve(buoys, li, lf, FS, weight=wgt, pairs=given)
            _assert_exact(got, alone, "step %d against a fresh engine" % n)
            _assert_exact(got, _ref(key, buoys, pairs, li, lf, wgt), "step %d" % n)
            if n == 1:
                again = eng.correlate(iq)
                assert all(np.array_equal(a, b) for a, b in zip(first, again))
            if n == 2:
                o = [np.full((1, 3), -77.0), np.full(1, -77.0), np.full(1, -77, np.int32)]
                rc = lib.rmx_solve_batch(eng._ctx, _vp(buoys), 65, None, 0, _vp(li), _vp(lf), None, FS, 1, 60, *map(_vp, o), 0)
                assert rc == RMX_E_INVAL and np.all(o[0] == -77.0) and np.all(o[2] == -77)


# -- refusals through the raw ABI ---------------------------------------------------------------------------------------------------
def _refusals():
    B, W, P = 5, 3, 10
    bad_lo, bad_hi = kr.all_pairs(B), kr.all_pairs(B)
    bad_lo[4, 1], bad_hi[9, 0] = -1, B
    many = np.zeros((2017, 2), np.int32)
    many[:, 1] = 1
    big = dict(li=np.zeros((W, 2017), np.int32), lf=np.zeros((W, 2017), np.float32), wgt=None)
    out = {
        "n_buoys 1": dict(n_buoys=1, n_pairs=0), "n_buoys 65": dict(n_buoys=65, n_pairs=0),
        "fs 0": dict(fs=0.0), "fs -1": dict(fs=-1.0), "fs NaN": dict(fs=float("nan")),
        "max_iter 0": dict(max_iter=0), "n_windows -1": dict(n_windows=-1),
        "pair index -1": dict(pairs=bad_lo), "pair index n_buoys": dict(pairs=bad_hi),
        "no list, n_pairs 7": dict(n_pairs=7), "no list, n_pairs 11": dict(n_pairs=11),
        "2017 pairs": dict(pairs=many, n_pairs=2017, **big), "a list of 0 pairs": dict(pairs=kr.all_pairs(B), n_pairs=0),
    }
    for name in ("buoys", "li", "lf", "pos", "cost", "iters"):
        out["NULL " + name] = {name: None}
    return out


@pytest.mark.parametrize("name", sorted(_refusals()))
def test_refusals_leave_the_outputs_alone_and_the_ctx_usable(xc, name):
    B, W, P = 5, 3, 10
    buoys, tx, pairs, li, lf, _ = scenario(B, W, seed=45, noise_m=3.0)
    wgt = _weights(li.shape)
    ref = _ref(("ctx", B, W), buoys, pairs, li, lf, wgt)
    lib = xc.load_library()

    def call(eng, o, **kw):
        a = dict(buoys=buoys, n_buoys=B, pairs=None, n_pairs=P, li=li, lf=lf, wgt=wgt, fs=FS, n_windows=W, max_iter=60,
                 pos=o[0], cost=o[1], iters=o[2])
        a.update(kw)
        return lib.rmx_solve_batch(eng._ctx, _vp(a["buoys"]), a["n_buoys"], _vp(a["pairs"]), a["n_pairs"], _vp(a["li"]),
                                   _vp(a["lf"]), _vp(a["wgt"]), a["fs"], a["n_windows"], a["max_iter"], _vp(a["pos"]),
                                   _vp(a["cost"]), _vp(a["iters"]), 0)

    with _engine(xc) as eng:
        o = [np.full((W, 3), -77.0), np.full(W, -77.0), np.full(W, -77, np.int32)]
        assert call(eng, o, **_refusals()[name]) == RMX_E_INVAL
        assert len(lib.rmx_last_error(eng._ctx) or b"") > 0
        assert np.all(o[0] == -77.0) and np.all(o[1] == -77.0) and np.all(o[2] == -77)
        assert call(eng, o) == 0
        _assert_exact(o, ref, "the valid call after the refusal: " + name)


def test_no_windows_is_ok_and_writes_nothing(xc):
    buoys, tx, pairs, li, lf, _ = scenario(5, 3, seed=45, noise_m=3.0)
    lib = xc.load_library()
    o = [np.full((3, 3), -77.0), np.full(3, -77.0), np.full(3, -77, np.int32)]
    with _engine(xc) as eng:
        rc = lib.rmx_solve_batch(eng._ctx, _vp(buoys), 5, None, 10, _vp(li), _vp(lf), None, FS, 0, 60, *map(_vp, o), 0)
        assert rc == 0
        assert lib.rmx_synchronize(eng._ctx) == 0
        assert np.all(o[0] == -77.0) and np.all(o[1] == -77.0) and np.all(o[2] == -77)
        pos, cost, it = eng.solve(buoys, li[:0], lf[:0], FS)
        assert pos.shape == (0, 3) and cost.shape == (0,) and it.shape == (0,)
