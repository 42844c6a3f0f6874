"""rmx_xcorr_batch_refined on the GPU: the fine lag search against the float64 restatement (tests/refined_ref.py) on every
spectrum layout (g_fwd_small, k_fwd, the four-step rows), through every door (uint8, device pointers, custom pairs), across
chunk boundaries, composed with band / PHAT / bounds / integration / a dead receiver, its identities (refine = 0, repeats,
nothing left behind for the next call) and the accuracy it exists for."""
import ctypes as C

import numpy as np
import pytest

import integrated_ref as ir
import radio_mapper_amd as rm
import refined_ref as rr

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def xc():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    if xcorr.device_count() < 1:
        pytest.fail("no GPU visible")
    return xcorr


@pytest.fixture
def opts(xc):
    xc.clear_default_options()
    yield xc.set_default_option
    xc.clear_default_options()


def _scene(W, B, N, seed=7, **kw):
    return rm.synth.make_windows(W, B, N, 10e6, seed=seed, snr_db=10, bandwidth=0.8, max_delay=min(40, N / 8), **kw)


def _full(N, P):
    return np.tile(np.array([[-(N - 1), N - 1]], np.int64), (P, 1))


def _assert_refined(got, ref, N, lag_bounds=None, what="", dead_ok=False):
    """the parity rule of rmx_xcorr_batch_refined (include/rmx.h).  The reference's coarse top-two margin must exceed 1e-5 on
    every pair-window -- asserted first, so no case is excused; dead_ok: except where the reference's peak is exactly 0 (a
    dead receiver: both sides then give the slice's start, 0, 0)."""
    li, lf, pk = got
    ri, rf, rp, mg, fm, fb = ref
    dead = (rp == 0) if dead_ok else np.zeros(rp.shape, bool)
    assert np.all((mg > TOL) | dead), (what, float(mg.min()))
    assert np.all(np.isfinite(lf)) and np.all(np.isfinite(pk))
    lag, want = li + lf.astype(np.float64), ri + rf
    rel = np.abs(lag - want) / np.maximum(np.abs(want), 1.0)
    worst = int(np.argmax(rel))
    print("%s: worst |dlag| / max(|lag|, 1) = %.3e (flat-peak bound there %.3e), worst peak deviation %.3e relative"
          % (what, rel.max(), fb.ravel()[worst], float(np.max(np.abs(pk - rp) / np.maximum(rp, 1e-30) * (rp > 0)))))
    assert np.all((rel <= TOL) | (rel <= fb)), (what, float(rel.max()), float(fb.ravel()[worst]))
    assert np.all(np.abs(pk - rp) <= 1e-5 * rp + 1e-6 * fm), what
    lb = _full(N, li.shape[1]) if lag_bounds is None else np.asarray(lag_bounds)
    assert np.all(li >= lb[..., 0]) and np.all(li <= lb[..., 1]), what
    assert np.all(np.abs(lf) <= 0.5), what
    if dead_ok:
        assert np.array_equal(li[dead], ri[dead]) and np.all(lf[dead] == 0) and np.all(pk[dead] == 0)


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


# -- parity against the float64 restatement, one shape per spectrum layout ----------------------------------------------
# (N, buoys, windows, U, forward family)
PARITY = [(256, 3, 4, 8, "g_fwd_small"), (256, 3, 4, 2, "g_fwd_small"), (256, 3, 4, 16, "g_fwd_small"),
          (4096, 3, 2, 8, "k_fwd"), (4096, 8, 1, 8, "k_fwd"), (8192, 3, 2, 8, "g_rows_fwd")]


@pytest.mark.parametrize("N,B,W,U,fwd", PARITY, ids=["N%d-B%d-W%d-U%d" % p[:4] for p in PARITY])
def test_parity_on_every_layout(xc, opts, N, B, W, U, fwd):
    iq, _ = _scene(W, B, N)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        got = eng.correlate(iq, refine=U)
        tk = eng.last_timing_by_kernel()
    assert fwd in tk and tk["k_refine"]["launches"] == 1, tk
    assert not set(tk) & {"g_win_*", "g_rows_fused", "k16_fwd", "k16_pairs"}, tk
    _assert_refined(got, rr.refined_batch(iq, U), N, what="N = %d, B = %d, W = %d, U = %d" % (N, B, W, U))


# -- the same numbers through every door ---------------------------------------------------------------------------------
def test_uint8_device_pointers_and_custom_pairs(xc):
    torch = pytest.importorskip("torch")
    N, B, W, U = 4096, 3, 2, 8
    iq, _, raw = _scene(W, B, N, return_u8=True)
    with xc.XcorrEngine(B, N, W) as eng:
        host = eng.correlate(iq, refine=U)
        assert _same(host, eng.correlate(raw, refine=U))
        d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
        out = [torch.zeros((W, 3), dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.float32)]
        torch.cuda.synchronize()
        eng.correlate_device(d_iq.data_ptr(), W, *[o.data_ptr() for o in out], refine=U)
        eng.synchronize()
        assert _same(host, [o.cpu().numpy() for o in out])
        pairs = [(2, 0), (1, 2)]
        got = eng.correlate(iq, np.array(pairs, np.int32), refine=U)
    _assert_refined(got, rr.refined_batch(iq, U, pairs=pairs), N, what="custom pairs")


# -- chunk boundaries: k_refine runs before the next chunk's forward kernels overwrite the spectra ----------------------
@pytest.mark.parametrize("W,chunk,launches", [(6, 2, 1), (20, 8, 3)])
def test_chunks_of_the_k_fwd_path(xc, W, chunk, launches):
    """(the option is rounded up to 8 windows and capped at the batch: 6 windows stay one chunk, 20 make three)"""
    N, B, U = 4096, 3, 8
    iq, _ = _scene(W, B, N, seed=3)
    with xc.XcorrEngine(B, N, W) as eng:
        whole = eng.correlate(iq, refine=U)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("chunk_windows", chunk)
        eng.set_option("timing", 1)
        parts = eng.correlate(iq, refine=U)
        assert eng.last_timing_by_kernel()["k_refine"]["launches"] == launches
    assert _same(whole, parts)
    if launches > 1:   # the last chunk's rows against the restatement: its spectra were the last ones written
        _assert_refined([a[-2:] for a in parts], rr.refined_batch(iq[-2:], U), N, what="last chunk")


@pytest.mark.parametrize("N", [1024, 8192])
def test_chunks_of_the_generic_paths(xc, opts, N):
    B, W, U = 3, 6, 8
    iq, _ = _scene(W, B, N, seed=4)
    with xc.XcorrEngine(B, N, W) as eng:
        whole = eng.correlate(iq, refine=U)
    opts("gen_chunk", 2)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        parts = eng.correlate(iq, refine=U)
        assert eng.last_timing_by_kernel()["k_refine"]["launches"] == 3
    assert _same(whole, parts)


# -- composition ------------------------------------------------------------------------------------------------------------
def test_band_phat_and_bounds(xc):
    N, B, W, U = 4096, 3, 2, 8
    iq, _ = _scene(W, B, N, seed=5)
    lb = np.array([[-85, 85], [-90, 100], [-120, 95]], np.int32)
    with xc.XcorrEngine(B, N, W) as eng:
        got = eng.correlate(iq, band=(-0.25, 0.25), whiten=True, lag_bounds=lb, refine=U)
    _assert_refined(got, rr.refined_batch(iq, U, band=(-0.25, 0.25), phat=True, lag_bounds=lb), N, lb, "band + PHAT + bounds")


@pytest.mark.parametrize("N", [256, 4096])
def test_lag0_on_either_edge_of_its_bounds(xc, N):
    B, W, U = 3, 3, 8
    iq, _ = _scene(W, B, N, seed=6)
    lag0 = rr.refined_batch(iq, U, detail=True)[-1]["lag0"]
    lb = np.stack([lag0, lag0], axis=-1).astype(np.int32)     # [W][P][2]
    lb[:, 0, 1] += 5                                          # pair (0,1): lag0 == lo
    lb[:, 1, 0] -= 5                                          # pair (0,2): lag0 == hi
    lb[:, 2] = (-(N - 1), N - 1)
    ref = rr.refined_batch(iq, U, lag_bounds=lb, detail=True)
    assert np.array_equal(ref[-1]["lag0"], lag0)
    with xc.XcorrEngine(B, N, W) as eng:
        got = eng.correlate(iq, lag_bounds=lb, refine=U)
    _assert_refined(got, ref[:6], N, lb, "lag0 on lo / hi")
    lag = got[0] + got[1].astype(np.float64)
    assert np.all(lag[:, 0] >= lag0[:, 0]) and np.all(lag[:, 1] <= lag0[:, 1])


def test_integrated_groups(xc):
    N, K, U = 1024, 4, 8
    iq = ir.segments(ir.offset_scene(8 * N, 3, 3.0, cycles=(0, 1, 3)), 8)   # [8][3][1024]: two groups of four windows
    with xc.XcorrEngine(3, N, 8) as eng:
        got = eng.correlate(iq, integrate=K, refine=U)
        again = eng.correlate(iq, integrate=K, refine=U)
    assert _same(got, again)
    assert got[0].shape == (2, 3)
    _assert_refined(got, rr.refined_batch(iq, U, integrate=K), N, what="integrate = 4")
    assert np.all(np.abs(got[0] + got[1] - ir.TRUE_LAGS) < 0.5)


@pytest.mark.parametrize("N,whiten", [(256, False), (4096, True)])
def test_a_dead_receiver(xc, N, whiten):
    B, W, U = 3, 2, 8
    iq, _ = _scene(W, B, N, seed=9)
    iq[:, 1] = 0
    lb = np.array([[-(N - 1), N - 1], [-100, 100], [-5, 9]], np.int32)
    with xc.XcorrEngine(B, N, W) as eng:
        for bounds in (None, lb):
            got = eng.correlate(iq, whiten=whiten, lag_bounds=bounds, refine=U)
            _assert_refined(got, rr.refined_batch(iq, U, phat=whiten, lag_bounds=bounds), N, bounds, "dead receiver", dead_ok=True)
            assert np.all(got[2][:, [0, 2]] == 0) and np.all(got[2][:, 1] > 0)


# -- identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [256, 4096, 8192])
def test_refine_0_is_the_unrefined_call_and_repeats_are_identical(xc, N):
    B, W = 3, 4
    iq, _ = _scene(W, B, N, seed=8)
    lb = np.array([[-30, 30], [-40, 35], [-(N - 1), N - 1]], np.int32)
    with xc.XcorrEngine(B, N, W) as eng:
        for kw in ({}, {"lag_bounds": lb}, {"band": (-0.3, 0.2), "whiten": True}, {"integrate": 2, "lag_bounds": lb}):
            assert _same(eng.correlate(iq, **kw), eng.correlate(iq, refine=0, **kw)), kw
            a = eng.correlate(iq, refine=4, **kw)
            assert _same(a, eng.correlate(iq, refine=4, **kw)), kw


@pytest.mark.parametrize("N", [256, 4096, 8192])
def test_refusals_in_order_and_nothing_left_behind(xc, N):
    """refine is refused after integrate, the weighting and the bounds, with its value in the text; after a refused and a
    refined call the plain call and the Doppler search return, bit for bit, what a fresh engine returns"""
    B, W, P = 3, 4, 3
    lib = xc.load_library()
    iq, _ = _scene(W, B, N, seed=N)
    dops = np.array([0.0, 1.0 / N])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def raw(eng, K, weighting, bounds, U):
        out = [np.zeros((W, P), t) for t in (np.int32, np.float32, np.float32)]
        rc = lib.rmx_xcorr_batch_refined(eng._ctx, vp(iq), W, None, P, K, None, 0, weighting,
                                         None if bounds is None else vp(bounds), 0, U, *[vp(o) for o in out], 0)
        return rc, lib.rmx_last_error(eng._ctx).decode()

    with xc.XcorrEngine(B, N, W) as fresh:
        want_plain = fresh.correlate(iq)
    with xc.XcorrEngine(B, N, W) as fresh:
        want_caf = fresh.caf(iq, dops)
    bad_lb = np.array([[-3, 3], [7, 6], [-3, 3]], np.int32)
    with xc.XcorrEngine(B, N, W) as eng:
        rc, msg = raw(eng, 3, 7, bad_lb, 3)
        assert rc == -1 and "integrate = 3" in msg, msg
        rc, msg = raw(eng, 2, 7, bad_lb, 3)
        assert rc == -1 and "weighting" in msg, msg
        rc, msg = raw(eng, 2, 1, bad_lb, 3)
        assert rc == -1 and "lag_bounds" in msg and "pair 1" in msg, msg
        for U in (3, 1, 32, -2):
            rc, msg = raw(eng, 2, 1, None, U)
            assert rc == -1 and "refine = %d" % U in msg, msg
        got = eng.correlate(iq, whiten=True, refine=8)
        _assert_refined(got, rr.refined_batch(iq, 8, phat=True), N, what="after the refusals")
        got_plain = eng.correlate(iq)
        got_caf = eng.caf(iq, dops)
    assert _same(got_plain, want_plain)
    assert _same(got_caf, want_caf)


# -- the accuracy the feature exists for, on the device ------------------------------------------------------------------
def test_accuracy_on_the_device(xc):
    """the CPU assertion of tests/test_refined_cpu.py through correlate(): parabola >= 0.04 samples rms, refined <= 0.012"""
    iq, delays = rm.synth.make_windows(16, 3, 1024, 10e6, seed=7, snr_db=10, bandwidth=0.8, max_delay=40)
    true = np.stack([delays[:, j] - delays[:, i] for i, j in ((0, 1), (0, 2), (1, 2))], axis=1)
    with xc.XcorrEngine(3, 1024, 16) as eng:
        ci, cf, _ = eng.correlate(iq)
        li, lf, _ = eng.correlate(iq, refine=8)
    rms_par = float(np.sqrt(np.mean((ci + cf - true) ** 2)))
    lag = li + lf.astype(np.float64)
    rms_ref = float(np.sqrt(np.mean((lag - true) ** 2)))
    closure = np.abs(lag[:, 0] + lag[:, 2] - lag[:, 1])
    print("parabola rms %.4f, refined rms %.4f, closure max %.4f" % (rms_par, rms_ref, closure.max()))
    assert rms_par >= 0.04
    assert rms_ref <= 0.012
    assert np.all(closure <= 0.03)
