"""rmx_xcorr_batch_quality on the GPU: the four figures against the float64 restatement (tests/quality_ref.py) on every
spectrum layout (g_fwd_small, k_fwd, the four-step rows), composed with band / PHAT / bounds / integration / refinement,
across chunk boundaries, on custom pair lists, through host and device pointers, on a dead receiver and on identical
windows; the three lag outputs against the same call without quality, bit for bit; the refusals of the new entry.

Tolerances (include/rmx.h): coherence, rms_bw and n_eff within 1e-4 relative of the restatement; psr compared as
Et / p0^2 = (L - 1) / psr + 1 within 1e-4 relative."""
import ctypes as C

import numpy as np
import pytest

import integrated_ref as ir
import quality_ref as qr
import radio_mapper_amd as rm
import weighted_ref as wr

pytestmark = pytest.mark.gpu
TOL = 1e-4


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


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def _assert_quality(got, ref, N, what=""):
    """got float32 [R][P][4] against the restatement float64 [R][P][4]; prints the worst deviation of each figure first"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got[..., [qr.COHERENCE, qr.RMS_BW, qr.NEFF]])) and not np.any(np.isnan(got)), what
    dev = {}
    for name, k in (("coherence", qr.COHERENCE), ("rms_bw", qr.RMS_BW), ("n_eff", qr.NEFF)):
        zero = ref[..., k] == 0
        assert np.all(got[..., k][zero] == 0), (what, name)
        dev[name] = float(np.max(np.abs(got[..., k] - ref[..., k])[~zero] / ref[..., k][~zero], initial=0.0))
    zero = ref[..., qr.PSR] == 0
    assert np.all(got[..., qr.PSR][zero] == 0), (what, "psr")
    ge, re_ = qr.et_over_p2(got[~zero], N), qr.et_over_p2(ref[~zero], N)      # (psr = +inf gives 1 on either side)
    dev["Et/p0^2"] = float(np.max(np.abs(ge - re_) / re_, initial=0.0))
    print("%s: worst relative deviation %s" % (what, ", ".join("%s %.2e" % kv for kv in dev.items())))
    for name, d in dev.items():
        assert d <= TOL, (what, name, d)
    assert np.all(got[..., qr.COHERENCE] >= 0) and np.all(got[..., qr.COHERENCE] <= 1), what


def _both(eng, iq, pairs=None, **kw):
    """the quality call -> (three lag outputs, quality); test_lag_outputs_equal_the_call_without_quality compares the
    three with the same call without quality, case by case"""
    got = eng.correlate(iq, pairs, quality=True, **kw)
    assert len(got) == 4 and got[3].dtype == np.float32 and got[3].shape == got[0].shape + (4,)
    return got[:3], got[3]


# -- the three lag outputs against the same call without quality, bit for bit, in every case of this file --------------------
def _dead(iq):
    iq[:, 1] = 0
    return iq


def _identical(iq):
    iq[:, 1] = iq[:, 0]
    iq[:, 2] = iq[:, 0]
    return iq


_LB = np.array([[-85, 85], [-90, 100], [-120, 95]], np.int32)
_PAIRS = [(2, 0), (1, 3), (2, 0), (0, 1), (3, 1)]
# (id, N, B, W, seed, keyword arguments, pair list, what is done to the scene, chunk_windows / gen_chunk)
IDENTITY = [
    ("layout-N256", 256, 3, 4, 7, {}, None, None, None),
    ("layout-N4096-B3", 4096, 3, 2, 7, {}, None, None, None),
    ("layout-N4096-B8", 4096, 8, 1, 7, {}, None, None, None),
    ("layout-N8192", 8192, 3, 2, 7, {}, None, None, None),
    ("band-phat-bounds", 4096, 3, 2, 5, dict(band=(-0.25, 0.25), whiten=True, lag_bounds=_LB), None, None, None),
    ("integrate4", 1024, 3, 8, 0, dict(integrate=4), None, "offset", None),
    ("refine8-N256", 256, 3, 2, 6, dict(refine=8), None, None, None),
    ("refine8-N4096", 4096, 3, 2, 6, dict(refine=8), None, None, None),
    ("refine8-N8192", 8192, 3, 2, 6, dict(refine=8), None, None, None),
    ("chunks-N4096", 4096, 3, 5, 4, {}, None, None, ("chunk_windows", 2)),
    ("chunks-N1024", 1024, 3, 5, 4, {}, None, None, ("gen_chunk", 2)),
    ("chunks-N8192", 8192, 3, 5, 4, {}, None, None, ("gen_chunk", 2)),
    ("pairs-N256", 256, 4, 2, 2, {}, _PAIRS, None, None),
    ("pairs-N4096", 4096, 4, 2, 2, {}, _PAIRS, None, None),
    ("dead-N256", 256, 3, 2, 9, {}, None, _dead, None),
    ("dead-N4096-phat", 4096, 3, 2, 9, dict(whiten=True), None, _dead, None),
    ("dead-N4096", 4096, 3, 2, 9, {}, None, _dead, None),
    ("dead-N8192-phat", 8192, 3, 2, 9, dict(whiten=True), None, _dead, None),
    ("identical-N256", 256, 3, 2, 10, {}, None, _identical, None),
    ("identical-N4096", 4096, 3, 2, 10, {}, None, _identical, None),
    ("identical-N8192", 8192, 3, 2, 10, {}, None, _identical, None),
]


@pytest.mark.parametrize("N,B,W,seed,kw,pairs,change,chunk", [c[1:] for c in IDENTITY], ids=[c[0] for c in IDENTITY])
def test_lag_outputs_equal_the_call_without_quality(xc, opts, N, B, W, seed, kw, pairs, change, chunk):
    """In every case of this file the three lag outputs equal those of the same call without quality, bit for bit; the
    count of differing slots is printed first.  The cases without a band, weighting, integration or refinement at L <= 4096
    and at most 4 buoys (layout-N256, chunks-N1024, pairs-N256, dead-N256, identical-N256) are those whose call without
    quality takes g_win_fused, a different transform from the per-transform kernels: there the quality call runs that
    kernel too and computes the figures in a second pass (on a device, before that: 10 of 12 lag_frac and 3 of 12 peak
    differed in layout-N256)."""
    if change == "offset":
        iq = ir.segments(ir.offset_scene(W * N, 3, 3.0, cycles=(0, 1, 3)), W)
    else:
        iq, _ = _scene(W, B, N, seed=seed)
        if change is not None:
            iq = change(iq)
    pl = None if pairs is None else np.array(pairs, np.int32)
    if chunk is not None and chunk[0] == "gen_chunk":
        opts(*chunk)
    with xc.XcorrEngine(B, N, W) as eng:
        if chunk is not None and chunk[0] == "chunk_windows":
            eng.set_option(*chunk)
        got = eng.correlate(iq, pl, quality=True, **kw)
        plain = eng.correlate(iq, pl, **kw)
    assert len(got) == 4 and len(plain) == 3
    diff = [int(np.count_nonzero(u != v)) for u, v in zip(got[:3], plain)]
    print("%d slots; differing lag_int / lag_frac / peak: %s" % (plain[0].size, diff))
    assert diff == [0, 0, 0]


# -- parity against the float64 restatement, one shape per spectrum layout ----------------------------------------------
# (N, buoys, windows, forward family)
LAYOUTS = [(256, 3, 4, "g_fwd_small"), (4096, 3, 2, "k_fwd"), (4096, 8, 1, "k_fwd"), (8192, 3, 2, "g_rows_fwd")]


@pytest.mark.parametrize("N,B,W,fwd", LAYOUTS, ids=["N%d-B%d-W%d" % p[:3] for p in LAYOUTS])
def test_parity_on_every_layout(xc, opts, N, B, W, fwd):
    iq, _ = _scene(W, B, N)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        got = eng.correlate(iq, quality=True)
        tk = eng.last_timing_by_kernel()
        assert fwd in tk and tk["k_quality"]["launches"] == 1 and "k_refine" not in tk, tk
        lags, q = _both(eng, iq)
    assert _same(got[:3], lags) and np.array_equal(got[3], q)
    _assert_quality(q, qr.quality_batch(iq), N, "N = %d, B = %d, W = %d" % (N, B, W))


# -- composition ------------------------------------------------------------------------------------------------------------
def test_band_phat_and_bounds(xc):
    N, B, W = 4096, 3, 2
    iq, _ = _scene(W, B, N, seed=5)
    lb = np.array([[-85, 85], [-90, 100], [-120, 95]], np.int32)
    kw = dict(band=(-0.25, 0.25), whiten=True, lag_bounds=lb)
    with xc.XcorrEngine(B, N, W) as eng:
        _, q = _both(eng, iq, **kw)
    _assert_quality(q, qr.quality_batch(iq, band=(-0.25, 0.25), phat=True, lag_bounds=lb), N, "band + PHAT + bounds")
    kept = wr.mask(-0.25, 0.25, N).sum()     # n_eff under PHAT: the kept bins
    assert np.all(np.abs(q[..., qr.NEFF] / kept - 1.0) <= TOL)


def test_integrated_groups(xc):
    N, K = 1024, 4
    iq = ir.segments(ir.offset_scene(8 * N, 3, 3.0, cycles=(0, 1, 3)), 8)   # [8][3][1024]: two groups of four windows
    with xc.XcorrEngine(3, N, 8) as eng:
        lags, q = _both(eng, iq, integrate=K)
    assert lags[0].shape == (2, 3) and q.shape == (2, 3, 4)
    _assert_quality(q, qr.quality_batch(iq, integrate=K), N, "integrate = 4")


@pytest.mark.parametrize("N", [256, 4096, 8192])
def test_refine_with_quality_keeps_the_coarse_peak(xc, N):
    B, W, U = 3, 2, 8
    iq, _ = _scene(W, B, N, seed=6)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        lags, q = _both(eng, iq, refine=U)
        tk = eng.last_timing_by_kernel()
        assert tk["k_quality"]["launches"] == 1 and tk["k_refine"]["launches"] == 1, tk
        assert not set(tk) & {"g_win_*", "g_rows_fused", "k16_fwd", "k16_pairs"}, tk
        other = eng.correlate(iq, refine=2, quality=True)
    assert np.array_equal(q, other[3])                # quality reads the coarse peak, whatever k_refine writes afterwards
    assert not np.array_equal(lags[2], other[2])      # (the refined peaks of U = 8 and U = 2 differ)
    _assert_quality(q, qr.quality_batch(iq), N, "refine = 8, N = %d" % N)


# -- chunk boundaries and pair lists -------------------------------------------------------------------------------------
def test_chunks_of_the_k_fwd_path(xc):
    """(the option is rounded up to 8 windows and capped at the batch: 20 windows make three chunks)"""
    N, B, W = 4096, 3, 20
    iq, _ = _scene(W, B, N, seed=3)
    with xc.XcorrEngine(B, N, W) as eng:
        whole = eng.correlate(iq, quality=True)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("chunk_windows", 8)
        eng.set_option("timing", 1)
        parts = eng.correlate(iq, quality=True)
        assert eng.last_timing_by_kernel()["k_quality"]["launches"] == 3
    assert _same(whole, parts)
    _assert_quality(parts[3][-2:], qr.quality_batch(iq[-2:]), N, "last chunk")


def test_five_windows_in_chunks_of_two(xc):
    N, B, W = 4096, 3, 5
    iq, _ = _scene(W, B, N, seed=4)
    with xc.XcorrEngine(B, N, W) as eng:
        whole = eng.correlate(iq, quality=True)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("chunk_windows", 2)
        parts = eng.correlate(iq, quality=True)
    assert _same(whole, parts)
    _assert_quality(parts[3], qr.quality_batch(iq), N, "W = 5, chunk_windows = 2")


@pytest.mark.parametrize("N", [1024, 8192])
def test_chunks_of_the_generic_paths(xc, opts, N):
    B, W = 3, 5
    iq, _ = _scene(W, B, N, seed=4)
    with xc.XcorrEngine(B, N, W) as eng:
        whole = eng.correlate(iq, quality=True)
    opts("gen_chunk", 2)
    with xc.XcorrEngine(B, N, W) as eng:
        eng.set_option("timing", 1)
        parts = eng.correlate(iq, quality=True)
        assert eng.last_timing_by_kernel()["k_quality"]["launches"] == 3
    assert _same(whole, parts)
    _assert_quality(parts[3], qr.quality_batch(iq), N, "gen_chunk = 2, N = %d" % N)


@pytest.mark.parametrize("N", [256, 4096])
def test_custom_partly_repeated_pairs(xc, N):
    B, W = 4, 2
    iq, _ = _scene(W, B, N, seed=2)
    pairs = [(2, 0), (1, 3), (2, 0), (0, 1), (3, 1)]
    with xc.XcorrEngine(B, N, W) as eng:
        _, q = _both(eng, iq, np.array(pairs, np.int32))
    _assert_quality(q, qr.quality_batch(iq, pairs=pairs), N, "custom pairs, N = %d" % N)
    assert np.array_equal(q[:, 0], q[:, 2])
    assert np.array_equal(q[:, 1, [qr.RMS_BW, qr.NEFF]], q[:, 4, [qr.RMS_BW, qr.NEFF]])     # (i, j) and (j, i): the same magnitudes


# -- pointer forms and determinism ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,U", [(256, 1, 4), (4096, 1, 4), (1024, 2, 4), (256, 1, 0), (4096, 1, 0), (8192, 1, 0)])
def test_host_and_device_pointers_and_repeats(xc, N, K, U):
    """(U = 0, K = 1: nothing but quality is asked for, the figures come from the second pass)"""
    torch = pytest.importorskip("torch")
    B, W, P = 3, 4, 3
    iq, _, raw = _scene(W, B, N, return_u8=True)
    with xc.XcorrEngine(B, N, W) as eng:
        host = eng.correlate(iq, integrate=K, refine=U, quality=True)
        assert _same(host, eng.correlate(iq, integrate=K, refine=U, quality=True))         # two identical calls
        assert _same(host, eng.correlate(raw, integrate=K, refine=U, quality=True))
        d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
        out = [torch.zeros((W // K, P), dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.float32)]
        d_q = torch.full((W // K, P, 4), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.correlate_device(d_iq.data_ptr(), W, *[o.data_ptr() for o in out], integrate=K, refine=U, quality_ptr=d_q.data_ptr())
        eng.synchronize()
        assert _same(host, [o.cpu().numpy() for o in out] + [d_q.cpu().numpy()])
        d_q.fill_(-1.0)
        torch.cuda.synchronize()
        eng.correlate_device(d_iq.data_ptr(), W, *[o.data_ptr() for o in out], integrate=K, refine=U)   # quality_ptr = 0
        eng.synchronize()
        assert _same(host[:3], [o.cpu().numpy() for o in out]) and bool((d_q == -1.0).all())


# -- edge inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,whiten", [(256, False), (4096, True), (4096, False), (8192, True)])
def test_a_dead_receiver(xc, N, whiten):
    B, W = 3, 2
    iq, _ = _scene(W, B, N, seed=9)
    iq[:, 1] = 0
    with xc.XcorrEngine(B, N, W) as eng:
        _, q = _both(eng, iq, whiten=whiten)
    assert not np.any(np.isnan(q))
    assert np.all(q[:, [0, 2]] == 0) and np.all(q[:, 1] > 0)
    _assert_quality(q, qr.quality_batch(iq, phat=whiten), N, "dead receiver, N = %d" % N)


@pytest.mark.parametrize("N", [256, 4096, 8192])
def test_identical_windows(xc, N):
    B, W = 3, 2
    iq, _ = _scene(W, B, N, seed=10)
    iq[:, 1] = iq[:, 0]
    iq[:, 2] = iq[:, 0]
    with xc.XcorrEngine(B, N, W) as eng:
        lags, q = _both(eng, iq)
        q2 = eng.correlate(iq, integrate=2, quality=True)[3]
    assert np.all(lags[0] == 0)
    assert np.all(np.abs(q[..., qr.COHERENCE] - 1.0) <= 1e-5), q[..., qr.COHERENCE]
    assert np.all(np.abs(q2[..., qr.COHERENCE] - 1.0) <= 1e-5), q2[..., qr.COHERENCE]


# -- the raw entry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [256, 4096])
def test_null_quality_is_the_refined_entry_and_bad_arguments_are_refused(xc, N):
    """quality == NULL through the new entry equals the refined entry bit for bit; the refusals come in the refined entry's
    order (integrate, weighting, lag_bounds, refine) and then the new one, each RMX_E_INVAL with text; after them a plain
    call returns what a fresh engine returns"""
    B, W, P = 3, 4, 3
    lib = xc.load_library()
    iq, _ = _scene(W, B, N, seed=N)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def raw(eng, K, weighting, bounds, U, quality="own", refined_entry=False):
        out = [np.zeros((W // max(K, 1), P) if W % max(K, 1) == 0 else (W, P), t) for t in (np.int32, np.float32, np.float32)]
        q = np.full(out[0].shape + (4,), -1.0, np.float32)
        head = (eng._ctx, vp(iq), W, None, P, K, None, 0, weighting, vp(bounds), 0, U)
        if refined_entry:
            rc = lib.rmx_xcorr_batch_refined(*head, *[vp(o) for o in out], 0)
        else:
            qp = {"own": vp(q), "null": None, "peak": vp(out[2]), "frac": vp(out[1])}[quality]
            rc = lib.rmx_xcorr_batch_quality(*head, *[vp(o) for o in out], qp, 0)
        return rc, lib.rmx_last_error(eng._ctx).decode(), out, q

    with xc.XcorrEngine(B, N, W) as fresh:
        want_plain = fresh.correlate(iq)
    lb = np.array([[-30, 30], [-40, 35], [-(N - 1), N - 1]], np.int32)
    bad_lb = np.array([[-3, 3], [7, 6], [-3, 3]], np.int32)
    with xc.XcorrEngine(B, N, W) as eng:
        for K, wt, bounds, U in ((1, 0, None, 0), (1, 1, lb, 8), (2, 0, lb, 4)):
            rc_r, _, out_r, _ = raw(eng, K, wt, bounds, U, refined_entry=True)
            rc_n, _, out_n, q_n = raw(eng, K, wt, bounds, U, quality="null")
            rc_q, _, out_q, q_q = raw(eng, K, wt, bounds, U)
            assert rc_r == 0 and rc_n == 0 and rc_q == 0
            assert _same(out_r, out_n) and np.all(q_n == -1.0)
            assert _same(out_r, out_q)
            assert not np.any(q_q == -1.0)
        rc, msg, _, _ = raw(eng, 3, 7, bad_lb, 3, "peak")
        assert rc == -1 and "integrate = 3" in msg, msg
        rc, msg, _, _ = raw(eng, 2, 7, bad_lb, 3, "peak")
        assert rc == -1 and "weighting" in msg, msg
        rc, msg, _, _ = raw(eng, 2, 1, bad_lb, 3, "peak")
        assert rc == -1 and "lag_bounds" in msg and "pair 1" in msg, msg
        rc, msg, _, _ = raw(eng, 2, 1, None, 3, "peak")
        assert rc == -1 and "refine = 3" in msg, msg
        rc, msg, _, q = raw(eng, 2, 1, None, 8, "peak")
        assert rc == -1 and "quality overlaps peak" in msg, msg
        rc, msg, _, _ = raw(eng, 1, 0, None, 0, "frac")
        assert rc == -1 and "quality overlaps lag_frac" in msg, msg
        assert _same(eng.correlate(iq), want_plain)
