"""rmx_xcorr_batch_bands_integrated on the GPU: noncoherent integration over K consecutive windows under several bands per
window, over one set of forward spectra -- bit for bit against the single-band integrated quality call band by band,
against the reference (tests/bands_integrated_ref.py) at the bars of the refined and the quality entries on every route and
seam, the identities with their launch counts, uint8 input, device pointers on a caller's stream, the refusals in their
order, a dead receiver and the seam with share_integrated.  The parity helpers and the band generators are those of
tests/test_gpu_bands_quality.py."""
import ctypes as C
import math

import numpy as np
import pytest

import bands_integrated_ref as bi
import bands_ref as br
import radio_mapper_amd as rm
import test_gpu_bands_quality as tbq
import weighted_ref as wr

pytestmark = pytest.mark.gpu
CUSTOM = tbq.CUSTOM   # a reversed pair and a self pair


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


# (route name, N, buoys, windows, K, bands, default options, engine options, forward families, pair family, chunks)
ROUTES = [
    ("k_pair_str", 4096, 3, 4, 2, 3, {}, {}, ("k_fwd",), "k_win|k_pair", 1),
    # two groups in the first chunk, one in the second: the seam
    ("k_pair_str chunk seam", 4096, 3, 12, 4, 2, {}, {"chunk_windows": 8}, ("k_fwd",), "k_win|k_pair", 2),
    ("small N=16 gen_chunk 3", 16, 3, 6, 3, 3, {"gen_chunk": 3}, {}, ("g_fwd_small",), "g_pair_small", 2),
    ("small N=16 64 bands", 16, 3, 2, 2, 64, {}, {}, ("g_fwd_small",), "g_pair_small", 1),
    ("small N=256", 256, 4, 6, 2, 3, {}, {}, ("g_fwd_small",), "g_pair_small", 1),
    ("four-step N=256 gen_chunk 2", 256, 3, 6, 2, 3, {"small_maxl": 256, "gen_chunk": 2}, {}, ("g_cols_fwd", "g_rows_fwd"), "g_rows_inv", 3),
    ("four-step N=8192", 8192, 3, 2, 2, 2, {}, {}, ("g_cols_fwd", "g_rows_fwd"), "g_rows_inv", 1),
]
ALL_U = ("k_pair_str", "small N=256", "four-step N=256 gen_chunk 2")   # all four U on one route per layout
WITH_CUSTOM = ("k_pair_str", "small N=256", "four-step N=256 gen_chunk 2")
# the case generator's seed per route: the smallest for which the reference's own coarse top-two margin exceeds 1e-5 on
# every slot of every case (found on the CPU with the reference alone: 8e-4 is the smallest margin of any route)
SEEDS = {r[0]: 1 for r in ROUTES}
FORBIDDEN = tbq.FORBIDDEN


def _inputs(route):
    """every window of a group carries the group's delays (the scene integration is for); noise and signal differ"""
    name, N, B, W, K = route[:5]
    rng = np.random.default_rng(100 + len(name))
    D = min(40, N / 8)
    delays = np.repeat(rng.uniform(-D, D, size=(W // K, B)), K, axis=0)
    return rm.synth.make_windows(W, B, N, 10e6, seed=len(name), snr_db=10, bandwidth=0.8, max_delay=D, return_u8=True, delays=delays)


def _cases(route):
    """the calls of one route, (bands, PHAT, lag bounds, pair list, U): per-window bands that differ inside a group and
    shared bands, NONE and PHAT, no / shared / per-group bounds, U = 2, 8 and 16 -- 4 too, and a custom pair list, on one
    route per layout"""
    name, N, B, W, K, M = route[:6]
    rng = np.random.default_rng(SEEDS[name])
    delays = _inputs(route)[1][::K]                                            # [G][B]
    G, P = W // K, B * (B - 1) // 2
    shared = tbq._wide_bands(rng, (M,), N)
    per_win = tbq._wide_bands(rng, (W, M), N)
    lb_group = tbq._bounds_around(rng, (G, P), N, tbq._true_lags(delays, None, B))
    reach = min(42, N - 1)
    lb_shared = np.tile(np.array([[-reach, reach]], np.int32), (P, 1))
    lb_shared[0] = (-(N - 1), reach)
    cases = [(per_win, False, None, None, 2), (shared, True, lb_shared, None, 16), (per_win, True, lb_group, None, 8)]
    if name in ALL_U:
        cases.append((shared, False, lb_group, None, 4))
    if name in WITH_CUSTOM:
        lb_custom = np.tile(np.array([[-reach, reach]], np.int32), (len(CUSTOM), 1))
        cases.append((per_win, False, lb_custom, CUSTOM, 8))
    return cases


def _launches(tk):
    return {k: v["launches"] for k, v in tk.items()}


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_against_the_single_band_call_and_the_reference(xc, opts, route):
    """Per route and case: (a) [:, m] of all four arrays bit for bit correlate(band=bands[:, m], integrate=K, refine=U,
    quality=True) on the same engine -- three buoys or a custom list: never g_rows_anchor --; (b) parity with
    bands_integrated_ref at the refined and the quality bars, no slot left out by the margin rule; quality leaves the three
    lag outputs alone; a repeated call and uint8 input bit-identical; ONE forward pass, one k_quality and one k_refine launch
    per chunk and none of the kernels that keep their spectra to themselves."""
    name, N, B, W, K, M, dopt, eopt, fwd, pair_family, chunks = route
    for k, v in dopt.items():
        opts(k, v)
    iq, _, raw = _inputs(route)
    G = W // K
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        eng.set_option("timing", 1)
        for n_case, (bands, phat, bounds, pairs, U) in enumerate(_cases(route)):
            what = "%s case %d U=%d" % (name, n_case, U)
            got = eng.correlate_bands(iq, bands, pairs, lag_bounds=bounds, whiten=phat, refine=U, quality=True, integrate=K)
            tk = eng.last_timing_by_kernel()
            P = len(pairs) if pairs else B * (B - 1) // 2
            assert len(got) == 4 and got[0].shape == (G, M, P) and got[3].shape == (G, M, P, 4) and got[3].dtype == np.float32
            pw = br.per_window(bands, W)
            if pw.ndim == 3 and np.asarray(bands).ndim == 3:
                assert any(not np.array_equal(pw[g * K], pw[g * K + 1]) for g in range(G)), "bands must differ inside a group"
            for m in range(M if M <= 8 else 5):                                  # (a)
                mm = m if M <= 8 else (0, 1, 31, 62, 63)[m]
                one = eng.correlate(iq, pairs, lag_bounds=bounds, band=pw[:, mm], whiten=phat, integrate=K, refine=U, quality=True)
                tk1 = eng.last_timing_by_kernel()
                assert "g_rows_anchor" not in tk1
                assert tbq._same([g[:, mm] for g in got], one), "%s: band %d differs from the single-band call" % (what, mm)
            ref = bi.bands_integrated_batch(iq, bands, K, U, phat, bounds, pairs)   # (b)
            tbq._assert_refined(got, ref, N, bounds, what)
            tbq._assert_quality(got[3], ref[6], N, what)
            four = {"g_cols_inv", "g_final"} if len(fwd) == 2 else set()
            assert set(tk) == set(fwd) | {pair_family, "k_refine", "k_quality"} | four, tk
            assert not set(tk) & set(FORBIDDEN)
            for f in fwd:
                assert tk[f]["launches"] == tk1[f]["launches"], (f, tk, tk1)
            assert tk["k_refine"]["launches"] == chunks and tk["k_quality"]["launches"] == chunks, tk
            no_q = eng.correlate_bands(iq, bands, pairs, lag_bounds=bounds, whiten=phat, refine=U, integrate=K)
            assert len(no_q) == 3 and tbq._same(no_q, got[:3]), what + ": quality changed a lag output"
            assert "k_quality" not in eng.last_timing_by_kernel()
            assert tbq._same(got, eng.correlate_bands(iq, bands, pairs, lag_bounds=bounds, whiten=phat, refine=U, quality=True,
                                                      integrate=K)), "twice"
            if n_case == 0:
                assert tbq._same(got, eng.correlate_bands(raw, bands, pairs, lag_bounds=bounds, whiten=phat, refine=U, quality=True,
                                                          integrate=K)), "uint8 input"


@pytest.mark.parametrize("route", [ROUTES[0], ROUTES[4], ROUTES[5], ROUTES[6]], ids=lambda r: r[0])
def test_narrow_bands_and_the_coarse_call_against_the_single_band_call(xc, opts, route):
    """Random bands down to two bins wide (held to the single-band call and the quality bar only, as
    tests/test_gpu_bands_quality.py argues), refined and coarse (refine = 0, with and without quality)."""
    name, N, B, W, K, M, dopt, eopt = route[:8]
    for k, v in dopt.items():
        opts(k, v)
    iq = _inputs(route)[0]
    rng = np.random.default_rng(N + M + K)
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        for U, phat, q in ((0, False, False), (0, True, True), (4, False, True), (16, True, True)):
            bands = tbq._random_bands(rng, (W, M), N)
            got = eng.correlate_bands(iq, bands, whiten=phat, refine=U, quality=q, integrate=K)
            for m in range(M):
                one = eng.correlate(iq, band=bands[:, m], whiten=phat, refine=U, quality=q, integrate=K)
                assert tbq._same([g[:, m] for g in got], one), (name, U, phat, m)
            if q:
                tbq._assert_quality(got[3], bi.bands_integrated_batch(iq, bands, K, 0, phat)[6], N, "%s narrow U=%d" % (name, U))


def _direct(xc, eng, entry, iq, bands, K=None, refine=None, quality=False, whiten=False, lag_bounds=None, rows=None):
    """a banded C entry itself with host pointers and the default pair list -> (rc, text, outs [+ quality])"""
    lib = xc.load_library()
    W, B = iq.shape[0], iq.shape[1]
    P = B * (B - 1) // 2
    bd = np.ascontiguousarray(bands, np.float64)
    M, pw = bd.shape[-2], int(bd.ndim == 3)
    lb = None if lag_bounds is None else np.ascontiguousarray(lag_bounds, np.int32)
    rows = W if rows is None else rows
    outs = [np.zeros((rows, M, P), t) for t in (np.int32, np.float32, np.float32)]
    ql = np.zeros((rows, M, P, 4), np.float32) if quality else None
    vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731
    args = [eng._ctx, vp(iq), W, None, P] + ([K] if K is not None else [])
    args += [vp(bd), M, pw, 1 if whiten else 0, vp(lb), 0 if lb is None else int(lb.ndim == 3)]
    args += ([refine] if refine is not None else []) + [vp(o) for o in outs] + ([vp(ql)] if refine is not None else []) + [0]
    rc = getattr(lib, entry)(*args)
    return rc, lib.rmx_last_error(eng._ctx).decode(), outs + ([ql] if quality else [])


@pytest.mark.parametrize("route", [ROUTES[0], ROUTES[2], ROUTES[5], ROUTES[6]], ids=lambda r: r[0])
def test_the_identities(xc, opts, route):
    """integrate == 1 IS rmx_xcorr_batch_bands_quality; refine == 0, quality == NULL and integrate == 1 IS
    rmx_xcorr_batch_bands; n_bands == 1 IS rmx_xcorr_batch_quality: the same bits from the same launches."""
    name, N, B, W, K, M, dopt, eopt = route[:8]
    for k, v in dopt.items():
        opts(k, v)
    iq, delays, _ = _inputs(route)
    rng = np.random.default_rng(N + W)
    bands = tbq._random_bands(rng, (W, M), N)
    P = B * (B - 1) // 2
    lb_w = tbq._bounds_around(rng, (W, P), N, tbq._true_lags(delays, None, B))
    lb_g = lb_w[::K]
    new = "rmx_xcorr_batch_bands_integrated"
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        eng.set_option("timing", 1)
        for phat, bounds in ((False, None), (True, lb_w)):
            rc, text, old = _direct(xc, eng, "rmx_xcorr_batch_bands_quality", iq, bands, None, 8, True, phat, bounds)
            t_old = _launches(eng.last_timing_by_kernel())
            assert rc == 0, text
            rc, text, got = _direct(xc, eng, new, iq, bands, 1, 8, True, phat, bounds)
            assert rc == 0, text
            assert tbq._same(old, got) and t_old == _launches(eng.last_timing_by_kernel())
            rc, text, old = _direct(xc, eng, "rmx_xcorr_batch_bands", iq, bands, None, None, False, phat, bounds)
            t_old = _launches(eng.last_timing_by_kernel())
            assert rc == 0, text
            rc, text, got = _direct(xc, eng, new, iq, bands, 1, 0, False, phat, bounds)
            assert rc == 0, text
            assert tbq._same(old, got) and t_old == _launches(eng.last_timing_by_kernel())
        for phat, bounds in ((False, None), (True, lb_g)):
            b = eng.correlate(iq, lag_bounds=bounds, band=bands[:, 0], whiten=phat, integrate=K, refine=8, quality=True)
            t_b = _launches(eng.last_timing_by_kernel())
            rc, text, a = _direct(xc, eng, new, iq, bands[:, :1], K, 8, True, phat, bounds, rows=W // K)
            assert rc == 0, text
            assert tbq._same([x[:, 0] for x in a], b) and t_b == _launches(eng.last_timing_by_kernel())


@pytest.mark.parametrize("route", [ROUTES[1], ROUTES[4], ROUTES[6]], ids=lambda r: r[0])
def test_device_pointers_on_a_callers_stream_back_to_back(xc, opts, route):
    """Device pointers on a non-null stream: two asynchronous calls with DIFFERENT bands back to back, the caller's host
    arrays overwritten as soon as each call returns; each result is the host-pointer call's."""
    torch = pytest.importorskip("torch")
    name, N, B, W, K, M, dopt, eopt = route[:8]
    for k, v in dopt.items():
        opts(k, v)
    iq, delays, raw = _inputs(route)
    G, P = W // K, B * (B - 1) // 2
    rng = np.random.default_rng(11)
    lb = tbq._bounds_around(rng, (G, P), N, tbq._true_lags(delays[::K], None, B))
    sets = [tbq._random_bands(rng, (W, M), N) for _ in range(2)]
    with xc.XcorrEngine(B, N, W) as eng:
        for k, v in eopt.items():
            eng.set_option(k, v)
        host = [eng.correlate_bands(iq, b, lag_bounds=lb, whiten=True, refine=4, quality=True, integrate=K) for b in sets]
        stream = torch.cuda.Stream()
        eng.set_stream(stream.cuda_stream)
        try:
            for x, u8 in ((iq.view(np.float32), False), (raw, True)):
                with torch.cuda.stream(stream):
                    d_iq = torch.from_numpy(x).cuda()
                    outs = [[torch.full((G, M, P), -7, dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.float32)]
                            for _ in range(2)]
                    d_q = [torch.full((G, M, P, 4), -7, dtype=torch.float32, device="cuda") for _ in range(2)]
                    stream.synchronize()
                    for n in range(2):
                        mine, mine_lb = sets[n].copy(), lb.copy()
                        eng.correlate_bands_device(d_iq.data_ptr(), W, mine, *[o.data_ptr() for o in outs[n]], u8=u8, lag_bounds=mine_lb,
                                                   whiten=True, refine=4, quality_ptr=d_q[n].data_ptr(), integrate=K)
                        mine[:] = (0.0, 0.0)                     # the caller may reuse its arrays at once
                        mine_lb[:] = 0
                    eng.synchronize()
                for n in range(2):
                    assert tbq._same(host[n], [o.cpu().numpy() for o in outs[n]] + [d_q[n].cpu().numpy()]), (name, u8, n)
        finally:
            eng.set_stream(0)


def test_refusals_in_their_order_leave_the_outputs_untouched(xc):
    N, W, K, M, P = 256, 4, 2, 3, 3
    G = W // K
    iq, _ = rm.synth.make_windows(W, 3, N, 10e6, seed=1)
    lib = xc.load_library()
    good = np.tile([[-0.5, 0.5], [0.0, 0.25], [-0.1, 0.1]], (W, 1, 1))
    with xc.XcorrEngine(3, N, W) as eng:
        block = np.full(8 * G * M * P, 77, np.float32)      # quality, and room to overlap the others with
        out = [np.full((G, M, P), 77, t) for t in (np.int32, np.float32, np.float32)]
        ql = block[:4 * G * M * P].reshape(G, M, P, 4)
        vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)   # noqa: E731

        def call(bands, n_bands=M, per_window=1, bounds=None, bounds_pg=0, weighting=0, iq_p=iq, refine=4, quality=ql, outs=out,
                 n_windows=W, pairs=None, n_pairs=P, integrate=K):
            b = None if bands is None else np.ascontiguousarray(bands, np.float64)
            lb = None if bounds is None else np.ascontiguousarray(bounds, np.int32)
            rc = lib.rmx_xcorr_batch_bands_integrated(eng._ctx, vp(iq_p), n_windows, vp(pairs), n_pairs, integrate, vp(b), n_bands,
                                                      per_window, weighting, vp(lb), bounds_pg, refine, *[vp(o) for o in outs],
                                                      vp(quality), 0)
            return rc, lib.rmx_last_error(eng._ctx).decode()
        assert call(good)[0] == 0 and not np.any(out[0] == 77) and not np.any(ql == 77)
        for o in out + [block]:
            o[:] = 77
        over = out[2].reshape(-1)[:1]
        # 1. integrate and the group count, in front of everything else
        for k_bad in (0, -3):
            rc, text = call(None, integrate=k_bad, n_bands=0, refine=3, quality=over)
            assert rc == -1 and "integrate = %d" % k_bad in text, text
        rc, text = call(None, integrate=3, n_bands=0, refine=3)
        assert rc == -1 and "not a positive multiple of integrate = 3" in text, text
        rc, text = call(good, n_windows=0)
        assert rc == -1 and "not a positive multiple" in text, text
        for more in ({}, {"refine": 3}, {"refine": 3, "quality": over}):
            # 2. NULL buffer, band_cps included; 3. (alignment: host pointers need none); 4. n_bands
            assert call(None, **more) == (-1, "NULL buffer") and call(good, iq_p=None, **more) == (-1, "NULL buffer")
            assert call(None, n_bands=0, **more)[1] == "NULL buffer"
            for n_bands in (0, 65, -1):
                rc, text = call(good, n_bands=n_bands, **more)
                assert rc == -1 and "n_bands" in text
            # 5. weighting and bands: band m of the REAL window w
            rc, text = call(good, weighting=2, **more)
            assert rc == -1 and "weighting" in text
            assert "n_bands" in call(good, n_bands=0, weighting=2, **more)[1]
            for bad in ([0.5, 0.5], [np.nan, 0.1], [0.2, 0.1], [-0.6, 0.1], [1e-9, 2e-9]):
                bands = good.copy()
                bands[3, 1] = bad
                rc, text = call(bands, **more)
                assert rc == -1 and "band 1 of window 3" in text, text
                rc, text = call(bands[3], per_window=0, **more)
                assert rc == -1 and "band 1 of window 0" in text and "shared" in text, text
            # 6. the batch shape
            rc, text = call(good, n_pairs=2, **more)
            assert rc == -1 and "pairs == NULL needs" in text, text
            rc, text = call(good, n_windows=W + K, **more)
            assert rc == -1 and "n_windows" in text, text
            # 7. the bounds, per GROUP
            for lo, hi in ((-N, 0), (0, N), (5, 4)):
                lb = np.tile(np.array([[-3, 3]], np.int32), (G, P, 1))
                lb[1, 2] = (lo, hi)
                rc, text = call(good, bounds=lb, bounds_pg=1, **more)
                assert rc == -1 and "lag_bounds of group 1, pair 2" in text, text
        # 8. refine, in front of 9. the overlap, whose text counts G * n_bands * P slots
        for bad in (1, 3, -2, 32):
            rc, text = call(good, refine=bad, quality=over)
            assert rc == -1 and "refine = %d" % bad in text, text
        for refine in (0, 8):
            for k, nm in enumerate(("lag_int", "lag_frac", "peak")):
                rc, text = call(good, refine=refine, quality=out[k].view(np.float32).reshape(-1)[-1:])
                assert rc == -1 and "quality overlaps " + nm in text and "the %d x 4 floats" % (G * M * P) in text, text
        assert all(np.all(o == 77) for o in out) and np.all(block == 77), "a refused call wrote an output"
    # the route: K = 128 fits this ctx's chunk of 128 windows, but 64 bands leave a chunk of 4096 / 64 = 64 windows
    W, K, M = 128, 128, 64
    iq, _ = rm.synth.make_windows(W, 3, 16, 10e6, seed=2)
    bands = np.tile([[-0.5, 0.5]], (M, 1))
    with xc.XcorrEngine(3, 16, W) as eng:
        li, lf, pk = eng.correlate(iq, integrate=K)                       # alone, K fits
        assert li.shape == (1, 3)
        outs = [np.full((1, M, 3), 77, t) for t in (np.int32, np.float32, np.float32)]
        vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
        rc = lib.rmx_xcorr_batch_bands_integrated(eng._ctx, vp(iq), W, None, 3, K, vp(bands), M, 0, 0, None, 0, 0, *[vp(o) for o in outs],
                                                  None, 0)
        text = lib.rmx_last_error(eng._ctx).decode()
        assert rc == -1 and "integrate = 128" in text and "n_bands = 64" in text and "64 windows" in text and "shrank" in text, text
        assert all(np.all(o == 77) for o in outs)
        got = eng.correlate_bands(iq, bands[:32], integrate=K)            # 32 bands leave 128 windows: served
        assert tbq._same([g[:, 0] for g in got], (li, lf, pk))


@pytest.mark.parametrize("N,whiten", [(256, False), (4096, True), (8192, False)])
def test_a_dead_receiver_gives_zeros_never_nan(xc, N, whiten):
    B, W, K = 3, 4, 2
    iq, _ = rm.synth.make_windows(W, B, N, 10e6, seed=9, snr_db=10, max_delay=20)
    iq[:, 1] = 0
    bands = np.array([[-0.4, 0.0], [-0.1, 0.45]])
    with xc.XcorrEngine(B, N, W) as eng:
        li, lf, pk, q = eng.correlate_bands(iq, bands, whiten=whiten, refine=4, quality=True, integrate=K)
        for m in range(2):
            one = eng.correlate(iq, band=bands[m], whiten=whiten, refine=4, quality=True, integrate=K)
            assert tbq._same([x[:, m] for x in (li, lf, pk, q)], one)
    assert not np.any(np.isnan(q)) and not np.any(np.isnan(pk)) and not np.any(np.isnan(lf))
    assert np.all(pk[..., [0, 2]] == 0) and np.all(q[..., [0, 2], :] == 0) and np.all(pk[..., 1] > 0)
    tbq._assert_quality(q, bi.bands_integrated_batch(iq, bands, K, 0, whiten)[6], N, "dead receiver, N = %d" % N)


def test_seam_share_integrated_gives_the_measurements_of_the_separate_calls(xc):
    """TDoAProcessor with band_limit, integrate = 4, refine = 8 and min_psr on a two-transmitter capture of three buoys,
    N = 4096: the two frequency groups once as 2 x 4 segments of the single-band integrated quality call and once,
    share_captures + share_qualified + share_integrated, as 4 segments under two bands -- identical measurements in the same
    order, and the banded call carried integrate, refine and quality."""
    from radio_mapper_amd import tdoa_processor as tp
    fs, N, fc, K = 2.048e6, 4096, 121.0e6, 4
    lat0, lng0 = 37.0, -122.0
    buoys = [("B0", lat0, lng0), ("B1", lat0 + 0.3, lng0), ("B2", lat0, lng0 + 0.4)]
    xyz = [tp.GeodeticCalculator.lat_lng_to_xyz(la, lo, 0.0) for _, la, lo in buoys]
    tx = {"strong": (lat0 + 0.1, lng0 + 0.12), "weak": (lat0 + 0.22, lng0 + 0.3)}
    delays = {}
    for k, (la, lo) in tx.items():
        e = tp.GeodeticCalculator.lat_lng_to_xyz(la, lo, 0.0)
        d = [math.dist(e, x) / tp.TDoACalculator.SPEED_OF_LIGHT * fs for x in xyz]
        delays[k] = [int(round(v - min(d))) for v in d]
    iq, _, _ = wr.two_emitter_scene(N=N, d_strong=delays["strong"], d_weak=delays["weak"], seed=6)
    f_strong, f_weak = fc + 0.10 * fs, fc - 0.25 * fs
    t0 = 1_700_000_000_000_000_000

    def run(bound_lags, min_psr, **flags):
        p = tp.TDoAProcessor(band_limit=True, integrate=K, refine=8, min_psr=min_psr, correlation_confidence=True, **flags)
        p.tdoa_calculator.bound_lags = bound_lags
        for bid, la, lo in buoys:
            p.register_buoy(tp.BuoyPosition(bid, la, lo, 0.0, timing_accuracy_ns=20))
        calls, groups = [], []
        eng_of = p.tdoa_calculator._engine

        def engine(*a, **k):
            eng = eng_of(*a, **k)
            if not getattr(eng, "_recorded", False):
                for name in ("correlate", "correlate_bands"):
                    def rec(*aa, _f=getattr(eng, name), _n=name, **kk):
                        calls.append((_n, np.asarray(aa[0]).shape, kk.get("integrate", 1), kk.get("refine", 0), bool(kk.get("quality", False))))
                        return _f(*aa, **kk)
                    setattr(eng, name, rec)
                eng._recorded = True
            return eng
        p.tdoa_calculator._engine = engine
        p.hyperbolic_positioner.triangulate_position = lambda meas, pos: groups.append(
            [(m.buoy1_id, m.buoy2_id, m.frequency_mhz, m.time_difference_ns, m.confidence) for m in meas])
        dets = []
        for f in (f_strong, f_weak):
            dets += [tp.SignalDetection(bid, f / 1e6, -60.0, "t", t0, la, lo, 0.9, iq_samples=iq[0, b], sample_rate_hz=fs,
                                        center_freq_hz=fc, bandwidth_hz=0.1 * fs)
                     for b, (bid, la, lo) in enumerate(buoys)]
        p.process_signal_detections(dets)
        p.tdoa_calculator.close()
        return calls, groups

    for bound_lags in (False, True):
        for min_psr in (2.0, 1e9):         # every pair passes / every pair is dropped, on both sides alike
            calls_on, meas_on = run(bound_lags, min_psr, share_captures=True, share_qualified=True, share_integrated=True)
            calls_off, meas_off = run(bound_lags, min_psr, share_captures=False)
            assert calls_on == [("correlate_bands", (K, 3, N // K), K, 8, True)], calls_on
            assert calls_off == [("correlate", (2 * K, 3, N // K), K, 8, True)], calls_off
            assert meas_on == meas_off
            assert len(meas_on) == (2 if min_psr < 1e9 else 0)
            if meas_on:
                assert [len(g) for g in meas_on] == [3, 3]
                for g, k in zip(meas_on, ("strong", "weak")):
                    lag = np.array([m[3] * 1e-9 * fs for m in g])
                    assert np.all(np.abs(lag - wr.true_lags(delays[k])) < 0.5), (k, lag)
            # share_captures and share_qualified alone still stand back for integration
            assert run(bound_lags, min_psr, share_captures=True, share_qualified=True)[0] == calls_off
