"""Peak selection of rmx_detect_batch checked exactly (include/rmx.h, detection block).

CPU: the selection reference (tests/detect_select_ref.py) pinned against scipy's find_peaks / _local_maxima_1d /
_select_by_peak_distance, and the exact-spectrum windows pinned against scipy.fft.

GPU:
  - windows whose DFT every radix-2/4 FFT computes exactly (non-zero only at n = 0, N/4, N/2, 3N/4, Gaussian-integer
    values: the only twiddles involved are 1 and +-i), so the peak set is known without any FFT rounding: plateaus,
    edges, -240 dB bins, exact ties, every window length, distances up to 2^31 - 1;
  - realistic windows: one call with every local maximum (distance 1, no threshold, no cuts), then a parameter grid
    whose results must be the reference's selection applied to that call's own candidates, bit for bit (both calls
    see the same spectrum, so no FFT-rounding excuse is needed); the candidates against the oracle bin by bin;
  - truncation at max_peaks on several windows, the device-pointer flags, one ctx across window lengths, errors."""
import ctypes as C

import numpy as np
import pytest
import scipy.fft
import scipy.signal
from scipy.signal._peak_finding_utils import _local_maxima_1d, _select_by_peak_distance

from detect_select_ref import F32, keep_by_distance, local_maxima, noise_floor, select, select_candidates
from oracle import detect_ref as dr
from test_detect import make_windows

LENGTHS = [1 << k for k in range(4, 15)]        # 16 ... 16384: every length the ABI takes
RMX_E_INVAL = -1
BIG = [2**30 + 1, 2**31 - 1]                    # 2 (d - 1) + 1 overflows int for both


# ------------------------------------------------------------------------------------------- the exact windows
# quarter q -> the sample at n = q N / 4.  |X| repeats with period 4 (k = 0, 1, 2, 3):
PATTERNS = (
    {0: -4 - 4j, 1: 2 - 4j, 2: -2, 3: -2},   # 10 10 6 2: plateaus of 2 (lower bin), the one at bins 0-1 is no peak
    {0: 2, 1: -0.5, 2: -0.5, 3: -0.5},       # .5 2.5 2.5 2.5: plateaus of 3, the last touches N-1 (no peak)
    {0: 1, 2: 1},                            # 2 0: -240 dB bins, a median between distinct middle values
    {0: 3, 2: 1},                            # 4 2: N/2 - 1 equal peaks -- the tie rule at every distance >= 3
)
UNITS = (1, 1j, -1, -1j)
_ROT = (1, -1j, -1, 1j)                          # (-i)^m


def exact_window(N, k, unit=1):
    x = np.zeros(N, np.complex64)
    for q, v in PATTERNS[k].items():
        x[q * N // 4] = v * unit
    return x


def exact_spectrum(N, k, unit=1):
    """X[f] = sum_q x_q (-i)^(q f), in complex128 (exact: Gaussian integers and halves)"""
    X4 = np.array([sum(v * unit * _ROT[(q * f) % 4] for q, v in PATTERNS[k].items()) for f in range(4)], np.complex128)
    return np.tile(X4, N // 4)


def exact_batch(N, W=8):
    """W windows mixing the four patterns and four unit factors; returns (x [W][N], |X| float64 [W][N])"""
    x = np.zeros((W, N), np.complex64)
    m = np.zeros((W, N))
    for w in range(W):
        k, u = w % 4, UNITS[(w // 4) * 2 + w % 2]
        x[w] = exact_window(N, k, u)
        m[w] = np.abs(exact_spectrum(N, k, u))
    return x, m


def db32(m):
    """float32 dB spectrum of exact magnitudes (what the kernel computes, up to log10f's last bits)"""
    return (F32(20.0) * np.log10(np.asarray(m, np.float32) + F32(1e-12))).astype(np.float32)


def db64(m):
    """20 log10(m + 1e-12) of exact magnitudes, the addition in float32 as the kernel does it"""
    return 20.0 * np.log10((np.asarray(m, np.float32) + F32(1e-12)).astype(np.float64))


def ulps(x, n):
    return n * np.spacing(np.abs(np.asarray(x, np.float32)))


# ------------------------------------------------------------------------------------------- CPU: the reference
def _distinct_spectrum(rng, N):
    while True:
        p = (rng.standard_normal(N) * 10.0).astype(np.float32)
        if np.unique(p).shape[0] == N:
            return p


@pytest.mark.parametrize("N", [16, 64, 1000, 4096])
def test_reference_equals_find_peaks_on_distinct_heights(N):
    rng = np.random.default_rng(N)
    for rep in range(3):
        p = _distinct_spectrum(rng, N)
        cand = local_maxima(p)
        for thr in (None, float(np.quantile(p[cand], 0.4))):
            h = cand if thr is None else cand[p[cand] >= F32(thr)]
            for d in (1, 2, 3, 10, 25, N - 1, N, 10 * N, 1.5, 2.5, 7.3, N - 0.5):
                want, _ = scipy.signal.find_peaks(p, height=thr, distance=d)
                got = h[keep_by_distance(h, p[h], d, N)]
                assert np.array_equal(got, want), (N, rep, thr, d)
                if len(h):
                    k = _select_by_peak_distance(h.astype(np.intp), p[h].astype(np.float64), float(d))
                    assert np.array_equal(got, h[k.astype(bool)]), (N, rep, thr, d)
                if d >= N and len(h):
                    assert np.array_equal(got, [h[np.argmax(p[h])]])


def test_reference_ceils_fractional_distance():
    """peaks at 5 and 7, distance 2.5: scipy ceils to 3 and keeps one"""
    p = np.zeros(16, np.float32)
    p[5], p[7] = 2.0, 1.0
    want, _ = scipy.signal.find_peaks(p, distance=2.5)
    assert list(want) == [5]
    c = local_maxima(p)
    assert list(c[keep_by_distance(c, p[c], 2.5, 16)]) == [5]
    assert list(c[keep_by_distance(c, p[c], 2, 16)]) == [5, 7]


def test_reference_tie_rule():
    """exact ties keep the higher bin (the kernel's documented rule; scipy's order there is numpy's unstable argsort)"""
    p = np.zeros(64, np.float32)
    p[2:62:4] = 1.0                                   # 15 equal peaks, 4 bins apart
    c = local_maxima(p)
    assert list(c) == list(range(2, 62, 4))
    assert list(c[keep_by_distance(c, p[c], 5, 64)]) == list(range(58, 0, -8))[::-1]
    assert list(c[keep_by_distance(c, p[c], 64, 64)]) == [58]
    assert list(c[keep_by_distance(c, p[c], 4, 64)]) == list(c)


def _plateau_arrays():
    out = []
    for L in range(1, 6):
        for start in (0, 1, 2, 5):
            for tail in (0, 1, 3):
                a = [0.0] * start + [3.0] * L + [0.0] * tail
                out.append(a)
                out.append([1.0] + a)
                out.append(a + [2.0, 0.5])
    out += [[1, 2, 2, 1, 2, 2, 2, 1, 3, 3, 3, 3, 3, 0], [5, 5, 5], [0, 1, 0], [0, 1], [1], [],
            [0, 2, 2, 1, 2, 2, 0], [0, 1, 1, 2, 2, 0, 4, 4, 4, 4, 4]]
    return out


def test_reference_local_maxima_equals_scipy():
    for a in _plateau_arrays():
        x = np.asarray(a, np.float64)
        want = _local_maxima_1d(x)[0]
        assert np.array_equal(local_maxima(x.astype(np.float32)), want), a
    rng = np.random.default_rng(5)
    for _ in range(200):                             # many plateaus of every length, at both ends too
        x = rng.integers(0, 4, size=int(rng.integers(3, 80))).astype(np.float64)
        assert np.array_equal(local_maxima(x.astype(np.float32)), _local_maxima_1d(x)[0]), x


def test_reference_floor_and_exclusions():
    rng = np.random.default_rng(3)
    for n in (16, 17, 1024):
        p = (rng.standard_normal(n) * 20.0).astype(np.float32)
        assert noise_floor(p) == np.median(p)
    # dc exclusion compares |signed bin| in double; confidence in float32 against float32(min_confidence)
    N = 64
    bins = np.array([2, 4, 6, 58, 60])
    db = np.array([10.0, 10.0, 10.0, 10.0, 10.0], np.float32)
    b, *_ = select_candidates(N, bins, db, F32(0.0), distance=1, dc_exclude_bins=4.0, min_confidence=0.0)
    assert list(b) == [4, 6, 58, 60]
    b, *_ = select_candidates(N, bins, db, F32(0.0), distance=1, dc_exclude_bins=4.0000001, min_confidence=0.0)
    assert list(b) == [6, 58]
    b, pw, snr, conf = select_candidates(N, bins, db, F32(4.0), distance=1, min_confidence=0.3)
    assert list(b) == list(bins) and np.all(conf == F32(0.3)) and np.all(snr == F32(6.0))
    b, *_ = select_candidates(N, bins, db, F32(4.0), distance=1, min_confidence=float(np.nextafter(F32(0.3), F32(1))))
    assert len(b) == 0


@pytest.mark.parametrize("N", LENGTHS)
def test_exact_windows_on_the_cpu(N):
    """scipy.fft computes the patterns exactly, so the oracle's spectrum is the exact one; and the patterns exercise
    what they are meant to (candidate bins pinned here)."""
    x, m = exact_batch(N)
    for w in range(x.shape[0]):
        k, u = w % 4, UNITS[(w // 4) * 2 + w % 2]
        X = scipy.fft.fft(x[w])
        assert X.dtype == np.complex64 and np.array_equal(X.astype(np.complex128), exact_spectrum(N, k, u)), (N, w)
        assert np.array_equal(dr.power_spectrum_db(x[w]), db32(m[w]))
    c = [local_maxima(db32(np.abs(exact_spectrum(N, k)))) for k in range(4)]
    assert list(c[0]) == list(range(4, N, 4))                 # plateau (4m, 4m+1) -> 4m; bins 0-1 no peak
    assert list(c[1]) == list(range(2, N - 4, 4))             # plateau 4m+1..4m+3 -> 4m+2; N-3..N-1 no peak
    assert list(c[2]) == list(range(2, N - 1, 2)) and list(c[3]) == list(range(2, N - 1, 2))
    fl = noise_floor(db32(np.abs(exact_spectrum(N, 2))))
    assert fl == F32(F32(db32([0.0])[0] + db32([2.0])[0]) * F32(0.5))


# ------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def xc():
    import __graft_entry__ as g
    g.build()
    from radio_mapper_amd import xcorr
    if xcorr.device_count() < 1:
        pytest.fail("no GPU visible")
    return xcorr


@pytest.fixture(scope="module")
def eng(xc):
    e = xc.XcorrEngine(2, 4096, 1)
    yield e
    e.close()


def raw_detect(xc, e, iq, W, N, max_peaks, thr=-70.0, dist=10, dc=0.0, mc=0.3, flags=0, fill=-7):
    """rmx_detect_batch with host arrays, the count and the whole [W][max_peaks] arrays returned (pre-filled with
    `fill`: entries the call does not write keep it)"""
    out = host_outputs(max(W, 1), max(max_peaks, 1), fill)
    src = C.c_void_p(iq) if isinstance(iq, int) else iq.ctypes.data_as(C.c_void_p)
    rc = xc.load_library().rmx_detect_batch(e._ctx, src, W, N, thr, dist, dc, mc, max_peaks,
                                            *[out[k].ctypes.data_as(C.c_void_p) for k in OUTS], flags)
    return rc, out


OUTS = ("count", "bin", "pw", "snr", "conf", "floor")


def host_outputs(W, max_peaks, fill=-7):
    return dict(count=np.full(W, fill, np.int32), bin=np.full((W, max_peaks), fill, np.int32),
                pw=np.full((W, max_peaks), fill, np.float32), snr=np.full((W, max_peaks), fill, np.float32),
                conf=np.full((W, max_peaks), fill, np.float32), floor=np.full(W, fill, np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("N", LENGTHS)
def test_gpu_exact_spectrum_windows(eng, N):
    x, m = exact_batch(N)
    W = x.shape[0]
    p32 = [db32(m[w]) for w in range(W)]
    p64 = [db64(m[w]) for w in range(W)]
    for d in [1, 2, 3, 4, 5, 8, N - 1, N, N + 1] + BIG:
        for dc in (4.0, 4.0000001):
            for mc in (0.0, 0.3):
                got = eng.detect(x, threshold_db=-70.0, distance=d, dc_exclude_bins=dc, min_confidence=mc,
                                 max_peaks=N // 2)
                for w in range(W):
                    gb, gp, gs, gc, gf = got[w]
                    wb, _, _, _, _ = select(p32[w], -70.0, d, dc, mc)
                    ctx = (N, w, d, dc, mc)
                    assert np.array_equal(gb, wb), ctx
                    assert np.all(np.abs(gp - p64[w][gb]) <= ulps(p64[w][gb], 4)), ctx
                    q = np.sort(p64[w])
                    lo, hi = q[N // 2 - 1], q[N // 2]
                    assert abs(gf - (lo + hi) / 2) <= ulps(max(abs(lo), abs(hi)), 4), ctx
                    assert np.array_equal(gs, (gp - F32(gf)).astype(np.float32)), ctx
                    assert np.array_equal(gc, np.clip(gs / F32(20.0), F32(0), F32(1))), ctx
                    if d >= N and dc == 4.0 and mc == 0.0:    # ties: the highest bin (N - 2 of patterns 2, 3: dc)
                        assert list(gb) == [[N - 4], [N - 6], [], []][w % 4], ctx


def _fft_tolerance_db(x):
    """(oracle dB spectrum, float64 dB spectrum, per-bin dB tolerance of a second float32 FFT against the oracle): the
    4x-own-error rule on the magnitude scale -- a float32 FFT's magnitude error is absolute (of the order of eps times
    the window's rms), so a second one is allowed four times the oracle's largest magnitude error in the window, plus
    the oracle's own, plus 1e-5 dB"""
    m_o = np.abs(scipy.fft.fft(x)).astype(np.float64)
    m64 = np.abs(np.fft.fft(x.astype(np.complex128)))
    e = float(np.max(np.abs(m_o - m64)))
    tol = 5.0 * (20.0 / np.log(10.0)) * e / np.maximum(m64, 1e-30) + 1e-5
    return dr.power_spectrum_db(x), 20.0 * np.log10(m64 + 1e-12), tol


def _margin_ok(k, p64, tol):
    """bin k is a local maximum on one side only: excused only if its comparison with a neighbour is within what the
    two FFTs agree on"""
    return any(abs(p64[k] - p64[j]) <= tol[k] + tol[j] for j in (k - 1, k + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("N", LENGTHS)
def test_gpu_selection_is_the_reference_on_its_own_candidates(eng, N, u8):
    W = 8
    x, raw = make_windows(W, N, seed=700 + N + (1 if u8 else 0), u8=u8)
    iq = raw if u8 else x
    # call A: every local maximum with the kernel's own dB values, and the floor
    A = eng.detect(iq, threshold_db=-np.inf, distance=1, dc_exclude_bins=0.0, min_confidence=0.0, max_peaks=N // 2)
    for w in range(W):
        ab, ap, asn, ac, af = A[w]
        p_o, p64, tol = _fft_tolerance_db(x[w])
        want = _local_maxima_1d(p_o.astype(np.float64))[0]
        for k in np.setxor1d(ab, want):
            assert _margin_ok(int(k), p64, tol), (N, u8, w, int(k))
        common, ia, _ = np.intersect1d(ab, want, return_indices=True)
        dev = np.abs(ap[ia] - p_o[common].astype(np.float64))
        bad = ~((dev < 2e-4) | (dev <= tol[common]))
        assert not bad.any(), (N, u8, w, common[bad], dev[bad], tol[common][bad])
        rf, f64 = float(np.median(p_o)), float(np.median(p64))
        assert abs(af - rf) < 2e-4 or abs(af - rf) <= 4.0 * abs(rf - f64) + 1e-5, (N, u8, w, af, rf, f64)
    # cut levels taken from window 0's candidates: a dB value and a confidence, each exactly and its float32 successor
    ab0, ap0, _, ac0, _ = A[0]
    t0 = F32(np.sort(ap0)[(3 * len(ap0)) // 4])
    inner = np.sort(ac0[(ac0 > 0) & (ac0 < 1)])
    c0 = F32(inner[len(inner) // 2]) if len(inner) else F32(0.5)
    nxt = lambda v: float(np.nextafter(F32(v), F32(np.inf)))   # noqa: E731
    thrs = [-70.0, -np.inf, float(t0), nxt(t0)]
    dists = [2, 3, 10, 25, N - 1, N, 4 * N, 2**30 + 1]
    dcs = [0.0, 10e3 * N / 2.4e6, 3.0]
    mcs = [0.0, 0.3, float(c0), nxt(c0)]
    grid = [(t, d, dcs[c % 3], mcs[(c // 3) % 4]) for c, (t, d) in enumerate((t, d) for t in thrs for d in dists)]
    grid += [(-70.0, 2, 0.0, float(c0)), (-70.0, 2, 0.0, nxt(c0)), (float(t0), 2, 0.0, 0.0), (nxt(t0), 2, 0.0, 0.0)]
    for t, d, dc, mc in grid:
        B = eng.detect(iq, threshold_db=t, distance=d, dc_exclude_bins=dc, min_confidence=mc, max_peaks=N // 2)
        for w in range(W):
            ab, ap, asn, ac, af = A[w]
            bb, bp, bs, bc, bf = B[w]
            wb, wp, ws, wc = select_candidates(N, ab, ap, af, t, d, dc, mc)
            ctx = (N, u8, w, t, d, dc, mc)
            assert np.array_equal(bb, wb), ctx
            ix = np.searchsorted(ab, bb)
            assert np.array_equal(bp, ap[ix]) and np.array_equal(bs, asn[ix]) and np.array_equal(bc, ac[ix]), ctx
            assert np.array_equal(bp, wp) and np.array_equal(bs, ws) and np.array_equal(bc, wc), ctx
            assert np.float32(bf).tobytes() == np.float32(af).tobytes(), ctx
    # the exact cut levels decide window 0's candidate at them (the grid's edges are live)
    i0 = int(np.flatnonzero(ap0 == t0)[0])
    assert ab0[i0] in select_candidates(N, ab0, ap0, A[0][4], float(t0), 1, 0.0, 0.0)[0]
    assert ab0[i0] not in select_candidates(N, ab0, ap0, A[0][4], nxt(t0), 1, 0.0, 0.0)[0]


@pytest.mark.gpu
def test_gpu_truncation_on_several_windows(xc, eng):
    """each window's arrays hold the first max_peaks entries of its own full list (at offset w * max_peaks), and the
    count is the full count"""
    for N, mps in ((4096, (1, 3, 8)), (256, (1, 5))):
        x, _ = make_windows(6, N, seed=31 + N)
        x[2] = 0                                                             # flat: no peak at all
        x[4] = 100 * np.exp(2j * np.pi * 64 * np.arange(N) / N)              # on-bin tone: a few peaks
        rc, full = raw_detect(xc, eng, x, 6, N, N // 2, dist=10, mc=0.0)
        assert rc == 0
        assert full["count"][2] == 0 and full["count"][[0, 1, 3, 5]].min() > max(mps)
        for mp in mps:
            rc, cut = raw_detect(xc, eng, x, 6, N, mp, dist=10, mc=0.0)
            assert rc == 0 and np.array_equal(cut["count"], full["count"]) and np.array_equal(cut["floor"], full["floor"])
            for w in range(6):
                n = min(int(full["count"][w]), mp)
                for k in ("bin", "pw", "snr", "conf"):
                    assert np.array_equal(cut[k][w, :n], full[k][w, :n]), (N, mp, w, k)


@pytest.mark.gpu
@pytest.mark.parametrize("u8", [False, True])
def test_gpu_device_pointer_flags(xc, u8):
    """RMX_IN_DEVICE / RMX_OUT_DEVICE / both, with torch tensors: bit-identical to the host path (count, floor and
    the first min(count, max_peaks) entries; with RMX_OUT_DEVICE nothing past them is written)"""
    import torch
    N, W, MP = 2048, 5, 64
    x, raw = make_windows(W, N, seed=77, u8=u8)
    x[1] = 0.5 + 0.5j                                                        # DC only: no candidate at all
    if u8:
        raw[1] = 128
    host_in = raw if u8 else x
    base = xc.RMX_IN_U8 if u8 else 0
    args = (-70.0, 10, 10e3 * N / 2.4e6, 0.3)
    dev = torch.device("cuda", 0)
    lib = xc.load_library()
    with xc.XcorrEngine(2, 4096, 1) as eng:
        rc, want = raw_detect(xc, eng, host_in, W, N, MP, *args, flags=base)
        assert rc == 0 and want["count"][1] == 0 and want["count"].max() > MP   # truncation is part of the comparison
        eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        d_in = torch.from_numpy(host_in.view(np.uint8).reshape(-1).copy()).to(dev)
        for fl in (xc.RMX_IN_DEVICE, xc.RMX_OUT_DEVICE, xc.RMX_IN_DEVICE | xc.RMX_OUT_DEVICE):
            src = C.c_void_p(d_in.data_ptr()) if fl & xc.RMX_IN_DEVICE else host_in.ctypes.data_as(C.c_void_p)
            if fl & xc.RMX_OUT_DEVICE:
                o = {k: torch.from_numpy(v).to(dev) for k, v in host_outputs(W, MP).items()}
                ptrs = [C.c_void_p(o[k].data_ptr()) for k in OUTS]
            else:
                got = host_outputs(W, MP)
                ptrs = [got[k].ctypes.data_as(C.c_void_p) for k in OUTS]
            torch.cuda.synchronize(dev)
            rc = lib.rmx_detect_batch(eng._ctx, src, W, N, *args, MP, *ptrs, base | fl)
            assert rc == 0, fl
            eng.synchronize()
            if fl & xc.RMX_OUT_DEVICE:
                got = {k: v.cpu().numpy() for k, v in o.items()}
            for k in ("count", "floor"):
                assert want[k].tobytes() == got[k].tobytes(), (u8, fl, k)
            for w in range(W):
                n = min(int(want["count"][w]), MP)
                for k in ("bin", "pw", "snr", "conf"):
                    assert want[k][w, :n].tobytes() == got[k][w, :n].tobytes(), (u8, fl, w, k)
                    if fl & xc.RMX_OUT_DEVICE:
                        assert np.all(got[k][w, n:] == -7), (u8, fl, w, k)


@pytest.mark.gpu
def test_gpu_one_ctx_across_window_lengths(xc):
    """one ctx: detect at 16384 -> 16 -> 2048 (more windows) -> 16384, with correlate calls between (the twiddle table
    and the staging buffers are rebuilt and regrown): every result bit-identical to a fresh engine's"""
    import radio_mapper_amd as rm
    iq_c, _ = rm.synth.make_windows(2, 3, 1024, 10e6, seed=12)
    iq_c = np.ascontiguousarray(iq_c, np.complex64)
    steps = [("d", 16384, 3, False), ("c",), ("d", 16, 5, True), ("d", 2048, 40, False), ("c",), ("d", 16384, 3, True)]
    seq = []
    with xc.XcorrEngine(3, 1024, 2) as e:
        for s in steps:
            if s[0] == "c":
                seq.append(e.correlate(iq_c))
            else:
                x, raw = make_windows(s[2], s[1], seed=40 + s[1], u8=s[3])
                seq.append(e.detect(raw if s[3] else x, distance=7, dc_exclude_bins=3.0, min_confidence=0.1,
                                    max_peaks=s[1] // 4))
    for s, got in zip(steps, seq):
        with xc.XcorrEngine(3, 1024, 2) as f:
            if s[0] == "c":
                want = f.correlate(iq_c)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
            else:
                x, raw = make_windows(s[2], s[1], seed=40 + s[1], u8=s[3])
                want = f.detect(raw if s[3] else x, distance=7, dc_exclude_bins=3.0, min_confidence=0.1,
                                max_peaks=s[1] // 4)
                assert len(got) == len(want) == s[2]
                for g_, w_ in zip(got, want):
                    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(g_, w_)), s


@pytest.mark.gpu
def test_gpu_detect_arguments(xc, eng):
    x, _ = make_windows(2, 64, seed=3)
    big = np.zeros((2, 32768), np.complex64)
    for kw in (dict(dist=0), dict(mp=0), dict(N=8), dict(N=1000), dict(N=32768), dict(W=-1)):
        a = dict(W=2, N=64, mp=8, dist=10)
        a.update(kw)
        rc, _ = raw_detect(xc, eng, big, a["W"], a["N"], a["mp"], dist=a["dist"])
        assert rc == RMX_E_INVAL, kw
    rc, out = raw_detect(xc, eng, x, 0, 64, 8)                                # W = 0: nothing written
    assert rc == 0 and np.all(out["count"] == -7) and np.all(out["bin"] == -7) and np.all(out["floor"] == -7)
    # the wrapper: distance below 1 is refused as scipy refuses it; a fractional one is rounded up; any huge one acts as N
    for d in (0, 0.5, -3, float("nan")):
        with pytest.raises(ValueError):
            eng.detect(x, distance=d)
    e2 = exact_batch(64)[0]
    r = lambda d: [w[0].tolist() for w in eng.detect(e2, distance=d, min_confidence=0.0, max_peaks=32)]  # noqa: E731
    assert r(2.5) == r(3) != r(2)
    assert r(1e12) == r(float("inf")) == r(2**31 - 1) == r(64)
