"""The reference side of the tests of rmx_caf_batch_request (include/rmx.h): the Doppler search under a band, PHAT and lag
bounds, and its sub-grid Doppler estimate.  A float32 restatement, one hypothesis at a time: tests/weighted_ref.py's
weighted_batch on (x_i, rot_mul(x_j, libm_phasor(nu))) -- the weight on both spectra, after the rotation -- then
caf_ref.first_max over the hypotheses' peaks and the S5 parabola over the winner's and its two neighbours' peaks.
The scenes: caf_ref's seeded windows with their true delays, a common DC offset, two emitters in disjoint bands with their
own Doppler offsets, an echo stronger than the direct path, windows whose lags differ.  A helper of
tests/test_caf_request_cpu.py and tests/test_gpu_caf_request.py, not part of the oracle."""
import math

import numpy as np

import caf_ref as cr
import radio_mapper_amd as rm
import weighted_ref as wr
from radio_mapper_amd.xcorr import doppler_estimate

LAG_MARGIN_BAR = 1e-5   # the project's bar on the winner's two largest magnitudes: above it no lag is excused


def pair_array(pairs, n_buoys):
    if pairs is None:
        return np.array([(i, j) for i in range(n_buoys) for j in range(i + 1, n_buoys)], np.int32)
    return np.asarray(pairs, np.int32).reshape(-1, 2)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def bin_results(iq, grid, pairs=None, band=None, phat=False, lag_bounds=None):
    """weighted_batch of every hypothesis of every pair: dict of peak float32, lag_int int32, lag_frac float64, each
    [W][P][D].  x_j is rotated by the table of rmx_caf_batch (caf_ref.libm_phasor) with the kernels' product
    (caf_ref.rot_mul); x_i is not."""
    iq = np.asarray(iq, np.complex64)
    W, B, N = iq.shape
    pl = pair_array(pairs, B)
    grid = np.asarray(grid, np.float64).reshape(-1)
    P, D = len(pl), len(grid)
    lb = None if lag_bounds is None else np.asarray(lag_bounds)
    pk = np.zeros((W, P, D), np.float32)
    li = np.zeros((W, P, D), np.int32)
    lf = np.zeros((W, P, D), np.float64)
    tables = [cr.libm_phasor(nu, N) for nu in grid]
    for q, (i, j) in enumerate(pl.tolist()):
        lbq = None if lb is None else (lb[q:q + 1] if lb.ndim == 2 else lb[:, q:q + 1])
        for d in range(D):
            x = np.stack([iq[:, i], cr.rot_mul(iq[:, j], tables[d])], axis=1)
            a, b, c = wr.weighted_batch(x, band, phat, lbq, pairs=[(0, 1)])[:3]
            li[:, q, d], lf[:, q, d] = a[:, 0], b[:, 0]
            pk[:, q, d] = c[:, 0].astype(np.float32)
            assert np.array_equal(pk[:, q, d].astype(np.float64), c[:, 0])    # the peaks ARE float32 values
    return dict(peak=pk, lag_int=li, lag_frac=lf)


def dop_parabola(peaks, dop):
    """dop_frac of rmx_caf_batch_request: (float32)((a - c) / (2 (a - 2 b + c))) in double from the float32 peaks of
    d* - 1, d*, d* + 1; 0 at d* = 0 and d* = D - 1 (and for a zero denominator, which the first-maximum rule excludes
    between neighbours)."""
    peaks = np.asarray(peaks, np.float32)
    dop = np.asarray(dop)
    D = peaks.shape[-1]
    out = np.zeros(dop.shape, np.float32)
    for idx in np.ndindex(*dop.shape):
        d = int(dop[idx])
        if d == 0 or d == D - 1:
            continue
        a, b, c = (float(peaks[idx + (k,)]) for k in (d - 1, d, d + 1))
        den = 2.0 * (a - 2.0 * b + c)
        out[idx] = np.float32((a - c) / den) if den != 0.0 else np.float32(0)
    return out


def dop_frac_bound(peaks, dop):
    """what one float32 ulp on each of the three taps moves dop_frac (the three-tap one-ulp bound, absolute), [W][P]"""
    peaks = np.asarray(peaks, np.float32)
    D = peaks.shape[-1]
    out = np.zeros(np.asarray(dop).shape)
    for idx in np.ndindex(*out.shape):
        d = int(dop[idx])
        if d == 0 or d == D - 1:
            continue
        a, b, c = (float(peaks[idx + (k,)]) for k in (d - 1, d, d + 1))
        den = a - 2.0 * b + c
        if den == 0.0:
            continue
        ulp = float(np.spacing(np.float32(b)))
        pa = 0.5 * (1.0 / den - (a - c) / den ** 2)
        pb = (a - c) / den ** 2
        pc = 0.5 * (-1.0 / den - (a - c) / den ** 2)
        out[idx] = (abs(pa) + abs(pb) + abs(pc)) * ulp
    return out


def winner_margins(iq, grid, dop, pairs=None, band=None, phat=False, lag_bounds=None):
    """For the winning hypothesis of each pair-window, on its weighted 'full' magnitude vector restricted to the lag
    interval: (relative margin of the two largest values, lag of the second largest, flat-peak bound), each [W][P]"""
    iq = np.asarray(iq, np.complex64)
    W, B, N = iq.shape
    pl = pair_array(pairs, B)
    bd = None if band is None else np.broadcast_to(np.asarray(band, np.float64), (W, 2))
    lb = np.array([[-(N - 1), N - 1]] * len(pl)) if lag_bounds is None else np.asarray(lag_bounds)
    if lb.ndim == 2:
        lb = np.broadcast_to(lb, (W,) + lb.shape)
    mg = np.zeros((W, len(pl)))
    second = np.zeros((W, len(pl)), np.int64)
    flat = np.zeros((W, len(pl)))
    for w in range(W):
        for q, (i, j) in enumerate(pl.tolist()):
            y = cr.rot_mul(iq[w, j], cr.libm_phasor(grid[int(dop[w, q])], N))
            m = wr.weighted_full(iq[w, i], y, None if bd is None else bd[w], phat)
            lo, hi = int(lb[w, q, 0]), int(lb[w, q, 1])
            s = m[lo + N - 1:hi + N]
            k = int(np.argmax(s))
            if len(s) > 1:
                rest = s.copy()
                rest[k] = -1.0
                k2 = int(np.argmax(rest))
                mg[w, q] = float((s[k] - s[k2]) / s[k]) if s[k] > 0 else 0.0
                second[w, q] = k2 + lo
            else:
                mg[w, q], second[w, q] = np.inf, lo
            flat[w, q] = wr.flat_bound(m, N, k + lo, lo, hi)
    return mg, second, flat


def reference(iq, grid, pairs=None, band=None, phat=False, lag_bounds=None):
    """Everything a test compares with, as caf_ref.reference returns it, under the request: dict of dop / dop_frac /
    lag_int / lag_frac / peak [W][P], bin_peak [W][P][D], hyp_margin, lag_margin, lag_second, flat_bound, dop_frac_bound"""
    r = bin_results(iq, grid, pairs, band, phat, lag_bounds)
    pk = r["peak"]
    dop = cr.first_max(pk)
    mg, second, flat = winner_margins(iq, grid, dop, pairs, band, phat, lag_bounds)
    return dict(dop=dop, dop_frac=dop_parabola(pk, dop), lag_int=cr.take(r["lag_int"], dop), lag_frac=cr.take(r["lag_frac"], dop),
                peak=cr.take(pk, dop), bin_peak=pk, hyp_margin=cr.hypothesis_margin(pk), lag_margin=mg, lag_second=second,
                flat_bound=flat, dop_frac_bound=dop_frac_bound(pk, dop))


# ---- the seeded scenes of caf_ref, with their true delays, and the four requests of the route tests --------------------
def scene_of(name):
    """caf_ref.scene_of(name) and the true delays [W][B] of its windows (the generator is seeded: the same windows)"""
    W, B, N, D, seed = cr.SCENES[name]
    iq, raw, grid, k = cr.scene(W, B, N, D, seed)
    iq2, delays = rm.synth.make_windows(W, B, N, 2.4e6, seed=seed, snr_db=10.0, doppler_cps=k * (0.5 / N))[:2]
    assert np.array_equal(iq, iq2)
    return iq, raw, grid, k, delays


def true_lags(delays, pairs):
    """delay(j) - delay(i), float [W][P]"""
    d = np.asarray(delays, np.float64)
    return np.stack([d[:, j] - d[:, i] for i, j in np.asarray(pairs).tolist()], axis=1)


def bounds_around(lags, n_samples, half, per_window):
    """int32 lag intervals that hold the true lags: [W][P][2] = round(lag) +- half per window, or [P][2] = the span of a
    pair's lags over the windows +- half; clipped to [-(N-1), N-1]"""
    r = np.rint(np.asarray(lags)).astype(np.int64)
    lo, hi = (r - half, r + half) if per_window else (r.min(0) - half, r.max(0) + half)
    nm1 = n_samples - 1
    return np.stack([np.clip(lo, -nm1, nm1), np.clip(hi, -nm1, nm1)], -1).astype(np.int32)


BAND = (-0.31, 0.27)   # keeps most of the generator's band (|f| <= 0.4), drops DC-symmetric edges: no edge on a bin centre


def window_bands(n_windows):
    """one band per window, each other than its neighbours', all inside the generator's band"""
    rows = [(-0.31, 0.27), (-0.22, 0.35), (-0.38, 0.12), (-0.05, 0.39), (-0.33, 0.33)]
    return np.array([rows[w % len(rows)] for w in range(n_windows)], np.float64)


def requests(n_windows, n_samples, lags):
    """The four calls of the route tests as (id, keyword arguments of caf() / reference()): PHAT, a band, shared bounds,
    per-window bounds + per-window bands + PHAT.  lags: the true lags [W][P] of the pair list the call is made with."""
    half = max(2, min(8, n_samples // 8))
    return [("phat", dict(whiten=True)),
            ("band", dict(band=np.array(BAND))),
            ("bounds", dict(lag_bounds=bounds_around(lags, n_samples, half, False))),
            ("all", dict(lag_bounds=bounds_around(lags, n_samples, half, True), band=window_bands(n_windows), whiten=True))]


def ref_kwargs(kw):
    """caf()'s keywords -> reference()'s"""
    return dict(band=kw.get("band"), phat=bool(kw.get("whiten", False)), lag_bounds=kw.get("lag_bounds"))


# ---- a common DC offset: the plain search finds nu = 0, lag ~0; PHAT finds the emitter ----------------------------------
DC_DELAYS = {256: (0, 80, 170), 1024: (0, 300, 620), 4096: (0, 1200, 2480)}
DC_STEPS = (0, 1, -1)   # the emitter's frequency offset per buoy, in grid steps


def dc_scene(N, seed=7, dc_over_rms=2.0, D=5):
    """One white emitter delayed per buoy and offset by DC_STEPS grid steps (step 0.5 / N) per buoy, the SAME DC of
    dc_over_rms x rms added to every buoy after the rotation, noise at 0.1 x rms (weighted_ref.dc_offset_scene with a
    frequency offset).  -> (iq [1][3][N], grid [D], true lags [3], true hypotheses [3]) for the default pair list"""
    delays = DC_DELAYS[N]
    rng = np.random.default_rng(seed)
    rms = 20.0
    s = ((rng.standard_normal(4 * N) + 1j * rng.standard_normal(4 * N)) / math.sqrt(2)) * rms
    step = 0.5 / N
    grid = (np.arange(D) - D // 2) * step
    dc = dc_over_rms * rms * np.exp(0.7j)
    n = np.arange(N)
    out = np.zeros((len(delays), N), np.complex64)
    for b, d in enumerate(delays):
        x = s[2 * N - d:2 * N - d + N] * np.exp(2j * np.pi * DC_STEPS[b] * step * n) + dc
        x = x + 0.1 * rms * (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / math.sqrt(2)
        out[b] = x.astype(np.complex64)
    B = len(delays)
    lags = np.array([delays[j] - delays[i] for i in range(B) for j in range(i + 1, B)])
    hyp = np.array([DC_STEPS[j] - DC_STEPS[i] + D // 2 for i in range(B) for j in range(i + 1, B)])
    return out[None], grid, lags, hyp


# ---- two emitters in disjoint bands, each with its own delays and its own frequency offsets ------------------------------
def two_emitter_scene(N, W=1, seed=2, strong_db=20.0, D=5):
    """weighted_ref.two_emitter_scene with a frequency offset per (emitter, buoy), W windows with their own delays.
    -> (iq [W][3][N], grid, lags of the strong emitter [W][3], its hypotheses [3], the weak one's lags, hypotheses)"""
    ka, kb = (0, 1, 2), (2, 0, 1)           # grid steps per buoy: the pairs' differences differ between the emitters
    rng = np.random.default_rng(seed)
    step = 0.5 / N
    grid = (np.arange(D) - D // 2) * step
    n = np.arange(N)
    B = 3
    iq = np.zeros((W, B, N), np.complex64)
    la, lw = np.zeros((W, 3), np.int64), np.zeros((W, 3), np.int64)
    top = max(4, N // 16)
    for w in range(W):
        a = wr.band_signal(rng, 4 * N, *wr.STRONG_BAND) * np.float32(10 ** (strong_db / 20) * 5)
        b = wr.band_signal(rng, 4 * N, *wr.WEAK_BAND) * np.float32(5)
        da = rng.permutation(top)[:B] + w          # distinct delays per window and emitter
        db = rng.permutation(top)[:B] + top
        for k in range(B):
            x = (a[2 * N - da[k]:3 * N - da[k]] * np.exp(2j * np.pi * ka[k] * step * n)
                 + b[2 * N - db[k]:3 * N - db[k]] * np.exp(2j * np.pi * kb[k] * step * n))
            x = x + 0.05 * 5 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
            iq[w, k] = x.astype(np.complex64)
        la[w] = [da[j] - da[i] for i in range(B) for j in range(i + 1, B)]
        lw[w] = [db[j] - db[i] for i in range(B) for j in range(i + 1, B)]
    ha = np.array([ka[j] - ka[i] + D // 2 for i in range(B) for j in range(i + 1, B)])
    hb = np.array([kb[j] - kb[i] + D // 2 for i in range(B) for j in range(i + 1, B)])
    return iq, grid, la, ha, lw, hb


# ---- an echo stronger than the direct path, outside the lag bounds --------------------------------------------------------
def echo_scene(N, W=1, seed=3, D=5, echo_gain=1.6):
    """Buoy 0 hears the emitter directly; buoys 1 and 2 hear it directly and, echo_gain times stronger, N // 4 samples
    later (a reflector near the receiver).  Frequency offsets of (0, 1, -1) grid steps.
    -> (iq [W][3][N], grid, direct lags [W][3], hypotheses [3], bounds [W][3][2] that hold the direct path only)"""
    steps = (0, 1, -1)
    rng = np.random.default_rng(seed)
    step = 0.5 / N
    grid = (np.arange(D) - D // 2) * step
    n = np.arange(N)
    B = 3
    far = N // 4
    iq = np.zeros((W, B, N), np.complex64)
    lags = np.zeros((W, 3), np.int64)
    for w in range(W):
        s = (rng.standard_normal(4 * N) + 1j * rng.standard_normal(4 * N)) / math.sqrt(2) * 20.0
        d = rng.permutation(max(4, N // 16))[:B] + 3 * w
        for k in range(B):
            x = s[2 * N - d[k]:3 * N - d[k]].copy()
            if k > 0:
                x = x + echo_gain * s[2 * N - d[k] - far:3 * N - d[k] - far]
            x = x * np.exp(2j * np.pi * steps[k] * step * n)
            x = x + 2.0 * (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / math.sqrt(2)
            iq[w, k] = x.astype(np.complex64)
        lags[w] = [d[j] - d[i] for i in range(B) for j in range(i + 1, B)]
    hyp = np.array([steps[j] - steps[i] + D // 2 for i in range(B) for j in range(i + 1, B)])
    half = max(3, N // 64)
    return iq, grid, lags, hyp, bounds_around(lags, N, half, True)


# ---- windows whose lags differ: per-window bounds must reach their own window under every hypothesis -------------------
def differing_scene(N, W, B, D, seed):
    """Seeded windows of one emitter with explicit delays: window w's lags are those of window 0 shifted pairwise by
    multiples of 9 samples, so narrow per-window intervals around them are disjoint.  On-grid frequency offsets.
    -> (iq [W][B][N], raw uint8, grid, true lags [W][P] of the default list, hypotheses [W][P])"""
    step = 0.5 / N
    grid = (np.arange(D) - D // 2) * step
    rng = np.random.default_rng(seed)
    k = rng.integers(0, D // 2 + 1, size=(W, B))
    reach = max(1, min(N // 4, 9 * W * B + 8))
    delays = np.array([[9.0 * (w + 1) * b + 0.25 * w - reach / 2 for b in range(B)] for w in range(W)])
    delays = np.clip(delays, -(N - 2) / 2.0, (N - 2) / 2.0)
    iq, _, raw = rm.synth.make_windows(W, B, N, 2.4e6, seed=seed, snr_db=10.0, return_u8=True, doppler_cps=k * step, delays=delays,
                                       max_delay=float(np.abs(delays).max()) + 1.0)
    pl = pair_array(None, B)
    hyp = np.stack([k[:, j] - k[:, i] + D // 2 for i, j in pl.tolist()], axis=1)
    return iq, raw, grid, true_lags(delays, pl), hyp


# ---- the sub-grid Doppler estimate on the reference (float64, numpy): the measurement of DESIGN.md section 5.5 -----------
def subgrid_trial(N, rng, snr_db=20.0, D=9, spacing=0.5, reach=2.5):
    """One pair, offset uniform within +-reach steps of spacing / N cycles per sample, a random whole delay.
    -> (true offset in steps, index-only estimate in steps, parabola estimate in steps), relative to the grid centre"""
    step = spacing / N
    grid = (np.arange(D) - D // 2) * step
    off = rng.uniform(-reach, reach)
    d = int(rng.integers(0, max(2, N // 8)))
    s = (rng.standard_normal(2 * N) + 1j * rng.standard_normal(2 * N)) / math.sqrt(2)
    amp = 10.0 ** (-snr_db / 20.0)
    n = np.arange(N)
    noise = lambda: amp * (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / math.sqrt(2)   # noqa: E731
    x_i = s[N // 2:N // 2 + N] + noise()
    x_j = s[N // 2 - d:N // 2 - d + N] * np.exp(2j * np.pi * off * step * n) + noise()
    Xi = np.fft.fft(x_i, 2 * N)
    peaks = np.zeros(D, np.float32)
    for k, nu in enumerate(grid):
        r = np.fft.ifft(np.fft.fft(x_j * np.exp(-2j * np.pi * nu * n), 2 * N) * np.conj(Xi))
        peaks[k] = np.float32(np.abs(r).max())      # (lag -N, the one circular lag outside 'full', is empty: x is N long)
    dop = cr.first_max(peaks[None, None])
    frac = dop_parabola(peaks[None, None], dop)
    est = doppler_estimate(grid, dop, frac)[0, 0] / step
    return off, float(dop[0, 0] - D // 2), float(est)


# ---- every (scene, pair list, request) the GPU tests hold to the parity rule: name -> loader -----------------------------
# tests/test_caf_request_cpu.py checks the conditions on the inputs of each on the reference alone; tests/test_gpu_caf_request.py
# runs them.  A loader returns (iq, raw or None, grid, pairs or None, caf() keywords); references are computed once per process.
ROUTE_SCENES = ("n16", "n256", "g4096", "n8192", "n8192b6", "one8", "one3", "chunked")
REQUEST_IDS = ("phat", "band", "bounds", "all")
_LOADED, _REFERENCES = {}, {}


def _route_case(name, custom, rid):
    iq, raw, grid, _, delays = _cached(("scene", name), lambda: scene_of(name))
    W, B, N = iq.shape
    pairs = cr.custom_pairs(B) if custom else None
    kw = dict(requests(W, N, true_lags(delays, pair_array(pairs, B))))[rid]
    return iq, raw, grid, pairs, kw


def _differing_case(N, W, what):
    iq, raw, grid, lags, _ = _cached(("differing", N, W), lambda: differing_scene(N, W, 3, 5, seed=900 + N + W))
    kw = dict(lag_bounds=bounds_around(lags, N, 3, True)) if what == "bounds" else dict(band=window_bands(W), whiten=True)
    return iq, raw, grid, None, kw


def _dc_case(N, whiten):
    iq, grid, _, _ = _cached(("dc", N), lambda: dc_scene(N))
    return iq, None, grid, None, dict(whiten=True) if whiten else {}


def _cached(key, make):
    if key not in _LOADED:
        _LOADED[key] = make()
        for a in _LOADED[key]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _LOADED[key]


CASES = {}
for _n in ROUTE_SCENES:
    for _c in (False, True):
        for _r in REQUEST_IDS:
            CASES["%s/%s/%s" % (_n, "custom" if _c else "default", _r)] = (lambda n=_n, c=_c, r=_r: _route_case(n, c, r))
for _N, _W in ((4096, 3), (256, 5), (8192, 5)):
    for _what in ("bounds", "bands"):
        CASES["differing%d/%s" % (_N, _what)] = (lambda N=_N, W=_W, what=_what: _differing_case(N, W, what))
for _N in (256, 4096):
    CASES["dc%d/plain" % _N] = (lambda N=_N: _dc_case(N, False))
    CASES["dc%d/phat" % _N] = (lambda N=_N: _dc_case(N, True))


def case(name):
    return CASES[name]()


def case_reference(name):
    """reference() of a case, computed once and left unchanged"""
    if name not in _REFERENCES:
        iq, _, grid, pairs, kw = case(name)
        ref = reference(iq, grid, pairs, **ref_kwargs(kw))
        for a in ref.values():
            a.setflags(write=False)
        _REFERENCES[name] = ref
    return _REFERENCES[name]
