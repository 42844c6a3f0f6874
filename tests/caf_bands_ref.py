"""The reference side of the tests of rmx_caf_batch_bands (include/rmx.h): the Doppler search under several bands per window.
Slot (w, m, q) is, by definition, slot (w, q) of rmx_caf_batch_request with band[w][m], so the reference stacks
caf_request_ref.reference per band.  The scenes hold one emitter per band, each with its own delays and its own frequency
offsets per (window, buoy): the winning hypothesis and the lag then differ between the bands of a window and between the
slots of a call, and a kernel that read another band's or another hypothesis' operand cannot pass.  A helper of
tests/test_caf_bands_cpu.py and tests/test_gpu_caf_bands.py, not part of the oracle."""
import numpy as np

import caf_ref as cr
import caf_request_ref as rr
import weighted_ref as wr

LAG_MARGIN_BAR = rr.LAG_MARGIN_BAR   # on the lag margin AND the hypothesis margin of every slot: none is excused
OUT_KEYS = ("dop", "dop_frac", "lag_int", "lag_frac", "peak", "hyp_margin", "lag_margin", "lag_second", "flat_bound", "dop_frac_bound")

# one emitter per band (cycles per sample), disjoint, with gaps that the per-window jitter below never closes
EMITTER_BANDS = ((0.05, 0.17), (-0.31, -0.19), (0.24, 0.38))


def per_window(bands, n_windows):
    """bands [M][2] (shared) or [W][M][2] -> float64 [W][M][2]"""
    b = np.asarray(bands, np.float64)
    if b.ndim == 2:
        b = np.broadcast_to(b, (n_windows,) + b.shape)
    assert b.shape[0] == n_windows and b.shape[2] == 2, b.shape
    return b


def reference(iq, grid, bands, pairs=None, phat=False, lag_bounds=None):
    """caf_request_ref.reference per band, stacked: dict of OUT_KEYS, each [W][M][P], and bin_peak [W][M][P][D].  lag_bounds:
    None, [P][2] or [W][P][2] -- per (window, pair), shared by the window's bands and hypotheses."""
    b = per_window(bands, np.asarray(iq).shape[0])
    per_band = [rr.reference(iq, grid, pairs, band=b[:, m], phat=phat, lag_bounds=lag_bounds) for m in range(b.shape[1])]
    return {k: np.stack([r[k] for r in per_band], axis=1) for k in OUT_KEYS + ("bin_peak",)}


# ---- the scenes: one emitter per band ------------------------------------------------------------------------------------------
def scene(W, B, N, D, seed, n_emitters=3):
    """W windows of B buoys; emitter e lives in EMITTER_BANDS[e], reaches buoy b of window w delayed by a whole d[e][w][b]
    samples and offset by k[e][w][b] grid steps (step 0.5 / N, k in 0 .. D // 2: every pair's difference is a grid point).
    Quantised to the uint8 grid, as synth.make_windows does.
    -> (iq complex64 [W][B][N], raw uint8 [W][B][2N] that decodes to iq, grid [D], true lags [E][W][P] and true hypotheses
    [E][W][P] of the default pair list)"""
    step = 0.5 / N
    grid = (np.arange(D) - D // 2) * step
    rng = np.random.default_rng(seed)
    n = np.arange(N)
    top = max(B + 1, N // 16)
    E = n_emitters
    k = rng.integers(0, D // 2 + 1, size=(E, W, B))
    d = np.zeros((E, W, B), np.int64)
    x = np.zeros((W, B, N), np.complex128)
    for w in range(W):
        for e in range(E):
            s = wr.band_signal(rng, 4 * N, *EMITTER_BANDS[e]).astype(np.complex128) * (14.0 + 3.0 * e)
            d[e, w] = rng.permutation(top)[:B]
            for b in range(B):
                x[w, b] += s[2 * N - d[e, w, b]:3 * N - d[e, w, b]] * np.exp(2j * np.pi * k[e, w, b] * step * n)
        x[w] += 1.5 * (rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N)))
    re = np.clip(np.floor(x.real + 128.0), 0, 255).astype(np.uint8)
    im = np.clip(np.floor(x.imag + 128.0), 0, 255).astype(np.uint8)
    iq = ((re.astype(np.float32) - np.float32(127.5)) + 1j * (im.astype(np.float32) - np.float32(127.5))).astype(np.complex64)
    raw = np.empty((W, B, 2 * N), np.uint8)
    raw[..., 0::2] = re
    raw[..., 1::2] = im
    pl = rr.pair_array(None, B)
    lags = np.stack([d[:, :, j] - d[:, :, i] for i, j in pl.tolist()], axis=-1)
    hyp = np.stack([k[:, :, j] - k[:, :, i] + D // 2 for i, j in pl.tolist()], axis=-1)
    return iq, raw, grid, lags, hyp


def band_set(M, W=None):
    """M bands, one per emitter 0 .. M - 1: [M][2] shared by every window (W None), or [W][M][2] where column m holds
    emitter (m + w) mod 3's band, its edges moved outwards by 0.001 (w + 1): a different band in every window"""
    if W is None:
        return np.array(EMITTER_BANDS[:M], np.float64)
    out = np.zeros((W, M, 2))
    for w in range(W):
        for m in range(M):
            lo, hi = EMITTER_BANDS[(m + w) % 3]
            out[w, m] = (lo - 0.001 * (w + 1), hi + 0.001 * (w + 1))
    return out


def emitter_of(M, W, per_window_bands):
    """[W][M]: the emitter that column m of window w keeps (band_set)"""
    return np.array([[(m + w) % 3 if per_window_bands else m for m in range(M)] for w in range(W)])


def pair_lags(lags, pairs, n_buoys):
    """true lags of the default list [E][W][P] -> those of `pairs` (None: as they are); a reversed pair changes sign"""
    if pairs is None:
        return lags
    index = {tuple(p): q for q, p in enumerate(rr.pair_array(None, n_buoys).tolist())}
    cols = []
    for i, j in np.asarray(pairs).tolist():
        cols.append(lags[..., index[(i, j)]] if i < j else -lags[..., index[(j, i)]])
    return np.stack(cols, axis=-1)


def bounds_holding(lags, n_samples, half=3):
    """int32 [W][P][2]: per (window, pair) the interval that holds every emitter's true lag, +- half -- shared by the window's
    bands, as the entry shares it"""
    lo, hi = lags.min(axis=0) - half, lags.max(axis=0) + half
    nm1 = n_samples - 1
    return np.stack([np.clip(lo, -nm1, nm1), np.clip(hi, -nm1, nm1)], -1).astype(np.int32)


# ---- every (scene, pair list, bands, request) the GPU tests run: name -> loader; references computed once --------------------------
ROUTE_SCENES = ("n16", "n256", "g4096", "n8192", "n8192b6", "one8", "one3", "chunked", "seam256", "seam8192")
REQUEST_IDS = ("none", "phat", "bounds", "phat+bounds")
_LOADED, _REFERENCES = {}, {}


def _cached(key, make):
    if key not in _LOADED:
        _LOADED[key] = make()
        for a in _LOADED[key]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _LOADED[key]


def scene_of(name):
    W, B, N, D, seed = cr.SCENES[name]
    return _cached(("scene", name), lambda: scene(W, B, N, D, seed))


def case(name):
    """"<scene>/<default|custom>/<M>/<shared|perwin>/<request>" -> (iq, raw, grid, pairs or None, bands, caf_bands() keywords)"""
    sc, pl, M, form, rid = name.split("/")
    iq, raw, grid, lags, _ = scene_of(sc)
    W, B, N = iq.shape
    pairs = cr.custom_pairs(B) if pl == "custom" else None
    bands = band_set(int(M), W if form == "perwin" else None)
    kw = {}
    if "phat" in rid:
        kw["whiten"] = True
    if "bounds" in rid:
        kw["lag_bounds"] = bounds_holding(pair_lags(lags, pairs, B), N)
    return iq, raw, grid, pairs, bands, kw


def case_reference(name):
    """reference() of a case, computed once and left unchanged"""
    if name not in _REFERENCES:
        iq, _, grid, pairs, bands, kw = case(name)
        ref = reference(iq, grid, bands, pairs, phat=bool(kw.get("whiten")), lag_bounds=kw.get("lag_bounds"))
        for a in ref.values():
            a.setflags(write=False)
        _REFERENCES[name] = ref
    return _REFERENCES[name]


# the cases held to the reference (every other combination of a route is held, bit for bit, to the single-band calls, which
# tests/test_gpu_caf_request.py holds to the same reference): both pair lists under the hardest request, and the plain one
REFERENCE_CASES = ["%s/%s" % (sc, tail) for sc in ROUTE_SCENES
                   for tail in ("default/3/perwin/phat+bounds", "custom/3/perwin/phat+bounds", "default/2/shared/none")]
# four-step, 6 buoys, the default list: the single-band call takes g_rows_anchor there, so these are held to the reference alone
# -- all 16 combinations of M, the bands' form and the request
ANCHOR_CASES = ["n8192b6/default/%d/%s/%s" % (M, form, rid) for M in (2, 3) for form in ("shared", "perwin") for rid in REQUEST_IDS]


# ---- windows whose lags differ: per-window bands and bounds must reach their own (window, band) ------------------------------------
def one_bin_bands(N, W, M):
    """[W][M][2]: band (w, m) keeps exactly ONE bin of the 2N-point transform, a different one for every (w, m), all inside
    the generator's band"""
    L = 2 * N
    out = np.zeros((W, M, 2))
    for w in range(W):
        for m in range(M):
            s = (L // 16) * (1 + m) + 3 * w + 1 if m % 2 == 0 else -((L // 16) * (1 + m) + 5 * w + 2)
            out[w, m] = ((s - 0.25) / L, (s + 0.25) / L)
    return out


def differing_case(N, W, M):
    """caf_request_ref.differing_scene (one wide emitter, window w's lags disjoint from its neighbours') under bands that
    differ in every window and narrow per-window bounds -> (iq, raw, grid, bands [W][M][2], bounds [W][P][2])"""
    iq, raw, grid, lags, _ = _cached(("differing", N, W), lambda: rr.differing_scene(N, W, 3, 5, seed=900 + N + W))
    rows = [(-0.31, 0.27), (-0.22, 0.35), (-0.38, 0.12), (-0.05, 0.39), (-0.33, 0.33), (-0.12, 0.30), (-0.36, 0.02)]
    bands = np.array([[rows[(2 * w + 3 * m) % len(rows)] for m in range(M)] for w in range(W)], np.float64)
    bands[..., 0] -= 0.0007 * np.arange(W)[:, None]
    return iq, raw, grid, bands, rr.bounds_around(lags, N, 3, True)
