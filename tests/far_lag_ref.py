"""Scenes whose correlation peak lies ANYWHERE in the lag range, and their float64 reference (tests/test_gpu_far_lags.py,
tests/test_far_lag_ref_cpu.py).  numpy only, no GPU.

The seeded generator keeps every buoy's delay inside +-50 km / c, so the parity tests only ever find a peak in the central
+-800 lags (2.4 MS/s) of the +-(N - 1) the kernels search.  Every peak-search kernel splits those 2N - 1 lags over
threads, waves, halves, quarters, tiles and rows; here the winning lag is put on every such seam, next to it, and
everywhere else:

  target_lags   the lags a route must find: 0, +-1, +-2^k (-1, +1), +-m N/8 (-1, +1), +-top, 32 seeded ones and the seam
                lags of the routes of that length (SEAMS);
  noise_scene   realistic windows (synth.make_windows, 10 dB, uint8 grid) whose true lag is target + u, |u| < 0.5;
  multi_scene   B >= 3 buoys with delays spread over +-(7/16) N (every pair's lag anywhere in +-7/8 N);
  impulse_scene single impulses: the reference is analytic, and the lags up to +-(N - 1) fit;
  ref64         IFFT_L(FFT_L(x_j) conj(FFT_L(x_i))) in complex128, 'full' order: lag_int, the header's three-point parabola
                on the float64 magnitudes, the peak, and the relative margin between the two largest magnitudes.
"""
import functools

import numpy as np

import radio_mapper_amd as rm

FS = 2.4e6


def top_lag(N):
    """largest |lag| of the target list: N - N/8 (the impulse scene adds +-(N - 2) and +-(N - 1))"""
    return N - N // 8


def noise_top(N):
    """largest |lag| of the noise scenes: top_lag(N) = N - N/8 leaves an overlap of N/8 samples, which carries the peak from
    N = 4096 on (smallest margin 0.005 measured at 10 dB).  Shorter windows need a longer overlap for the coherent
    peak (0.9 x overlap) to stand 1e-3 clear of the largest of 2N noise lags (about sqrt(2 N ln 2N)): N = 2048 and 1024
    keep N/4, N = 256 keeps N/2.  The impulse scene carries the whole target list, and +-(N - 1), at every length."""
    return {256: 128, 1024: 768, 2048: 1536}.get(N, top_lag(N))


# ---- seam lags ------------------------------------------------------------------------------------------------------
# Where a lag's owner changes, or a parabola tap m[k -+ 1] comes from somewhere else, in the search of each route (read
# off the kernels; tests/test_gpu_far_lags.py repeats the list per route).  Positive lag l sits at circular index l,
# negative lag l at l + L (L = 2N); every kernel's split is a split of that circular index, so one list of strides per
# length describes them: a seam lies at every multiple of the stride (the lag that starts a piece) and one below it (the
# lag that ends the previous piece), on either side of zero.
#   k_win, k_fwd + k_pair (N = 4096), k_win8kl (8192), k16_pairs (16384): index n = l mod 4096 is held by thread
#     2 (n mod 256) + half, register slot n / 256: waves change every 32 lags, slots every 256; k_win8kl's bin-parity
#     halves change at +-4096, k16_pairs' residue quarters at +-4096, +-8192 and +-12288; the negative and the positive
#     lags are the two lanes of a pair (seam -1 / 0).
#   g_pair_small, g_win_fused, g_win_scr, g_win_scr14, g_win_eo15: thread tid takes the indices tid + e x threads (threads =
#     L / 16 ... 1024), the taps come out of the LDS image by circular index: the seams are the waves (every 64 lags), the
#     register slots (every `threads` lags) and the wrap between index L - 1 and 0 (lags -1 / 0); g_win_eo15's two
#     half-length transforms change at lag +-8192 (index 8192 / 24576).
#   four-step (g_cols_inv + g_final, behind g_rows_fused / g_rows_inv / g_rows_anchor): index = row x L2 + column, a tile
#     holds 8 ... 32 columns of every row: tiles change every 8 / 16 / 32 lags (the tap then comes from the halo of the
#     next tile), rows every L2 lags (the tap comes from the last tile's halo of the previous row).
STRIDES = {
    256: (8, 16, 32, 64),
    1024: (8, 16, 32, 64, 128, 256),
    2048: (8, 16, 32, 64, 256, 1024),
    4096: (32, 64, 256, 512, 1024),
    8192: (8, 16, 32, 64, 256, 1024, 4096),
    16384: (8, 16, 32, 64, 256, 1024, 2048, 4096, 8192),
    65536: (8, 16, 32, 64, 1024, 2048),
    1 << 20: (),
}


def seam_lags(N, seed):
    """For every stride s of STRIDES[N]: the first multiple, the last one below top, a multiple in the far half of the
    range that is NO multiple of 2 s (so it is a seam of this stride and not of the next), and one seeded multiple, each
    with the lag below it, on both sides of zero."""
    top, rng, out = top_lag(N), np.random.default_rng(seed + 7), set()
    for s in STRIDES[N]:
        n = top // s                       # multiples 1 .. n lie inside +-top
        if n < 1:
            continue
        far = n if n % 2 else n - 1        # odd multiple nearest the top
        picks = {1, n, max(far, 1), int(rng.integers(1, n + 1)), (n // 2) | 1 if (n // 2) | 1 <= n else 1}
        for m in picks:
            for sign in (1, -1):
                for d in (-1, 0, 1):
                    out.add(sign * m * s + d)
    return sorted(l for l in out if abs(l) <= top)


def target_lags(N, seed):
    """The lags every route of length N must find (sorted, unique, inside +-top_lag(N))."""
    top, rng = top_lag(N), np.random.default_rng(seed)
    lags = {0, 1, -1, top, -top}
    k = 1
    while (1 << k) < top:
        for d in (-1, 0, 1):
            lags.update(((1 << k) + d, -(1 << k) - d))
        k += 1
    for m in range(1, 8):
        for d in (-1, 0, 1):
            lags.update((m * N // 8 + d, -(m * N // 8) - d))
    lags.update(int(v) for v in rng.integers(-top, top + 1, size=32))
    lags.update(seam_lags(N, seed))
    return np.array(sorted(l for l in lags if abs(l) <= top), np.int64)


# ---- the float64 reference ------------------------------------------------------------------------------------------
def ref64(x_i, x_j):
    """(lag_int, lag_frac, peak, margin) of one pair: r = IFFT_L(FFT_L(x_j) conj(FFT_L(x_i))) in complex128, L = 2N, in
    'full' order; argmax of |r| (lowest index on a tie), the header's parabola 0.5 (a - c) / (a - 2 b + c) on the float64
    taps (0 at the two ends and on a flat top), and margin = (largest - second largest) / largest."""
    x_i, x_j = np.asarray(x_i, np.complex128), np.asarray(x_j, np.complex128)
    n = x_i.shape[-1]
    L = 2 * n
    r = np.fft.ifft(np.fft.fft(x_j, L) * np.conj(np.fft.fft(x_i, L)))
    m = np.abs(np.concatenate([r[L - (n - 1):], r[:n]]))
    k = int(np.argmax(m))
    frac = 0.0
    if 0 < k < 2 * n - 2:
        den = m[k - 1] - 2.0 * m[k] + m[k + 1]
        if den != 0.0:
            frac = 0.5 * (m[k - 1] - m[k + 1]) / den
    b = float(m[k])
    second = max(m[:k].max(initial=0.0), m[k + 1:].max(initial=0.0))
    return k - (n - 1), float(frac), b, (b - second) / b if b > 0 else 0.0


def ref64_batch(iq, pairs):
    """ref64 for every (window, pair): lag_int int64 [W][P], lag_frac, peak, margin float64 [W][P]; one FFT per buoy."""
    iq = np.asarray(iq)
    W, B, n = iq.shape
    pairs = np.asarray(pairs).reshape(-1, 2)
    L, P = 2 * n, len(pairs)
    li, lf = np.zeros((W, P), np.int64), np.zeros((W, P))
    pk, mg = np.zeros((W, P)), np.zeros((W, P))
    for w in range(W):
        spec = np.fft.fft(iq[w].astype(np.complex128), L, axis=-1)
        for q, (i, j) in enumerate(pairs):
            r = np.fft.ifft(spec[j] * np.conj(spec[i]))
            m = np.abs(np.concatenate([r[L - (n - 1):], r[:n]]))
            k = int(np.argmax(m))
            if 0 < k < 2 * n - 2:
                den = m[k - 1] - 2.0 * m[k] + m[k + 1]
                lf[w, q] = 0.5 * (m[k - 1] - m[k + 1]) / den if den != 0.0 else 0.0
            b = m[k]
            m[k] = -1.0
            li[w, q], pk[w, q], mg[w, q] = k - (n - 1), b, (b - m.max()) / b if b > 0 else 0.0
    return li, lf, pk, mg


def mirrored(pairs):
    """each pair followed by its mirror (j, i): both signs of every lag through the custom-list kernels"""
    p = np.asarray(pairs, np.int32).reshape(-1, 2)
    return np.stack([p, p[:, ::-1]], axis=1).reshape(-1, 2).copy()


# ---- scenes ---------------------------------------------------------------------------------------------------------
def noise_scene(N, lags, seed, repeat=1, doppler_cps=None):
    """One two-buoy window per lag: delays (-t/2, +t/2), t = lag + u, u seeded uniform in (-0.5, 0.5).  repeat = K: K
    consecutive windows per lag with the SAME delays and their own source and noise (the groups of an integrated call).
    doppler_cps [W][2]: per-buoy frequency offsets (the Doppler search).  Returns (iq complex64 [W][2][N], raw uint8
    [W][2][2N], true lag float64 [W])."""
    lags = np.asarray(lags, np.float64)
    u = np.random.default_rng(seed + 1).uniform(-0.5, 0.5, size=lags.shape)
    t = np.repeat(lags + u, repeat)
    d = np.stack([-t / 2.0, t / 2.0], axis=1)
    iq, _, raw = rm.synth.make_windows(len(t), 2, N, FS, seed, max_delay=(N - 2) / 2.0, delays=d, return_u8=True,
                                       doppler_cps=doppler_cps)
    return iq, raw, t


def multi_scene(N, B, W, seed, doppler_cps=None):
    """W windows of B >= 3 buoys, delays seeded uniform in +-noise_top(N) / 2 (= +-(7/16) N from N = 4096 on): every
    pair's lag anywhere in +-noise_top.  Returns (iq, raw, delays [W][B])."""
    half = noise_top(N) / 2.0
    d = np.random.default_rng(seed + 2).uniform(-half, half, size=(W, B))
    iq, _, raw = rm.synth.make_windows(W, B, N, FS, seed, max_delay=(N - 2) / 2.0, delays=d, return_u8=True,
                                       doppler_cps=doppler_cps)
    return iq, raw, d


def impulse_scene(N, lags, B, seed):
    """x_0 = A d[p], x_b = C_b d[p + lag_b]: the sorted lags in groups of B - 1 per window, p chosen so that every impulse
    of the group lies inside the window (a group is cut where its lags span more than N - 1; an unfilled group repeats its
    last lag).  |A|, |C_b| in 1 ... 3 with seeded phases.  Returns (iq complex64 [W][B][N], pos int64 [W][B], amp float64
    [W][B]): for EVERY ordered pair (i, j) the correlation is the single sample A_j conj(A_i) at lag pos_j - pos_i, so
    lag_int = pos_j - pos_i exactly, peak = |A_i| |A_j|, and the neighbour taps are round-off: |lag_frac| <= 1e-5."""
    lags = sorted(int(l) for l in lags)
    assert all(abs(l) <= N - 1 for l in lags)
    groups, cur = [], []
    for l in lags:
        if cur and (len(cur) == B - 1 or max(l, 0) - min(cur[0], 0) > N - 1):
            groups.append(cur)
            cur = []
        cur.append(l)
    groups.append(cur)
    rng = np.random.default_rng(seed + 3)
    W = len(groups)
    iq = np.zeros((W, B, N), np.complex64)
    pos = np.zeros((W, B), np.int64)
    amp = np.zeros((W, B))
    for w, g in enumerate(groups):
        g = g + [g[-1]] * (B - 1 - len(g))
        lo, hi = min(min(g), 0), max(max(g), 0)
        assert hi - lo <= N - 1
        p = int(rng.integers(-lo, N - hi))             # -lo <= p <= N - 1 - hi
        pos[w] = [p] + [p + l for l in g]
        amp[w] = rng.uniform(1.0, 3.0, size=B)
        ph = np.exp(2j * np.pi * rng.random(B))
        iq[w, np.arange(B), pos[w]] = (amp[w] * ph).astype(np.complex64)
    return iq, pos, amp


def impulse_ref(pos, amp, pairs):
    """the analytic (lag_int [W][P], peak [W][P]) of an impulse scene for a pair list"""
    p = np.asarray(pairs).reshape(-1, 2)
    return pos[:, p[:, 1]] - pos[:, p[:, 0]], amp[:, p[:, 1]] * amp[:, p[:, 0]]


# ---- the scenes of one window length, built once and shared by every route of that length -----------------------------
SEED = 20260


def scene_lags(N):
    """the lags of the two-buoy noise scene: the target list inside +-noise_top(N); at N = 65536 every third of them with 0,
    +-1 and +-top (a window costs 0.1 s to make and to reference; the impulse scene keeps the whole list); at N = 2^20 two
    windows, one lag next to each end of +-top (a window is 8 MiB, its reference four transforms of 2^21 points)"""
    if N == 1 << 20:
        top = top_lag(N)
        return np.array([-(top - 3), top - 5], np.int64)
    t = target_lags(N, SEED + N % 1009)
    if N >= 65536:
        t = np.union1d(t[::3], [-top_lag(N), -1, 0, 1, top_lag(N)])
    return t[np.abs(t) <= noise_top(N)]


def impulse_lags(N):
    """the lags of the impulse scene: the whole target list and the four lags at the two ends of the range"""
    if N == 1 << 20:
        return np.array([-(N - 1), N - 2], np.int64)
    return np.union1d(target_lags(N, SEED + N % 1009), [-(N - 1), -(N - 2), N - 2, N - 1])


@functools.lru_cache(maxsize=None)
def two_buoy(N):
    """dict(iq, raw, lags, true, ref = (lag_int, lag_frac, peak, margin) [W] of pair (0, 1), rev = those of pair (1, 0)).
    With u up to half a sample the two middle taps of a window can come within 1e-3 of each other, or the noise can move
    the float64 peak to the neighbouring lag (a few windows in two hundred): such a window is drawn again from the next
    seed (noise and u), until every slot carries its lag with a margin of 1e-3."""
    lags = scene_lags(N)
    iq, raw, t = noise_scene(N, lags, SEED + N % 1009)
    ref = list(ref64_batch(iq, [(0, 1), (1, 0)]))
    for attempt in range(1, 9):
        bad = np.nonzero((ref[0][:, 0] != lags) | (ref[0][:, 1] != -lags) | (ref[3].min(axis=1) < 1e-3))[0]
        if not len(bad):
            break
        iq[bad], raw[bad], t[bad] = noise_scene(N, lags[bad], SEED + N % 1009 + 1000 * attempt)
        for a, b in zip(ref, ref64_batch(iq[bad], [(0, 1), (1, 0)])):
            a[bad] = b
    for a in (iq, raw):
        a.setflags(write=False)
    return dict(iq=iq, raw=raw, lags=lags, true=t, ref=tuple(a[:, 0] for a in ref), rev=tuple(a[:, 1] for a in ref))


def pack(x, B):
    """Two-buoy windows x [W][2][...] as windows of B buoys: window v holds the two-buoy windows (B // 2) v + g as its buoys
    (2 g, 2 g + 1) (the last ones repeated to fill the last window; an odd B gets a copy of buoy 0 as its last buoy), so
    that an engine of B buoys finds every designed lag at a pair (2 g, 2 g + 1) of its default list -- the other pairs
    correlate unrelated windows and are not looked at.  Returns (packed [V][B][...], src int [V][B // 2]: the two-buoy
    window behind each designed pair)."""
    W, G = x.shape[0], B // 2
    V = (W + G - 1) // G
    src = np.minimum(np.arange(V * G), W - 1).reshape(V, G)
    out = np.empty((V, B) + x.shape[2:], x.dtype)
    for g in range(G):
        out[:, 2 * g] = x[src[:, g], 0]
        out[:, 2 * g + 1] = x[src[:, g], 1]
    if B % 2:
        out[:, B - 1] = out[:, 0]
    return out, src


def designed_pairs(B):
    """the pairs (2 g, 2 g + 1) of pack(), and their columns in the default pair list of B buoys"""
    dflt = [(i, j) for i in range(B) for j in range(i + 1, B)]
    des = [(2 * g, 2 * g + 1) for g in range(B // 2)]
    return np.array(des, np.int32), np.array([dflt.index(p) for p in des])


@functools.lru_cache(maxsize=None)
def multi_buoy(N, B):
    """dict(iq, raw, delays, pairs = every pair of the default list followed by its mirror, ref = ref64 of those); windows
    enough for two dozen pairs"""
    P = B * (B - 1) // 2
    iq, raw, d = multi_scene(N, B, max(2, -(-24 // P)), SEED + 31 + N % 1009 + B)
    for a in (iq, raw):
        a.setflags(write=False)
    pairs = mirrored([(i, j) for i in range(B) for j in range(i + 1, B)])
    return dict(iq=iq, raw=raw, delays=d, pairs=pairs, ref=ref64_batch(iq, pairs))
