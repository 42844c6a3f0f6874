"""Every lag and every bin of a correlation, in float64 (tests/test_gpu_every_lag.py, tests/test_gpu_every_bin.py,
tests/test_full_vector_cpu.py).  numpy only, no GPU.

The other references of this directory return a correlation's WINNER.  Here the whole 'full'-order magnitude vector is
the reference, so that a one-lag interval [k, k] -- which returns lag_int = k, lag_frac = 0, peak = m[k] by the sliced
rule of include/rmx.h -- reads out any one of its 2N - 1 values, and a one-bin band [s / L, s / L] reads out any one of
the L products |X_j[s]| |X_i[s]| / L.

  full64        |IFFT_L(FFT_L(x_j) conj(FFT_L(x_i)))| in complex128, 'full' order, as far_lag_ref.ref64 forms it; with a
                band and / or PHAT (weighted_ref's rule in complex128)
  integrated64  the root-sum-square of full64 over a group of windows (integrated_ref's rule in float64)
  derotated64   full64 with x_j de-rotated by one Doppler hypothesis (the exact phasor in double)
  spectra64, bin_product
  scenes        per length: a 10 dB emitter and a noise-only scene, two buoys and two distinct windows each, on the uint8 grid
  vectors       the float64 reference of a scene, once per distinct (window, ordered buoy pair)
  lag_plan, bin_plan   which lag / bin every output slot of a GPU call probes: pure functions, so that the CPU test proves
                the coverage the GPU tests claim
"""
import functools

import numpy as np

import far_lag_ref as F
import radio_mapper_amd as rm

FS = 2.4e6
SEED = 48611

# the bar of a value INSIDE a vector (tests/test_gpu_lag_bounds.py: _assert_sliced; include/rmx.h, the weighted entry)
REL, VEC = 1e-5, 1e-6


def bar(value, vec_max):
    """|got - value| must not exceed this: 1e-5 of the value + 1e-6 of the largest value of its vector"""
    return REL * np.asarray(value, np.float64) + VEC * np.asarray(vec_max, np.float64)


# ---- the float64 reference ------------------------------------------------------------------------------------------
def spectra64(x):
    """FFT_L of the zero-padded window(s), L = 2N, complex128 (along the last axis)"""
    x = np.asarray(x, np.complex128)
    return np.fft.fft(x, 2 * x.shape[-1], axis=-1)


def bin_product(X_i, X_j, s):
    """|X_j[s mod L]| |X_i[s mod L]| / L for the signed bin(s) s: the peak of the one-bin band [s / L, s / L]"""
    L = X_i.shape[-1]
    k = np.asarray(s, np.int64) % L
    return np.abs(X_j[..., k]) * np.abs(X_i[..., k]) / L


def kept(lo, hi, n_samples):
    """bool [L] over the natural bins: the signed bins s in [-N, N - 1] with lo <= s / L <= hi (include/rmx.h; 0.5 is bin
    N, which -N stands for: clamped to N - 1)"""
    L = 2 * n_samples
    s = np.arange(L)
    s = np.where(s < n_samples, s, s - L)
    s_lo = max(int(np.ceil(lo * L)), -n_samples)
    s_hi = min(int(np.floor(hi * L)), n_samples - 1)
    return (s >= s_lo) & (s <= s_hi)


def weighted_spectrum64(x, band=None, phat=False):
    """Y = M X, or M X / |X| under PHAT (0 where X == 0), complex128 [L]"""
    X = spectra64(x)
    if phat:
        a = np.abs(X)
        X = np.where(a > 0, X / np.where(a > 0, a, 1.0), 0.0)
    if band is not None:
        X = np.where(kept(float(band[0]), float(band[1]), np.asarray(x).shape[-1]), X, 0.0)
    return X


def full_of_spectra(Y_i, Y_j):
    """|IFFT_L(Y_j conj(Y_i))| in 'full' order: lag l at index l + N - 1, float64 [2N - 1]"""
    L = Y_i.shape[-1]
    n = L // 2
    r = np.fft.ifft(Y_j * np.conj(Y_i))
    return np.abs(np.concatenate([r[L - (n - 1):], r[:n]]))


def full64(x_i, x_j, band=None, phat=False):
    """the 'full'-order magnitudes of one pair, float64 [2N - 1] (band [lo, hi] in cycles per sample, PHAT)"""
    return full_of_spectra(weighted_spectrum64(x_i, band, phat), weighted_spectrum64(x_j, band, phat))


def integrated64(group_i, group_j, band=None, phat=False):
    """m = sqrt(sum_w |c_w|^2) over the K windows group_i[w], group_j[w] of one group, float64 [2N - 1]"""
    s = 0.0
    for x_i, x_j in zip(group_i, group_j):
        s = s + full64(x_i, x_j, band, phat) ** 2
    return np.sqrt(s)


def derotated64(x_i, x_j, nu, band=None, phat=False):
    """full64 with x_j de-rotated by the hypothesis nu (cycles per sample): x_j[n] exp(-2 pi i nu n), as rmx_caf_batch
    rotates it before the transform (the weight is applied after the rotation)"""
    n = np.arange(np.asarray(x_j).shape[-1])
    return full64(x_i, np.asarray(x_j, np.complex128) * np.exp(-2j * np.pi * float(nu) * n), band, phat)


# ---- scenes ---------------------------------------------------------------------------------------------------------
SCENES = ("emitter", "noise")


@functools.lru_cache(maxsize=None)
def scenes(N):
    """{"emitter": (iq, raw), "noise": (iq, raw)}: iq complex64 [2][2][N] -- two distinct windows of two buoys --, raw the
    uint8 [2][2][2N] that decodes to exactly iq.  The emitter is the generator's 10 dB scene with delays inside +-40
    samples; the noise scene has no common source (the generator at -200 dB): its correlation has no peak, every value
    is a few times the rms -- the hard case for an absolute bar."""
    out = {}
    for name, snr, seed in (("emitter", 10.0, SEED + N % 1009), ("noise", -200.0, SEED + 500 + N % 1009)):
        iq, _, raw = rm.synth.make_windows(2, 2, N, FS, seed, snr_db=snr, max_delay=40.0, return_u8=True)
        for a in (iq, raw):
            a.setflags(write=False)
        out[name] = (iq, raw)
    return out


def tile(x, n_windows, n_buoys):
    """[2][2][...] -> [W][B][...]: window w is distinct window w % 2, buoy b is scene buoy b % 2"""
    x = np.asarray(x)
    return np.ascontiguousarray(x[np.arange(n_windows)[:, None] % 2, np.arange(n_buoys)[None, :] % 2])


def combo(pairs):
    """the scene's ordered buoy pair behind each pair of a list over tiled buoys: 2 (i % 2) + (j % 2); 1 is the order
    (0, 1), 2 its mirror (1, 0), 0 and 3 the two autocorrelations"""
    p = np.asarray(pairs).reshape(-1, 2)
    return 2 * (p[:, 0] % 2) + (p[:, 1] % 2)


# slot kinds of lag_plan
ORDER01, MIRROR10, OTHER = 0, 1, 2
_KIND_OF_COMBO = np.array([OTHER, ORDER01, MIRROR10, OTHER])


def kinds_of(pairs, n_windows):
    """the slot kinds [W * P] (window-major) of a call over tiled windows and buoys"""
    return np.tile(_KIND_OF_COMBO[combo(pairs)], n_windows)


@functools.lru_cache(maxsize=None)
def vectors(N, scene, band=None, phat=False):
    """float64 [2][4][2N - 1]: full64 of distinct window w and combo c (the ordered scene pair (c // 2, c % 2)), once"""
    iq = scenes(N)[scene][0]
    out = np.empty((2, 4, 2 * N - 1))
    for w in range(2):
        Y = [weighted_spectrum64(iq[w, b], band, phat) for b in range(2)]
        for c in range(4):
            out[w, c] = full_of_spectra(Y[c // 2], Y[c % 2])
    out.setflags(write=False)
    return out


def slot_reference(m, lags, pairs, n_windows):
    """(m[k], max of m) of every slot [W][P] of a tiled call: m = vectors(...), lags [W][P] (or [P], shared)"""
    c = combo(pairs)
    N = (m.shape[-1] + 1) // 2
    lags = np.broadcast_to(np.asarray(lags), (n_windows, len(c)))
    w = np.arange(n_windows)[:, None] % 2
    return m[w, c[None, :], lags + N - 1], m.max(axis=-1)[w, c[None, :]]


# ---- coverage planners ----------------------------------------------------------------------------------------------
def seams(N, seed=SEED):
    """far_lag_ref.seam_lags where far_lag_ref.STRIDES knows the length, else nothing"""
    return list(F.seam_lags(N, seed)) if N in F.STRIDES else []


def _ends(N):
    return [-(N - 1), -(N - 2), N - 2, N - 1]


def mirror_lags(N, seed=SEED):
    """the lags an exhaustive plan also probes under the mirror (1, 0): every seam lag and +-1 around it, and the four
    lags at the two ends of the range; every lag where the length has no seam list (N = 16)"""
    if N not in F.STRIDES:
        return np.arange(-(N - 1), N)
    out = set(_ends(N))
    for l in seams(N, seed):
        out.update((l - 1, l, l + 1))
    return np.array(sorted(l for l in out if abs(l) <= N - 1), np.int64)


def sampled_lags(N, seed=SEED):
    """the lags a sampled plan probes under BOTH orders: the seam lags, 0, +-1, +-(N - 2), +-(N - 1)"""
    out = set(seams(N, seed)) | {0, 1, -1} | set(_ends(N))
    return np.array(sorted(out), np.int64)


N_SEEDED_LAGS = 2048


def seeded_lags(N, seed=SEED):
    return np.random.default_rng(seed + 11 + N).integers(-(N - 1), N, size=N_SEEDED_LAGS)


def lag_plan(N, slots, exhaustive, seed=SEED):
    """The lag probed by each output slot.  slots: the kind of every slot, int [S] of ORDER01 / MIRROR10 / OTHER (kinds_of).
    Exhaustive: every lag of +-(N - 1) on an ORDER01 slot, mirror_lags on MIRROR10 slots; sampled: sampled_lags on both,
    and 2048 seeded lags on what is left.  The slots left over walk the range again from a seeded start.  ValueError when
    the slots do not hold the plan."""
    kinds = np.asarray(slots).reshape(-1)
    every = np.arange(-(N - 1), N)
    want0 = every if exhaustive else sampled_lags(N, seed)
    want1 = mirror_lags(N, seed) if exhaustive else sampled_lags(N, seed)
    i0, i1 = np.flatnonzero(kinds == ORDER01), np.flatnonzero(kinds == MIRROR10)
    if len(i0) < len(want0) or len(i1) < len(want1):
        raise ValueError("%d / %d slots of the two orders for %d / %d lags" % (len(i0), len(i1), len(want0), len(want1)))
    lags = np.zeros(len(kinds), np.int64)
    used = np.zeros(len(kinds), bool)
    lags[i0[:len(want0)]], lags[i1[:len(want1)]] = want0, want1
    used[i0[:len(want0)]] = used[i1[:len(want1)]] = True
    rest = np.flatnonzero(~used)
    fill = np.zeros(0, np.int64)
    if not exhaustive:
        fill = seeded_lags(N, seed)
        if len(rest) < len(fill):
            raise ValueError("%d slots left for %d seeded lags" % (len(rest), len(fill)))
    more = len(rest) - len(fill)
    start = int(np.random.default_rng(seed + 13 + N).integers(0, len(every)))
    lags[rest] = np.concatenate([fill, every[(start + 7 * np.arange(more)) % len(every)]])
    return lags


def pair_list(n_pairs, every):
    """a custom list over two buoys: (0, 1), with every `every`-th pair the mirror (1, 0) (every = 2: alternating)"""
    p = np.tile(np.array([[0, 1]], np.int32), (n_pairs, 1))
    p[every - 1::every] = (1, 0)
    return p


N_SEEDED_BINS = 1024


def default_l1(N):
    """the column length the library picks for the four-step split L = L1 x L2 (rmx_hip.hip: generic_init)"""
    logL = int(np.log2(2 * N))
    l1 = 8 if logL == 18 else (logL - 3) // 2
    return 1 << min(max(l1, logL - 13), 10)


def _signed(k, N):
    k = np.asarray(k, np.int64) % (2 * N)
    return np.where(k < N, k, k - 2 * N)


def rows_sweep(N, L1):
    """four-step layout (natural bin k1 + L1 k2, xbin_rows): every k1 at two fixed k2, every k2 at two fixed k1"""
    L2 = 2 * N // L1
    k1, k2 = np.arange(L1), np.arange(L2)
    out = [k1 + L1 * f for f in (3 % L2, L2 - 2)] + [f + L1 * k2 for f in (1 % L1, L1 - 3)]
    return np.unique(_signed(np.concatenate(out), N))


def kfwd_sweep(N=4096):
    """k_fwd's layout (RMX_XBIN_KFWD: bin = 2 (k0 + 16 k1 + 256 slot) + p): every slot, k0, k1 and parity at two fixed
    values of the others"""
    assert N == 4096
    out = []
    r = np.arange(16)
    for a, b, p in ((5, 9, 0), (12, 2, 1)):
        out += [2 * (a + 16 * b + 256 * r) + p, 2 * (r + 16 * a + 256 * b) + p, 2 * (a + 16 * r + 256 * b) + p]
        out += [2 * (a + 16 * b + 256 * 7) + np.arange(2)]
    return np.unique(_signed(np.concatenate(out), N))


def bin_plan(N, exhaustive, layout=None, seed=SEED):
    """The signed bins s in [-N, N - 1] a sweep probes, sorted.  Exhaustive: all L.  Sampled: -N, -1, 0, 1, N - 1, both
    neighbours of every power of two on both signs, 1024 seeded bins, and the structure sweep of the layout: None,
    "kfwd", or ("rows", L1)."""
    if exhaustive:
        return np.arange(-N, N)
    out = {-N, -1, 0, 1, N - 1}
    k = 1
    while (1 << k) <= N:
        out.update(((1 << k) - 1, (1 << k) + 1, -(1 << k) - 1, -(1 << k) + 1))
        k += 1
    out.update(int(v) for v in np.random.default_rng(seed + 17 + N).integers(-N, N, size=N_SEEDED_BINS))
    if layout == "kfwd":
        out.update(int(v) for v in kfwd_sweep(N))
    elif layout is not None:
        out.update(int(v) for v in rows_sweep(N, int(layout[1])))
    return np.array(sorted(s for s in out if -N <= s <= N - 1), np.int64)


def one_bin_bands(bins, N):
    """[..., 2] float64: the band [s / L, s / L] of every signed bin (exact: L is a power of two)"""
    s = np.asarray(bins, np.float64) / (2 * N)
    return np.stack([s, s], axis=-1)
