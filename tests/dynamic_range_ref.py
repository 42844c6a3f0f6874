"""Inputs at other levels than rtl_sdr's +-127.5, and what a correct kernel must return for them
(tests/test_gpu_dynamic_range.py, tests/test_dynamic_range_cpu.py).  numpy only, no GPU.

Scaling an input by an exact power of two commutes with every IEEE add, multiply, fma and (even exponent) square root as
long as nothing overflows or goes subnormal.  So with every (window, buoy) scaled by its own 2^e[w, b] a correct float32
implementation returns, for pair (i, j) of window w,

    lag_int, lag_frac   the bits of the unscaled call          peak   ldexp(peak of the unscaled call, e[w, i] + e[w, j]).

  exponents          seeded e [W][B] in -20 ... +14 with the ends, the mixed pair and loud / quiet neighbours forced;
  scaled             the input at those levels, exact (ldexp);
  expect_peak        the peak row a correct kernel returns;
  scene              seeded windows at three levels -- the uint8 grid, +-1 floats (full 24-bit mantissas) and int16-scaled
                     floats -- with their float64 reference (far_lag_ref.ref64_batch);
  coherent_window    the constant window (127.5 + 127.5j) 2^k and its analytic result: the top of the range.

Why these ends: +14 puts the largest sample of the uint8 grid (|127.5 + 127.5j| = 180.3) at 2.95e6, inside the 4e6 that
include/rmx.h states for N = 4096; -7 and +8 are the +-1 float and the int16 conventions; -20 lies far below both, and the
float32 oracle stays in range there (test_dynamic_range_cpu.py)."""
import functools

import numpy as np

import far_lag_ref as F
import radio_mapper_amd as rm

E_LO, E_HI = -20, 14


def exponents(W, B, seed):
    """int64 [W][B], seeded uniform in E_LO ... E_HI, with these slots forced (W >= 5, B >= 2 holds them all):
      window 0   all zero: every call contains its own unscaled control;
      window 1   buoys 0, 1 at (E_LO, E_HI): the mixed pair (its mirror through a custom list);
      window 2   all E_HI: every pair at (E_HI, E_HI);
      window 3   all E_LO: every pair at (E_LO, E_LO), directly behind the loud window;
      window 4   all E_HI: the loud window directly behind the quiet one
    (a persistent workgroup runs consecutive windows).  Fewer windows keep what fits: W = 2 ... 4 keep the first W of these
    with window 1 = (E_LO, E_LO, E_HI, E_HI, seeded ...) cut to B; W = 1 is (E_LO, E_HI, seeded ...)."""
    assert W >= 1 and B >= 2
    e = np.random.default_rng(seed).integers(E_LO, E_HI + 1, size=(W, B)).astype(np.int64)
    if W == 1:
        e[0, :2] = (E_LO, E_HI)
        return e
    e[0] = 0
    if W < 5:
        row = np.array([E_LO, E_LO, E_HI, E_HI])[:B]
        e[1, :len(row)] = row
    else:
        e[1, :2] = (E_LO, E_HI)
    for w, v in ((2, E_HI), (3, E_LO), (4, E_HI)):
        if w < W:
            e[w] = v
    return e


def scaled(iq, e):
    """complex64 [W][B][N] with window w of buoy b multiplied by 2^e[w, b]: exact (ldexp on both parts)"""
    iq = np.asarray(iq, np.complex64)
    e = np.asarray(e, np.int64)
    assert e.shape == iq.shape[:2], (e.shape, iq.shape)
    out = np.empty(iq.shape, np.complex64)
    out.real = np.ldexp(iq.real, e[:, :, None])
    out.imag = np.ldexp(iq.imag, e[:, :, None])
    assert np.all(np.isfinite(out.view(np.float32)))
    return out


def expect_peak(peak0, e, pairs):
    """float32 [rows][P]: ldexp(peak0, e_i + e_j) per pair (i, j); e [rows][B]"""
    p = np.asarray(pairs).reshape(-1, 2)
    e = np.asarray(e, np.int64)
    peak0 = np.asarray(peak0, np.float32)
    assert peak0.shape == (e.shape[0], len(p)), (peak0.shape, e.shape, len(p))
    return np.ldexp(peak0, (e[:, p[:, 0]] + e[:, p[:, 1]]).astype(np.int32)).astype(np.float32)


def custom_pairs(B):
    """a pair, its mirror, a self pair and the pair of the two outer buoys"""
    return np.array([(0, 1), (1, 0), (1, 1), (B - 1, 0)], np.int32)


# ---- scenes -----------------------------------------------------------------------------------------------------------------
LEVELS = ("u8grid", "unit", "int16")
MARGIN = 1e-3              # the top-two margin test_far_lag_ref_cpu.py demands of its scenes


def windows_for(N):
    """the smallest batch that reaches every kernel of a length: 8 windows up to N = 16384, 2 at 65536, 1 at 2^20"""
    return 8 if N <= 16384 else 2 if N <= 65536 else 1


def _raw_scene(N, B, W, seed, quantise):
    """make_windows at 10 dB with every delay inside +-noise_top / 4 (every pair's lag inside +-noise_top / 2: the overlap
    carries the peak with a margin at every length)"""
    iq, _ = rm.synth.make_windows(W, B, N, F.FS, seed, quantise=quantise, max_delay=min(F.noise_top(N) / 4.0, 800.0))
    return iq


def _levels(N, B, W, seed):
    raw = _raw_scene(N, B, W, seed, False)
    assert np.abs(raw.view(np.float32)).max() <= 127.5
    return {"u8grid": _raw_scene(N, B, W, seed, True), "unit": (raw / np.float32(127.5)).astype(np.complex64),
            "int16": (raw * np.float32(257.0)).astype(np.complex64)}


@functools.lru_cache(maxsize=None)
def _scenes(N, B, W):
    """the three levels of one seed, the first of 7100 + N mod 1009 + 16 B (+ 1000, + 2000, ...) at which every slot of
    every level -- default and custom list -- has a top-two margin of MARGIN (a true lag half way between two samples
    makes a near tie of its neighbours: one window in a few hundred)"""
    pairs = np.array([(i, j) for i in range(B) for j in range(i + 1, B)], np.int32)
    custom = custom_pairs(B)
    for attempt in range(16):
        out = {}
        for level, iq in _levels(N, B, W, 7100 + N % 1009 + 16 * B + 1000 * attempt).items():
            iq.setflags(write=False)
            out[level] = dict(iq=iq, pairs=pairs, ref=F.ref64_batch(iq, pairs), custom=custom, cref=F.ref64_batch(iq, custom))
        if min(min(s["ref"][3].min(), s["cref"][3].min()) for s in out.values()) >= MARGIN:
            return out
    raise AssertionError("no seed with a margin for N = %d, B = %d, W = %d" % (N, B, W))


def scene(N, B, W, level="u8grid"):
    """dict(iq complex64 [W][B][N], pairs = the default list, ref = far_lag_ref.ref64_batch on it, custom, cref = the same
    for custom_pairs(B)).
      u8grid   make_windows as every other test uses it: 8 significant bits, rms 32;
      unit     make_windows(quantise=False) / 127.5: a non-power-of-two normalisation to +-1 that fills all 24 bits
               (quantise=False still clips to +-127.5, so the level is what it says);
      int16    the same unquantised data times 257.0: +-32767.5, the int16 convention, 24-bit mantissas."""
    return _scenes(N, B, W)[level]


def mantissa_bits(iq):
    """the largest number of significant bits among the samples' parts (24 = a full float32 mantissa)"""
    v = np.asarray(iq).view(np.float32).ravel()
    m, _ = np.frexp(v[v != 0])
    k = np.round(np.abs(m).astype(np.float64) * (1 << 24)).astype(np.int64)      # 24-bit integer mantissa
    low = k & -k                                                                  # lowest set bit
    return int(24 - np.log2(low.min()))


def coherent_window(N, k):
    """the constant window a = (127.5 + 127.5j) 2^k (every sample at the corner of the uint8 grid, fully coherent: the
    largest correlation a level allows) and its analytic self correlation: (x complex64 [N], lag_int 0, lag_frac 0.0,
    peak N |a|^2 float64).  The 'full' correlation is the triangle (N - |lag|) |a|^2: the parabola through lags -1, 0, 1 has
    its vertex at 0 exactly."""
    a = np.ldexp(np.float32(127.5), k)
    x = np.full(N, complex(a, a), np.complex64)
    return x, 0, 0.0, float(N) * 2.0 * float(a) ** 2
