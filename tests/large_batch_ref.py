"""Batches whose byte offsets, element indices and slot counts leave the range the small shapes use (numpy only, no GPU):
tests/test_gpu_large_batches.py runs them, tests/test_large_batch_ref_cpu.py shows that their comparison has teeth.

Periodic scenes.  A batch of W windows is T distinct base windows repeated: window w is base window w % T (T an odd prime,
7, or 5 where the float64 reference is slow), taken from far_lag_ref.multi_scene, so every pair's lag lies anywhere in the
range.  The expected value of slot (w, q) is the float64 reference of base window w % T -- never a second call of the
engine.  With integrate = K the group g holds windows g K ... g K + K - 1 of that map, base windows (g K + k) % T: T
distinct groups, group g being reference group g % T.

What a narrow address does to such a batch (wrong_rule).  A kernel that kept a byte offset in 32 bits, or an element index
in a signed 32-bit integer, would read unit u of a buffer -- a window of the input, a window's spectra, a slot's products --
at the wrapped offset: another unit, the middle of one, or nothing of the buffer at all.  On the index map alone that says
which base window the wrong read lands on, and the comparison reports it unless that window is the SAME base window: the
shift is 2^32 / (bytes per unit) units, a power of two wherever the unit's size is one, and no power of two is a multiple
of an odd prime.  T = 8 would hide every such wrap (test_large_batch_ref_cpu.py shows that too).

boundary_plan gives the smallest batch whose last 64 windows lie wholly beyond byte 2^32 of a buffer and names the windows
that straddle 2^31 and 2^32: the windows a failure message should point at."""
import functools

import numpy as np

import far_lag_ref as F

TAIL = 64            # windows that must lie wholly beyond byte 2^32
RULES = ("byte offset in uint32", "byte offset in int32", "element index in int32")
SEED = F.SEED + 4000


# ---- the index map ---------------------------------------------------------------------------------------------------
def window_map(n_windows, T):
    """base window of every window of the batch"""
    return np.arange(n_windows) % T


def group_members(T, K):
    """[T][K]: the base windows of the T distinct groups of an integrated call (group g of the batch is row g % T)"""
    return (np.arange(T)[:, None] * K + np.arange(K)[None, :]) % T


def group_scene(base, K):
    """the T distinct groups as a batch of T K windows, for the float64 helpers that take integrate = K"""
    return np.ascontiguousarray(base[group_members(len(base), K).ravel()])


def expand(ref, rows, T):
    """a reference over the T base windows (or groups): arrays [T][...] (a tuple or a dict of them) -> [rows][...]"""
    idx = np.arange(rows) % T
    if isinstance(ref, dict):
        return {k: np.asarray(v)[idx] for k, v in ref.items()}
    return tuple(np.asarray(a)[idx] for a in ref)


# ---- where a buffer crosses 2^31 and 2^32 bytes -----------------------------------------------------------------------
def boundary_plan(bytes_per_window, elem_size=8, tail=TAIL):
    """bytes_per_window of one buffer (of a slot, a spectrum set, ...: any unit that is laid out back to back) -> dict:
    windows     the smallest count whose last `tail` units lie wholly beyond byte 2^32
    straddle31  the units that hold byte 2^31 (one, or two neighbours when 2^31 is a unit's first byte: the unit that ends
                there and the one that begins there)
    straddle32  the same for byte 2^32
    elem31      the unit that holds ELEMENT index 2^31 (elem_size bytes each), or None when the batch ends before it"""
    bpw = int(bytes_per_window)
    assert bpw > 0 and elem_size > 0 and bpw % elem_size == 0
    first_beyond = -(-(1 << 32) // bpw)          # the first unit that begins at or beyond byte 2^32
    W = first_beyond + tail

    def at(byte):
        u = byte // bpw
        return [u - 1, u] if byte % bpw == 0 else [u]

    e31 = (elem_size << 31) // bpw
    return dict(windows=W, bytes_per_window=bpw, total_bytes=W * bpw, first_beyond=first_beyond, straddle31=at(1 << 31),
                straddle32=at(1 << 32), elem31=e31 if e31 < W else None)


def case_plan(c):
    """boundary_plan of a case's buffer at the case's own size: W * upw units"""
    p = boundary_plan(c["unit_bytes"], c["elem"], 0)
    n = c["W"] * c["upw"]
    p.update(windows=n, total_bytes=n * c["unit_bytes"], elem31=p["elem31"] if p["elem31"] is not None and p["elem31"] < n else None)
    return p


def describe(plan):
    return ("%d units of %d bytes (%.2f GiB); byte 2^31 in unit %s, byte 2^32 in unit %s, units %d ... %d wholly beyond it"
            % (plan["windows"], plan["bytes_per_window"], plan["total_bytes"] / 2.0 ** 30, plan["straddle31"], plan["straddle32"],
               plan["first_beyond"], plan["windows"] - 1))


# ---- the three wrong address rules, on the index map alone ------------------------------------------------------------
RIGHT, OTHER, TORN, OUTSIDE = 0, 1, 2, 3   # the unit itself / another whole unit / parts of two units / not in the buffer


def _wrap(rule, byte, elem_size):
    byte = np.asarray(byte, np.int64)
    if rule == RULES[0]:
        return byte & 0xFFFFFFFF
    if rule == RULES[1]:
        return ((byte + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    if rule == RULES[2]:
        return (((byte // elem_size + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)) * elem_size
    raise ValueError(rule)


def wrong_rule(rule, bytes_per_unit, elem_size, n_units):
    """what a kernel under `rule` reads for every unit u of a buffer of n_units back-to-back units: (kind [n_units] of
    RIGHT / OTHER / TORN / OUTSIDE, unit [n_units]: the unit the first element comes from, -1 for OUTSIDE).  The first and
    the last element of the unit are followed: a unit whose two ends wrap differently is TORN."""
    bpu = int(bytes_per_unit)
    u = np.arange(n_units, dtype=np.int64)
    first, last = u * bpu, u * bpu + bpu - elem_size
    a, b = _wrap(rule, first, elem_size), _wrap(rule, last, elem_size)
    total = n_units * bpu
    kind = np.full(n_units, OTHER)
    src = a // bpu
    kind[(a % bpu != 0) | (b - a != bpu - elem_size)] = TORN
    kind[(a < 0) | (b < 0) | (a >= total) | (b >= total)] = OUTSIDE
    kind[(a == first) & (b == last)] = RIGHT
    src[kind == OUTSIDE] = -1
    return kind, src


def reported(rule, bytes_per_unit, elem_size, n_windows, T, units_per_window=1, lags=None):
    """bool [n_windows]: the windows whose comparison fails when the buffer is addressed by `rule`.  A unit read from
    outside the buffer or torn between two units is garbage (or a fault): reported.  A unit read whole from another unit is
    reported when that unit holds something else: another base window (lags None), or -- lags int [T][units_per_window],
    the reference's integer lag of every slot -- a slot with another lag."""
    n_units = n_windows * units_per_window
    kind, src = wrong_rule(rule, bytes_per_unit, elem_size, n_units)
    u = np.arange(n_units)
    w, s = u // units_per_window, u % units_per_window
    ws, ss = np.maximum(src, 0) // units_per_window, np.maximum(src, 0) % units_per_window
    if lags is None:
        differs = (ws % T != w % T) | (ss != s)
    else:
        lags = np.asarray(lags)
        differs = lags[ws % T, ss] != lags[w % T, s]
    bad = (kind == TORN) | (kind == OUTSIDE) | ((kind == OTHER) & differs)
    return bad.reshape(n_windows, units_per_window).any(axis=1)


def wrapped(rule, bytes_per_unit, elem_size, n_windows, units_per_window=1):
    """bool [n_windows]: the windows of which `rule` misreads at least one unit"""
    kind, _ = wrong_rule(rule, bytes_per_unit, elem_size, n_windows * units_per_window)
    return (kind != RIGHT).reshape(n_windows, units_per_window).any(axis=1)


# ---- the matrix of tests/test_gpu_large_batches.py ---------------------------------------------------------------------
def _case(cid, N, B, W, T, buffer, unit_bytes, elem, upw=1, planned=True, P=None):
    """unit_bytes: bytes of one unit of the buffer under test; upw units per window; planned: W is boundary_plan's count
    for that buffer (else the issue's shape, checked to cross 2^32 with its last TAIL windows beyond)"""
    return dict(id=cid, N=N, B=B, W=W, T=T, buffer=buffer, unit_bytes=unit_bytes, elem=elem, upw=upw, planned=planned,
                P=B * (B - 1) // 2 if P is None else P)


def _input(cid, N, B, T=7, u8=False):
    bpw = B * N * (2 if u8 else 8)
    return _case(cid, N, B, boundary_plan(bpw, 1 if u8 else 8)["windows"], T, "uint8 input" if u8 else "complex64 input", bpw,
                 1 if u8 else 8)


CASES = {c["id"]: c for c in [
    _input("I1", 4096, 8),                                    # k_win, k_win_lb
    _input("I2", 4096, 8, u8=True),                           # k_win<U8>: sample index 2^31
    _input("I3", 8192, 8),                                    # k_win8kl
    _input("I4", 16384, 8),                                   # k16_fwd + k16_pairs
    _input("I5-g_win_fused", 2048, 4),                        # (g_win_fused takes at most four buoys)
    _input("I5-g_win_scr", 2048, 16),
    _input("I5-g_win_scr14", 8192, 8),
    _input("I5-g_win_eo15", 16384, 8),
    _input("I6", 1024, 16),                                   # g_fwd_small + g_pair_small<LagBounds>, chunk seams
    _input("I7", 65536, 3),                                   # four-step, gen_chunk 256
    _input("I8", 4096, 8),                                    # I1 through the host door
    # library scratch inside one chunk: d_spec (64 KiB per stored spectrum), the de-rotated set, g_spec, g_prod
    _case("S1", 4096, 20, 4096, 5, "d_spec", 20 * 65536, 16, planned=False),
    _case("S2", 4096, 20, 4096, 5, "d_spec_r", 20 * 65536, 16, planned=False),
    _case("S3", 65536, 8, 600, 7, "g_spec", 8 * 131072 * 8, 8, planned=False, P=2),
    _case("S4", 8192, 16, 546, 7, "g_prod", 16384 * 8, 8, upw=120, planned=False),   # (546 windows: the chunk of 560)
]}


@functools.lru_cache(maxsize=None)
def base_scene(N, B, T, seed=SEED, doppler=False):
    """(iq complex64 [T][B][N], raw uint8 [T][B][2N], k): T base windows with every pair's lag anywhere in +-noise_top(N).
    doppler: every buoy offset by k [T][B] in {0, 1} steps of 2 / N cycles per sample (the Doppler search: every pair's
    difference is a point of the grid caf_grid(N))."""
    k = np.random.default_rng(seed + N + B).integers(0, 2, size=(T, B)) if doppler else None
    iq, raw, _ = F.multi_scene(N, B, T, seed + N % 1009 + B, doppler_cps=None if k is None else k * (2.0 / N))
    for a in (iq, raw):
        a.setflags(write=False)
    return iq, raw, k


def caf_grid(N):
    return (np.arange(3) - 1) * (2.0 / N)


def distinct(lag_int):
    """any two base windows (rows of lag_int [T][P]) differ in the integer lag of at least one pair"""
    li = np.asarray(lag_int)
    return all((li[a] != li[b]).any() for a in range(len(li)) for b in range(a + 1, len(li)))
