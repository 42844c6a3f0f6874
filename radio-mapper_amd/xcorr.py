"""ctypes binding of the C-ABI library (include/rmx.h) -- the only compute path of this package.

There is no CPU fallback here: if ``librmx_hip.so`` is missing or no MI355X is visible the
constructor raises.  (The CPU oracle lives in ``oracle/`` and is test infrastructure only.)
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "librmx_hip.so"
LIB_PATH = os.path.join(_HERE, "csrc", LIB_NAME)

RMX_IN_DEVICE = 1
RMX_OUT_DEVICE = 2
RMX_IN_U8 = 4
_DEVICE = RMX_IN_DEVICE | RMX_OUT_DEVICE

RMX_WEIGHT_NONE = 0
RMX_WEIGHT_PHAT = 1

# quality[..., RMX_Q_*] of correlate(quality=True) (rmx_xcorr_batch_quality)
RMX_Q_COHERENCE = 0
RMX_Q_PSR = 1
RMX_Q_RMS_BW = 2
RMX_Q_NEFF = 3

_lib = None


class RmxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rmx error {code}: {msg}")
        self.code = code


def library_path() -> str:
    return os.environ.get("RMX_LIBRARY", LIB_PATH)


def load_library():
    """dlopen the HIP library (once).  torch, when importable, is imported first so that this
    library binds to the same libamdhip64 as torch (device pointers and streams are shared)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(hipcc --offload-arch=gfx950); there is no CPU fallback")
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(path)
    vp, ci, cu = C.c_void_p, C.c_int, C.c_uint
    lib.rmx_version.restype = ci
    lib.rmx_device_count.restype = ci
    lib.rmx_create.argtypes = [C.POINTER(vp), ci, ci, ci, ci, cu]
    lib.rmx_create.restype = ci
    lib.rmx_destroy.argtypes = [vp]
    lib.rmx_destroy.restype = None
    lib.rmx_last_error.argtypes = [vp]
    lib.rmx_last_error.restype = C.c_char_p
    lib.rmx_set_stream.argtypes = [vp, vp]
    lib.rmx_set_stream.restype = ci
    lib.rmx_set_option.argtypes = [vp, C.c_char_p, C.c_long]
    lib.rmx_set_option.restype = ci
    lib.rmx_set_default_option.argtypes = [C.c_char_p, C.c_long]
    lib.rmx_set_default_option.restype = ci
    lib.rmx_clear_default_options.argtypes = []
    lib.rmx_clear_default_options.restype = None
    lib.rmx_xcorr_batch.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, cu]
    lib.rmx_xcorr_batch.restype = ci
    lib.rmx_xcorr_batch_bounded.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, cu]
    lib.rmx_xcorr_batch_bounded.restype = ci
    lib.rmx_xcorr_batch_weighted.argtypes = [vp, vp, ci, vp, ci, vp, ci, cu, vp, ci, vp, vp, vp, cu]
    lib.rmx_xcorr_batch_weighted.restype = ci
    lib.rmx_xcorr_batch_bands.argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, cu, vp, ci, vp, vp, vp, cu]
    lib.rmx_xcorr_batch_bands.restype = ci
    lib.rmx_xcorr_batch_integrated.argtypes = [vp, vp, ci, vp, ci, ci, vp, ci, cu, vp, ci, vp, vp, vp, cu]
    lib.rmx_xcorr_batch_integrated.restype = ci
    lib.rmx_xcorr_batch_refined.argtypes = [vp, vp, ci, vp, ci, ci, vp, ci, cu, vp, ci, ci, vp, vp, vp, cu]
    lib.rmx_xcorr_batch_refined.restype = ci
    lib.rmx_xcorr_batch_quality.argtypes = [vp, vp, ci, vp, ci, ci, vp, ci, cu, vp, ci, ci, vp, vp, vp, vp, cu]
    lib.rmx_xcorr_batch_quality.restype = ci
    lib.rmx_xcorr_batch_bands_quality.argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, cu, vp, ci, ci, vp, vp, vp, vp, cu]
    lib.rmx_xcorr_batch_bands_quality.restype = ci
    lib.rmx_xcorr_batch_bands_integrated.argtypes = [vp, vp, ci, vp, ci, ci, vp, ci, ci, cu, vp, ci, ci, vp, vp, vp, vp, cu]
    lib.rmx_xcorr_batch_bands_integrated.restype = ci
    lib.rmx_caf_batch.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, cu]
    lib.rmx_caf_batch.restype = ci
    lib.rmx_caf_batch_request.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, ci, cu, vp, ci, vp, vp, vp, vp, vp, cu]
    lib.rmx_caf_batch_request.restype = ci
    lib.rmx_caf_batch_quality.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, ci, cu, vp, ci, ci, vp, vp, vp, vp, vp, vp, cu]
    lib.rmx_caf_batch_quality.restype = ci
    lib.rmx_caf_batch_integrated.argtypes = [vp, vp, ci, vp, ci, vp, ci, ci, vp, ci, cu, vp, ci, ci, vp, vp, vp, vp, vp, vp, cu]
    lib.rmx_caf_batch_integrated.restype = ci
    lib.rmx_caf_batch_bands.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, ci, ci, cu, vp, ci, vp, vp, vp, vp, vp, cu]
    lib.rmx_caf_batch_bands.restype = ci
    lib.rmx_solve_batch.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, C.c_double, ci, ci, vp, vp, vp, cu]
    lib.rmx_solve_batch.restype = ci
    lib.rmx_solve_batch_fix.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, C.c_double, vp, ci, ci, vp, vp, vp, vp, vp, vp, cu]
    lib.rmx_solve_batch_fix.restype = ci
    lib.rmx_detect_batch.argtypes = [vp, vp, ci, ci, C.c_float, ci, C.c_double, C.c_float, ci, vp, vp, vp, vp, vp, vp, cu]
    lib.rmx_detect_batch.restype = ci
    lib.rmx_synchronize.argtypes = [vp]
    lib.rmx_synchronize.restype = ci
    lib.rmx_last_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(ci), C.POINTER(C.c_float),
                                    C.POINTER(ci)]
    lib.rmx_last_timing.restype = ci
    lib.rmx_last_timing_kind.argtypes = [vp, ci, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(ci)]
    lib.rmx_last_timing_kind.restype = ci
    lib.rmx_build_info.argtypes = []
    lib.rmx_build_info.restype = C.c_char_p
    lib.rmx_scratch_bytes.argtypes = [vp]
    lib.rmx_scratch_bytes.restype = C.c_size_t
    _lib = lib
    return lib


def check_lag_bounds(lag_bounds, n_windows: int, n_pairs: int):
    """lag_bounds as correlate() takes it -> (contiguous int32 array or None, per_window).  Shape [P][2] (shared by every
    window) or [W][P][2]; an integer dtype.  Raises ValueError before any call into the library; the values themselves
    (-(N-1) <= lo <= hi <= N-1) are checked by the library (RmxError, RMX_E_INVAL)."""
    if lag_bounds is None:
        return None, False
    a = np.asarray(lag_bounds)
    if a.dtype.kind not in "iu":
        raise ValueError(f"lag_bounds must be an integer array, got dtype {a.dtype}")
    if a.ndim == 2 and a.shape == (n_pairs, 2):
        per_window = False
    elif a.ndim == 3 and a.shape == (n_windows, n_pairs, 2):
        per_window = True
    else:
        raise ValueError(f"lag_bounds must be [P][2] = [{n_pairs}][2] or [W][P][2] = [{n_windows}][{n_pairs}][2], "
                         f"got shape {a.shape}")
    if a.size and (a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max):
        raise ValueError("lag_bounds values do not fit int32")
    return np.ascontiguousarray(a, dtype=np.int32), per_window


def _check_band_rows(name: str, value, n_windows: int, sets: bool):
    """what check_band (sets False: rows [2] or [W][2]) and check_bands (sets True: [M][2] or [W][M][2]) share"""
    a = np.asarray(value)
    if a.dtype.kind not in "iuf":
        raise ValueError(f"{name} must be a real array, got dtype {a.dtype}")
    shared = 2 if sets else 1   # dimensions of the array that every window shares
    if a.ndim == shared and a.shape[-1] == 2:
        per_window = False
    elif a.ndim == shared + 1 and a.shape[0] == n_windows and a.shape[-1] == 2:
        per_window = True
    elif sets:
        raise ValueError(f"bands must be [M][2] or [W][M][2] = [{n_windows}][M][2], got shape {a.shape}")
    else:
        raise ValueError(f"band must be [2] or [W][2] = [{n_windows}][2], got shape {a.shape}")
    if sets and not 1 <= a.shape[-2] <= MAX_BANDS:
        raise ValueError(f"bands must hold 1..{MAX_BANDS} bands per window, got {a.shape[-2]}")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name} values must be finite")
    lo, hi = a[..., 0], a[..., 1]
    if np.any(lo < -0.5) or np.any(hi > 0.5) or np.any(lo > hi):
        raise ValueError(f"{name} must satisfy -0.5 <= lo <= hi <= 0.5 (cycles per sample; no wrap across +-fs/2)")
    return a, per_window


def check_band(band, n_windows: int):
    """band as correlate() takes it -> (contiguous float64 array or None, per_window).  Shape [2] (one [lo, hi] shared by
    every window) or [W][2], in cycles per sample; finite, -0.5 <= lo <= hi <= 0.5.  Raises ValueError before any call
    into the library.  Whether a band keeps a bin at all depends on the window length: the library checks that
    (RmxError, RMX_E_INVAL)."""
    if band is None:
        return None, False
    return _check_band_rows("band", band, n_windows, False)


MAX_BANDS = 64


def check_bands(bands, n_windows: int):
    """bands as correlate_bands() takes them -> (contiguous float64 array, per_window).  Shape [M][2] (one set of M bands
    shared by every window) or [W][M][2], 1 <= M <= 64, in cycles per sample; finite, -0.5 <= lo <= hi <= 0.5.  Raises
    ValueError before any call into the library.  Whether a band keeps a bin at all depends on the window length: the
    library checks that (RmxError, RMX_E_INVAL)."""
    if bands is None:
        raise ValueError("bands must be an array [M][2] or [W][M][2], got None")
    return _check_band_rows("bands", bands, n_windows, True)


def check_integrate(integrate, n_windows: int) -> int:
    """integrate as correlate() takes it -> K, the windows per group (noncoherent integration, rmx_xcorr_batch_integrated).
    An integer >= 1 that divides n_windows; raises ValueError before any call into the library."""
    if isinstance(integrate, bool) or not isinstance(integrate, (int, np.integer)):
        raise ValueError(f"integrate must be an integer, got {integrate!r}")
    k = int(integrate)
    if k < 1:
        raise ValueError(f"integrate must be >= 1, got {k}")
    if n_windows % k != 0:
        raise ValueError(f"the number of windows, {n_windows}, is not a multiple of integrate = {k}")
    return k


REFINE_VALUES = (0, 2, 4, 8, 16)


def check_refine(refine) -> int:
    """refine as correlate() takes it -> U, the fine lag grid of 1 / U samples around the integer peak
    (rmx_xcorr_batch_refined): one of 0 (none), 2, 4, 8, 16; raises ValueError before any call into the library."""
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)):
        raise ValueError(f"refine must be an integer, got {refine!r}")
    u = int(refine)
    if u not in REFINE_VALUES:
        raise ValueError(f"refine must be one of {REFINE_VALUES}, got {u}")
    return u


OUTPUTS = ("dop_idx", "dop_frac", "lag_int", "lag_frac", "peak", "quality")   # in the order every method returns them


_BANDED = ("bands", "caf_bands")   # the families whose outputs carry a band axis
_SEARCH = ("caf", "caf_bands")     # the families with a Doppler grid and a dop_idx output


class LagRequest(NamedTuple):
    """One checked correlation or Doppler-search call: what lag_request() made of the options of correlate(),
    correlate_bands(), caf(), caf_bands() and their device-pointer twins.  It holds the normalised host arrays themselves, so whoever holds
    the request keeps alive what the C entry reads; it is a tuple, so nothing changes it after the checks (MultiXcorrEngine
    hands one to several worker threads, and cut() returns views)."""
    family: str                    # "xcorr", "bands", "caf" or "caf_bands"
    n_windows: int
    K: int                         # windows per group
    U: int                         # fine lag grid, 0 for none
    P: int
    M: int                         # bands per window ("bands", "caf_bands"), else 0
    pairs: Optional[np.ndarray]    # int32 [P][2], None: every i < j
    bounds: Optional[np.ndarray]   # int32 [P][2] or [rows][P][2]
    bounds_per_row: bool
    band: Optional[np.ndarray]     # float64 [2] or [W][2]; "bands", "caf_bands": [M][2] or [W][M][2]
    band_per_window: bool
    grid: Optional[np.ndarray]     # float64 [D] ("caf", "caf_bands")
    whiten: bool
    fine: bool                     # a dop_frac output ("caf", "caf_bands")
    quality: bool                  # a quality output

    @property
    def rows(self) -> int:
        """the rows of every output: the windows, or the groups of K"""
        return self.n_windows // self.K

    def outputs(self, rows: Optional[int] = None):
        """(name, dtype, shape) of every output of the call (or of `rows` of its rows), in the order the methods return them"""
        shape = (self.rows if rows is None else rows,) + ((self.M,) if self.family in _BANDED else ()) + (self.P,)
        have = {"dop_idx": self.family in _SEARCH, "dop_frac": self.fine, "quality": self.quality}
        return [(n, np.int32 if n in ("dop_idx", "lag_int") else np.float32, shape + ((4,) if n == "quality" else ()))
                for n in OUTPUTS if have.get(n, True)]

    def cut(self, g0: int, g1: int):
        """(lag_bounds, band(s)) of rows g0 .. g1 - 1: an array every row shares goes whole, per-row bounds are cut by row,
        per-window band(s) by the rows' windows"""
        return (self.bounds[g0:g1] if self.bounds_per_row else self.bounds,
                self.band[g0 * self.K:g1 * self.K] if self.band_per_window else self.band)


def lag_request(family: str, n_buoys: int, n_windows: int, pairs=None, lag_bounds=None, band=None, whiten=False, integrate=1,
                refine=0, quality=False, doppler_cps=None, fine=False, n_pairs: Optional[int] = None) -> LagRequest:
    """The one place where the options of a call are checked: ValueError before any call into the library, in the order
    integrate, refine, pairs, then lag_bounds, band ("xcorr"), bands, lag_bounds ("bands": `band` is the band set) or grid,
    lag_bounds, band ("caf", where integrate = None is 1 without a check) or grid, bands, lag_bounds ("caf_bands", which has no
    integration, refinement or quality and says so).  n_pairs: the pair count of a caller that leaves the
    pair list to somebody else's check (MultiXcorrEngine: its engines see the caller's own list)."""
    if family == "caf_bands":
        for what, asked in (("integration", integrate is not None and integrate != 1), ("refinement", refine != 0),
                            ("quality", bool(quality))):
            if asked:
                raise ValueError(f"rmx_caf_batch_bands has no {what}: caf() takes integrate, refine and quality, one band per window")
    K = 1 if integrate is None and family in _SEARCH else check_integrate(integrate, n_windows)
    U = check_refine(refine)
    if n_pairs is not None:
        pairs, P = None, n_pairs
    elif pairs is None:
        P = n_buoys * (n_buoys - 1) // 2
    else:
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        P = pairs.shape[0]
    grid, M = None, 0
    if family in _BANDED:
        if family == "caf_bands":
            grid = np.ascontiguousarray(doppler_cps, dtype=np.float64).reshape(-1)
        bd, band_pw = check_bands(band, n_windows)
        M = bd.shape[-2]
        lb, per_row = check_lag_bounds(lag_bounds, n_windows // K, P)
    else:
        if family == "caf":
            grid = np.ascontiguousarray(doppler_cps, dtype=np.float64).reshape(-1)
        lb, per_row = check_lag_bounds(lag_bounds, n_windows // K, P)
        bd, band_pw = check_band(band, n_windows)
    return LagRequest._make((family, n_windows, K, U, P, M, pairs, lb, per_row, bd, band_pw, grid, bool(whiten), bool(fine),
                             bool(quality)))


# what each entry takes between (ctx, iq, n_windows, pairs, n_pairs[, grid, n_dopplers]) and (lag_int, lag_frac, peak, flags), in
# this order: K integrate; W band(s)[, n_bands], per window, weighting; B lag bounds, per row; U refine; (dop_idx: every
# caf entry); F dop_frac; (the three outputs); Q quality
_ENTRY_ARGS = {"rmx_xcorr_batch": "", "rmx_xcorr_batch_bounded": "B", "rmx_xcorr_batch_weighted": "WB",
               "rmx_xcorr_batch_integrated": "KWB", "rmx_xcorr_batch_refined": "KWBU", "rmx_xcorr_batch_quality": "KWBUQ",
               "rmx_xcorr_batch_bands": "WB", "rmx_xcorr_batch_bands_quality": "WBUQ", "rmx_xcorr_batch_bands_integrated": "KWBUQ",
               "rmx_caf_batch": "", "rmx_caf_batch_request": "WBF", "rmx_caf_batch_quality": "WBUFQ",
               "rmx_caf_batch_integrated": "KWBUFQ", "rmx_caf_batch_bands": "WBF"}


def entry_name(req: LagRequest) -> str:
    """The C entry a request goes through: the smallest one that takes what it asks for."""
    if req.family == "xcorr":
        if req.quality:
            return "rmx_xcorr_batch_quality"
        if req.U > 0:
            return "rmx_xcorr_batch_refined"
        if req.K > 1:
            return "rmx_xcorr_batch_integrated"
        if req.band is not None or req.whiten:
            return "rmx_xcorr_batch_weighted"
        return "rmx_xcorr_batch" if req.bounds is None else "rmx_xcorr_batch_bounded"
    if req.family == "caf_bands":
        return "rmx_caf_batch_bands"
    stem = "rmx_xcorr_batch_bands" if req.family == "bands" else "rmx_caf_batch"
    if req.K > 1:
        return stem + "_integrated"
    if req.U > 0 or req.quality:
        return stem + "_quality"
    if req.family == "bands" or (req.band is None and not req.whiten and req.bounds is None and not req.fine):
        return stem
    return "rmx_caf_batch_request"


def psr_threshold(n_lags: int, pfa: float, integrate: int = 1) -> float:
    """The peak-to-floor ratio (quality[..., RMX_Q_PSR]) that a white noise-only pair exceeds with probability `pfa` in a
    search over `n_lags` lags: the T with n_lags * Q(K, K T / 2) = pfa, where Q(K, x) = exp(-x) sum_{n < K} x^n / n! is the
    tail of the Gamma(K) that the sum of K = `integrate` windows' |r|^2 / floor follows (Exp(1) for K = 1: T = 2 ln(n_lags /
    pfa)).  The factor 1/2 is the worst case of the zero-padded correlation's triangular variance: near lag 0 a lag's own
    floor is up to twice the mean floor that psr divides by.  numpy only; no call into the library."""
    if isinstance(integrate, bool) or not isinstance(integrate, (int, np.integer)) or integrate < 1:
        raise ValueError(f"integrate must be an integer >= 1, got {integrate!r}")
    if not n_lags >= 1:
        raise ValueError(f"n_lags must be >= 1, got {n_lags!r}")
    if not 0.0 < pfa < 1.0:
        raise ValueError(f"pfa must lie in (0, 1), got {pfa!r}")
    K = int(integrate)
    target = math.log(pfa / n_lags)

    def log_q(x):   # log Q(K, x), terms relative to the largest one
        if x == 0.0:
            return 0.0
        logs = [n * math.log(x) - math.lgamma(n + 1.0) for n in range(K)]
        top = max(logs)
        return -x + top + math.log(sum(math.exp(v - top) for v in logs))

    lo, hi = 0.0, 1.0
    while log_q(hi) > target:
        hi *= 2.0
    for _ in range(200):   # log Q falls monotonically in x
        mid = 0.5 * (lo + hi)
        if log_q(mid) > target:
            lo = mid
        else:
            hi = mid
    return 2.0 * hi / K


def lag_sigma(quality) -> np.ndarray:
    """A rough Cramer-Rao-type standard deviation of each lag, in samples, from its quality figures [...][4]:
        sqrt((1 - rho^2) / (rho^2 n_eff)) / (2 pi rms_bw),   rho = coherence.
    An indicator for solver weights, not a bound that holds: on synthetic band-limited scenes the observed rms error of the
    refined lag was 0.33 ... 0.89 of this figure without PHAT and 1.64 of it with PHAT.  inf where coherence, n_eff or
    rms_bw is 0 (a dead receiver); 0 at coherence 1."""
    q = np.asarray(quality, np.float64)
    if q.shape[-1] != 4:
        raise ValueError(f"quality must be [...][4], got shape {q.shape}")
    rho, n_eff, bw = q[..., RMX_Q_COHERENCE], q[..., RMX_Q_NEFF], q[..., RMX_Q_RMS_BW]
    ok = (rho > 0) & (n_eff > 0) & (bw > 0)
    safe = np.where(ok, rho * rho * n_eff, 1.0)
    sig = np.sqrt(np.maximum(1.0 - rho * rho, 0.0) / safe) / (2.0 * math.pi * np.where(ok, bw, 1.0))
    return np.where(ok, sig, np.inf)


SPEED_OF_LIGHT = 299792458.0


def lag_weight(sigma_samples, sample_rate_hz: float, sigma_floor_samples: float) -> np.ndarray:
    """The weight of a lag in the position solve (solve_fix), float32 in m^-2, from its standard deviation in samples
    (lag_sigma):
        1 / ((sigma^2 + floor^2) * mps^2),   mps = 299792458 / sample_rate_hz metres per sample.
    sigma_floor_samples is the stations' clock-synchronisation uncertainty in samples, added in quadrature.  It must be
    finite and > 0: lag_sigma is 0 at coherence 1, which would otherwise be an infinite weight.  sigma = inf (a dead
    receiver) gives weight 0: the solve ignores the pair.  A negative or NaN sigma is a ValueError.  numpy only."""
    floor = float(sigma_floor_samples)
    if not (math.isfinite(floor) and floor > 0.0):
        raise ValueError(f"sigma_floor_samples must be finite and > 0, got {sigma_floor_samples}")
    fs = float(sample_rate_hz)
    if not (math.isfinite(fs) and fs > 0.0):
        raise ValueError(f"sample_rate_hz must be finite and positive, got {sample_rate_hz}")
    sig = np.asarray(sigma_samples, np.float64)
    if np.any(np.isnan(sig)) or np.any(sig < 0.0):
        raise ValueError("sigma_samples must be >= 0 (inf allowed) and not NaN")
    mps = SPEED_OF_LIGHT / fs
    with np.errstate(over="ignore"):
        return (1.0 / ((sig * sig + floor * floor) * (mps * mps))).astype(np.float32)


def error_ellipse(cov2, confidence: float = 0.95):
    """The error ellipse of a plane-mode fix from its covariance cov2 [...][3] = 11 12 22 (solve_fix(plane=...).cov).
    Returns (semi_major, semi_minor, angle): the semi-axes in the covariance's length unit, scaled by
    sqrt(-2 ln(1 - confidence)) (2.4477 at 0.95: the fix lies inside with that probability under Gaussian errors), and the
    angle of the major axis in radians from e1 towards e2, in (-pi/2, pi/2].  A singular covariance (inf on its diagonal)
    gives inf axes and angle 0.  numpy only."""
    c = np.asarray(cov2, np.float64)
    if c.shape[-1] != 3:
        raise ValueError(f"cov2 must be [...][3] (11 12 22), got shape {c.shape}")
    if not 0.0 < float(confidence) < 1.0:
        raise ValueError(f"confidence must lie strictly between 0 and 1, got {confidence}")
    k = math.sqrt(-2.0 * math.log(1.0 - float(confidence)))
    c11, c12, c22 = c[..., 0], c[..., 1], c[..., 2]
    ok = np.isfinite(c11) & np.isfinite(c12) & np.isfinite(c22)
    a, b, d = np.where(ok, c11, 1.0), np.where(ok, c12, 0.0), np.where(ok, c22, 1.0)
    mean, half = 0.5 * (a + d), 0.5 * (a - d)
    root = np.sqrt(half * half + b * b)
    major = np.sqrt(np.maximum(mean + root, 0.0))
    minor = np.sqrt(np.maximum(mean - root, 0.0))
    angle = 0.5 * np.arctan2(2.0 * b, a - d)
    angle = np.where(angle <= -0.5 * math.pi, angle + math.pi, angle)
    return np.where(ok, k * major, np.inf), np.where(ok, k * minor, np.inf), np.where(ok, angle, 0.0)


class SolveFix(NamedTuple):
    """XcorrEngine.solve_fix: the fix, and what says how far it can be trusted (rmx_solve_batch_fix)"""
    pos: np.ndarray      # float64 [W][3] ECEF metres
    cost: np.ndarray     # float64 [W]: f at pos; a chi-square where weight = 1 / sigma_d^2
    iters: np.ndarray    # int32 [W]
    info: np.ndarray     # float64 [W][6] xx xy xz yy yz zz (ECEF), or [W][3] 11 12 22 in plane coordinates
    cov: np.ndarray      # float64, info's inverse in the same layout; inf on the diagonal and 0 off it where singular
    resid: Optional[np.ndarray]   # float64 [W][P] metres, or None


def doppler_estimate(doppler_cps, dop_idx, dop_frac) -> np.ndarray:
    """The frequency offset, float64 in cycles per sample, that caf(..., fine=True) found:
        doppler_cps[dop_idx] + dop_frac * step,   step = the grid's spacing.
    dop_frac is in grid indices, so the grid must be uniformly spaced: ValueError for one that is not (a relative 1e-9
    of the step is allowed), for a grid of fewer than 2 points when a dop_frac is not 0, and for indices outside the
    grid.  numpy only; no call into the library."""
    grid = np.asarray(doppler_cps, np.float64).reshape(-1)
    idx = np.asarray(dop_idx)
    frac = np.asarray(dop_frac, np.float64)
    if idx.dtype.kind not in "iu":
        raise ValueError(f"dop_idx must be an integer array, got dtype {idx.dtype}")
    if idx.shape != frac.shape:
        raise ValueError(f"dop_frac must have dop_idx's shape {idx.shape}, got {frac.shape}")
    if grid.size < 1 or not np.all(np.isfinite(grid)):
        raise ValueError("doppler_cps must be a non-empty finite grid")
    if idx.size and (idx.min() < 0 or idx.max() >= grid.size):
        raise ValueError(f"dop_idx must lie in 0..{grid.size - 1}")
    if grid.size < 2:
        if np.any(frac != 0.0):
            raise ValueError("a grid of fewer than 2 points has no spacing: dop_frac must be 0")
        return grid[idx] + 0.0 * frac
    steps = np.diff(grid)
    step = (grid[-1] - grid[0]) / (grid.size - 1)
    if step == 0.0 or np.any(np.abs(steps - step) > 1e-9 * abs(step)):
        raise ValueError("doppler_cps is not uniformly spaced: dop_frac is in grid indices and has no meaning on it")
    return grid[idx] + frac * step


EXPORTS = ["rmx_version", "rmx_device_count", "rmx_create", "rmx_destroy", "rmx_last_error",
           "rmx_set_stream", "rmx_set_option", "rmx_set_default_option", "rmx_clear_default_options", "rmx_xcorr_batch", "rmx_xcorr_batch_bounded", "rmx_xcorr_batch_weighted", "rmx_xcorr_batch_bands", "rmx_xcorr_batch_integrated", "rmx_xcorr_batch_refined", "rmx_xcorr_batch_quality", "rmx_xcorr_batch_bands_quality", "rmx_xcorr_batch_bands_integrated", "rmx_caf_batch", "rmx_caf_batch_request", "rmx_caf_batch_quality", "rmx_caf_batch_integrated", "rmx_caf_batch_bands", "rmx_solve_batch", "rmx_solve_batch_fix", "rmx_detect_batch", "rmx_synchronize",
           "rmx_last_timing", "rmx_last_timing_kind", "rmx_build_info", "rmx_scratch_bytes"]


def build_info() -> dict:
    """rmx_build_info() parsed: {"source_digest": ..., "arch": ...} of the loaded binary."""
    txt = load_library().rmx_build_info().decode()
    out = {"text": txt}
    for tok in txt.split()[1:]:
        k, _, v = tok.partition("=")
        out[k] = v
    return out


def set_default_option(key: str, value: int) -> None:
    """Kernel-selection default for engines created afterwards (rmx_set_default_option: tests and A/B runs)."""
    lib = load_library()
    if lib.rmx_set_default_option(key.encode(), int(value)) != 0:
        msg = lib.rmx_last_error(None)
        raise RmxError(-1, msg.decode() if msg else "rmx_set_default_option failed")


def clear_default_options() -> None:
    load_library().rmx_clear_default_options()


def apply_env_options(environ=None, strict: bool = True, report=None) -> dict:
    """For the tools/ scripts only: turns RMX_<KEY>=<int> environment variables into default options (the library
    itself never reads the environment).  Returns what was applied.  A variable the library refuses (unknown key, value
    out of range, not an integer) raises ValueError when `strict` -- an A/B run must not silently measure the default
    path -- and is only reported otherwise; `report` (a file object, stderr in the tools) gets one line
    with what was applied and what was refused."""
    import os as _os
    env = _os.environ if environ is None else environ
    done, refused = {}, {}
    for k, v in sorted(env.items()):
        if not k.startswith("RMX_") or k in ("RMX_LIBRARY", "RMX_CPU_THREADS") or k.startswith("RMX_BENCH"):
            continue
        try:
            set_default_option(k[4:].lower(), int(v))
            done[k[4:].lower()] = int(v)
        except (RmxError, ValueError) as e:
            refused[k] = str(e)
    if report is not None and (done or refused):
        print(f"[rmx options] applied {done}" + (f"  REFUSED {refused}" if refused else ""), file=report, flush=True)
    if refused and strict:
        raise ValueError(f"environment options the library refused: {refused}")
    return done


def device_count() -> int:
    return int(load_library().rmx_device_count())


def pair_list(n_buoys: int) -> np.ndarray:
    """(i, j), i < j, nested-loop order of tdoa_processor.py:156-157."""
    return np.array([(i, j) for i in range(n_buoys) for j in range(i + 1, n_buoys)],
                    dtype=np.int32).reshape(-1, 2)


class XcorrEngine:
    """One engine = one rmx_ctx = one GPU.  Batched pairwise cross-correlation lags."""

    def __init__(self, n_buoys: int, n_samples: int, max_windows: int, device: int = 0):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        rc = self._lib.rmx_create(C.byref(self._ctx), device, n_buoys, n_samples, max_windows, 0)
        if rc != 0:
            msg = self._lib.rmx_last_error(None)
            self._ctx = C.c_void_p()
            raise RmxError(rc, msg.decode() if msg else "rmx_create failed")
        self.n_buoys, self.n_samples, self.max_windows, self.device = n_buoys, n_samples, max_windows, device

    # -- plumbing ------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            msg = self._lib.rmx_last_error(self._ctx)
            raise RmxError(rc, msg.decode() if msg else "?")

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.rmx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, hip_stream: int):
        self._check(self._lib.rmx_set_stream(self._ctx, C.c_void_p(hip_stream)))

    def set_option(self, key: str, value: int):
        self._check(self._lib.rmx_set_option(self._ctx, key.encode(), int(value)))

    def synchronize(self):
        self._check(self._lib.rmx_synchronize(self._ctx))

    def scratch_bytes(self) -> int:
        return int(self._lib.rmx_scratch_bytes(self._ctx))

    def last_timing(self) -> dict:
        f, p = C.c_float(), C.c_float()
        nf, npair = C.c_int(), C.c_int()
        self._check(self._lib.rmx_last_timing(self._ctx, C.byref(f), C.byref(nf), C.byref(p), C.byref(npair)))
        return dict(fwd_ms=f.value, fwd_launches=nf.value, pair_ms=p.value, pair_launches=npair.value)

    def last_timing_by_kernel(self) -> dict:
        """{kernel family: {"ms": summed HIP-event time, "launches": n}} of the last correlate / caf call (option
        "timing" = 1), families without a launch left out (rmx_last_timing_kind)."""
        out = {}
        kind = 0
        while True:
            name, ms, n = C.c_char_p(), C.c_float(), C.c_int()
            if self._lib.rmx_last_timing_kind(self._ctx, kind, C.byref(name), C.byref(ms), C.byref(n)) != 0:
                break
            if n.value:
                out[name.value.decode()] = {"ms": ms.value, "launches": n.value}
            kind += 1
        return out

    def _check_iq(self, iq):
        """Shape/dtype check of a host window array before its pointer goes to C (which reads
        n_windows * n_buoys * n_samples samples from it).  Returns (contiguous array, flags)."""
        iq = np.asarray(iq)
        flags = 0
        if iq.dtype == np.uint8:
            flags |= RMX_IN_U8
            if iq.ndim != 3 or iq.shape[1] != self.n_buoys or iq.shape[2] != 2 * self.n_samples:
                raise ValueError(f"uint8 iq must be [W][{self.n_buoys}][{2 * self.n_samples}], got {iq.shape}")
        else:
            iq = np.ascontiguousarray(iq, dtype=np.complex64)
            if iq.ndim != 3 or iq.shape[1] != self.n_buoys or iq.shape[2] != self.n_samples:
                raise ValueError(f"iq must be [W][{self.n_buoys}][{self.n_samples}], got {iq.shape}")
        return np.ascontiguousarray(iq), flags

    # -- the hot path ----------------------------------------------------------------------------
    def _call(self, req: LagRequest, iq_p, out_p, flags: int):
        """The one call into the library: the request through the entry entry_name() names.  iq_p and out_p, the pointers of
        OUTPUTS with None for an output the call does not have, are host or device pointers, as `flags` says; the host
        arrays are the request's own."""
        name = entry_name(req)
        args, vp = _ENTRY_ARGS[name], C.c_void_p
        family, W, K, U, P, M, pairs, bounds, per_row, band, band_pw, grid, whiten, _, _ = req
        dop_p, dop_frac_p, lag_int_p, lag_frac_p, peak_p, quality_p = out_p
        a = [self._ctx, iq_p, W, None if pairs is None else pairs.ctypes.data_as(vp), P]
        if family in _SEARCH:
            a += (grid.ctypes.data_as(vp), grid.shape[0])
        if "K" in args:
            a.append(K)
        if "W" in args:
            a.append(None if band is None else band.ctypes.data_as(vp))
            if family in _BANDED:
                a.append(M)
            a += (int(band_pw), RMX_WEIGHT_PHAT if whiten else RMX_WEIGHT_NONE)
        if "B" in args:
            a += (None if bounds is None else bounds.ctypes.data_as(vp), int(per_row))
        if "U" in args:
            a.append(U)
        if family in _SEARCH:
            a.append(dop_p)
        if "F" in args:
            a.append(dop_frac_p)
        a += (lag_int_p, lag_frac_p, peak_p)
        if "Q" in args:
            a.append(quality_p)
        self._check(getattr(self._lib, name)(*a, flags))

    def _host_call(self, req: LagRequest, iq: np.ndarray, flags: int):
        """the outputs of a host-array call as zeroed arrays, filled by _call unless the batch is empty (no call then)"""
        out = {n: np.zeros(shape, dt) for n, dt, shape in req.outputs()}
        if req.n_windows and req.P:
            vp = C.c_void_p
            self._call(req, iq.ctypes.data_as(vp), [out[n].ctypes.data_as(vp) if n in out else None for n in OUTPUTS], flags)
        return tuple(out.values())

    def _xcorr(self, iq_p, W: int, pp, P: int, K: int, bd, band_pw: bool, whiten: bool, lb, per_window: bool,
               lag_int_p, lag_frac_p, peak_p, flags: int, U: int = 0, quality_p=None):
        """(for callers that hold checked parts and pointers of their own: one correlation call, as _call makes it)"""
        pairs = None if pp is None else np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_int32)), (P, 2))
        self._call(LagRequest("xcorr", W, K, U, P, 0, pairs, lb, bool(per_window), bd, bool(band_pw), None, bool(whiten), False,
                              quality_p is not None), iq_p, (None, None, lag_int_p, lag_frac_p, peak_p, quality_p), flags)

    def _pairs_arg(self, pairs):
        """(as _xcorr) pairs as the entries take it -> (kept int32 array or None, its pointer or None, P)"""
        if pairs is None:
            return None, None, self.n_buoys * (self.n_buoys - 1) // 2
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        return pairs, pairs.ctypes.data_as(C.c_void_p), pairs.shape[0]

    def correlate(self, iq: np.ndarray, pairs: Optional[np.ndarray] = None, lag_bounds=None, band=None,
                  whiten: bool = False, integrate: int = 1, refine: int = 0, quality: bool = False):
        """Host arrays in, host arrays out.  iq: complex64 [W][B][N] (or uint8 [W][B][2N] raw
        rtl_sdr I,Q).  Returns (lag_int int32 [W][P], lag_frac float32 [W][P], peak float32 [W][P]);
        lag = lag_int + lag_frac = delay(j) - delay(i) in samples.
        lag_bounds: None (every lag of 'full'), or int [P][2] / [W][P][2] = [lo, hi] per pair (per window): the peak
        is searched over lags lo..hi only (rmx_xcorr_batch_bounded).
        band: None (every bin), or float [2] / [W][2] = [lo, hi] in cycles per sample (f / fs) kept of the
        cross-spectrum; whiten: PHAT, every bin at unit magnitude (rmx_xcorr_batch_weighted).
        integrate: K >= 1; every K consecutive windows form a group with ONE peak search on the sum of the windows'
        squared magnitudes (rmx_xcorr_batch_integrated).  W must be a multiple of K; the results are [W // K][P],
        lag_bounds [P][2] or [W // K][P][2]; band stays per window.
        refine: U in (0, 2, 4, 8, 16); U > 0 takes the sub-sample estimate from the band-limited interpolant of the
        correlation on a grid of 1 / U samples around the integer peak instead of the three-point parabola
        (rmx_xcorr_batch_refined): the same integer peak, the estimate relocated within +-1 sample of it.
        quality: True returns a fourth array, float32 [W // K][P][4] = (coherence, psr, rms_bw, n_eff) of every lag, indexed
        by RMX_Q_* (rmx_xcorr_batch_quality; psr_threshold and lag_sigma read them); the first three arrays are bit for bit
        those of the same call without it."""
        iq, flags = self._check_iq(iq)
        return self._host_call(lag_request("xcorr", self.n_buoys, iq.shape[0], pairs, lag_bounds, band, whiten, integrate, refine,
                                           quality), iq, flags)

    def correlate_bands(self, iq: np.ndarray, bands, pairs: Optional[np.ndarray] = None, lag_bounds=None,
                        whiten: bool = False, refine: int = 0, quality: bool = False, integrate: int = 1):
        """Every window under several bands with ONE forward transform per (window, buoy) (rmx_xcorr_batch_bands).
        iq: as for correlate().  bands: float [M][2] (shared by every window) or [W][M][2], [lo, hi] in cycles per sample,
        1 <= M <= 64.  lag_bounds: None, [P][2] or [W][P][2]: per (window, pair), shared by the window's bands.  whiten:
        PHAT.  Returns (lag_int int32, lag_frac float32, peak float32), each [W][M][P]; [:, m] is bit for bit what
        correlate(iq, band=bands[..., m, :], ...) returns.
        refine: U in (0, 2, 4, 8, 16), the fine lag search of correlate(refine=U) per (window, band, pair); quality: True
        returns a fourth array, float32 [W][M][P][4] indexed by RMX_Q_* (rmx_xcorr_batch_bands_quality; still one forward
        transform per (window, buoy)).  With neither, the call is rmx_xcorr_batch_bands.
        integrate: K >= 1, as for correlate(): every K consecutive windows form a group with ONE peak search per (group,
        band, pair) on the sum of the windows' squared magnitudes (rmx_xcorr_batch_bands_integrated).  W must be a multiple
        of K; the results are [W // K][M][P] ([...][4]), lag_bounds [P][2] or [W // K][P][2]; bands stay [M][2] or
        [W][M][2], and [:, m] is what correlate(iq, band=bands[..., m, :], integrate=K, ...) returns."""
        iq, flags = self._check_iq(iq)
        return self._host_call(lag_request("bands", self.n_buoys, iq.shape[0], pairs, lag_bounds, bands, whiten, integrate, refine,
                                           quality), iq, flags)

    def correlate_bands_device(self, iq_ptr: int, n_windows: int, bands, lag_int_ptr: int, lag_frac_ptr: int, peak_ptr: int,
                               pairs: Optional[np.ndarray] = None, u8: bool = False, lag_bounds=None, whiten: bool = False,
                               refine: int = 0, quality_ptr: Optional[int] = None, integrate: int = 1):
        """correlate_bands() with device pointers in and out (the bands, the pair list and the bounds stay host arrays; the
        library keeps its own copies); asynchronous on the ctx stream.  The outputs are [n_windows // K][M][P]; quality_ptr,
        if given, [n_windows // K][M][P][4] float32 on the device (rmx_xcorr_batch_bands_quality; with integrate = K > 1
        rmx_xcorr_batch_bands_integrated)."""
        req = lag_request("bands", self.n_buoys, n_windows, pairs, lag_bounds, bands, whiten, integrate, refine,
                          quality_ptr is not None)
        vp = C.c_void_p
        self._call(req, vp(iq_ptr), (None, None, vp(lag_int_ptr), vp(lag_frac_ptr), vp(peak_ptr),
                                     None if quality_ptr is None else vp(quality_ptr)), _DEVICE | (RMX_IN_U8 if u8 else 0))

    def caf(self, iq: np.ndarray, doppler_cps, pairs: Optional[np.ndarray] = None, lag_bounds=None, band=None,
            whiten: bool = False, fine: bool = False, refine: int = 0, quality: bool = False, integrate=None):
        """Cross-ambiguity search (rmx_caf_batch, rmx_caf_batch_request, rmx_caf_batch_quality): host arrays in and out.
        doppler_cps: hypotheses in cycles/sample.  lag_bounds, band, whiten: as for correlate(), shared by all hypotheses
        of a (window, pair).
        Returns (doppler_idx int32, lag_int int32, lag_frac float32, peak float32), each [W][P]; with fine=True
        (doppler_idx, dop_frac float32, lag_int, lag_frac, peak): dop_frac is the sub-grid Doppler estimate in grid
        indices (doppler_estimate turns it into cycles per sample); the other four are bit for bit those without it.
        refine: U in (0, 2, 4, 8, 16), the fine lag search of correlate(refine=U) on each slot's winning hypothesis; the
        winner and dop_frac do not move.  quality: True appends float32 [W][P][4] = (coherence, psr, rms_bw, n_eff) of the
        winner's pair, indexed by RMX_Q_*, as the last element (psr_threshold and lag_sigma read it).
        integrate: K windows per group (rmx_caf_batch_integrated): every hypothesis' |r|^2 is summed over the K consecutive
        windows of a group before ONE peak search; every output is then [W // K][P] (quality [W // K][P][4]), lag_bounds
        [P][2] or [W // K][P][2] per group, the band stays per window.  None (or 1): the search per window."""
        iq, flags = self._check_iq(iq)
        return self._host_call(lag_request("caf", self.n_buoys, iq.shape[0], pairs, lag_bounds, band, whiten, integrate, refine,
                                           quality, doppler_cps, fine), iq, flags)

    def caf_bands(self, iq: np.ndarray, doppler_cps, bands, pairs: Optional[np.ndarray] = None, lag_bounds=None,
                  whiten: bool = False, fine: bool = False):
        """The cross-ambiguity search under several bands per window with ONE set of forward transforms
        (rmx_caf_batch_bands): host arrays in and out.  iq, doppler_cps, lag_bounds, whiten, fine: as for caf(); bands: float
        [M][2] (shared by every window) or [W][M][2], as for correlate_bands().  The bounds are per (window, pair), shared by
        the window's bands and hypotheses.
        Returns (doppler_idx int32, lag_int int32, lag_frac float32, peak float32), each [W][M][P]; with fine=True
        (doppler_idx, dop_frac float32, lag_int, lag_frac, peak).  [:, m] is what caf(iq, doppler_cps,
        band=bands[..., m, :], ...) returns; every (window, band, pair) chooses its own hypothesis.
        The entry has no integration, refinement or quality: caf() takes those, one band per window."""
        iq, flags = self._check_iq(iq)
        return self._host_call(lag_request("caf_bands", self.n_buoys, iq.shape[0], pairs, lag_bounds, bands, whiten,
                                           doppler_cps=doppler_cps, fine=fine), iq, flags)

    @staticmethod
    def _solve_request(buoy_xyz, lag_int, lag_frac, sample_rate_hz, weight, pairs, max_iter):
        """the checks of solve() and solve_fix(): the arrays as the C entry reads them, (bx, li, lf, wgt or None, pairs or
        None), or a ValueError that names the argument"""
        bx = np.ascontiguousarray(buoy_xyz, dtype=np.float64)
        if bx.size % 3 != 0 or not 2 <= bx.size // 3 <= 64:
            raise ValueError(f"buoy_xyz must reshape to [B][3] with 2 <= B <= 64, got shape {bx.shape}")
        bx = bx.reshape(-1, 3)
        B = bx.shape[0]
        li = np.ascontiguousarray(lag_int, dtype=np.int32)
        if li.ndim != 2:
            raise ValueError(f"lag_int must be [W][P], got shape {li.shape}")
        lf = np.ascontiguousarray(lag_frac, dtype=np.float32)
        if lf.shape != li.shape:
            raise ValueError(f"lag_frac must have lag_int's shape {li.shape}, got {lf.shape}")
        W, P = li.shape
        wgt = None
        if weight is not None:
            wgt = np.asarray(weight, dtype=np.float32)
            if wgt.shape == (P,):
                wgt = np.broadcast_to(wgt, (W, P))
            elif wgt.shape != (W, P):
                raise ValueError(f"weight must be None, [{W}][{P}] or [{P}], got shape {wgt.shape}")
            wgt = np.ascontiguousarray(wgt)
        if pairs is not None:
            pairs = np.ascontiguousarray(pairs, dtype=np.int32)
            if pairs.size != 2 * P:
                raise ValueError(f"pairs must be [{P}][2] for lag arrays of {P} columns, got shape {pairs.shape}")
            pairs = pairs.reshape(-1, 2)
        elif P != B * (B - 1) // 2:
            raise ValueError(f"pairs is None: lag_int needs {B * (B - 1) // 2} columns for {B} buoys, got {P}")
        if not int(max_iter) >= 1:
            raise ValueError(f"max_iter must be >= 1, got {max_iter}")
        if not float(sample_rate_hz) > 0.0:
            raise ValueError(f"sample_rate_hz must be positive, got {sample_rate_hz}")
        return bx, li, lf, wgt, pairs

    def solve(self, buoy_xyz, lag_int, lag_frac, sample_rate_hz: float, weight=None,
              pairs: Optional[np.ndarray] = None, max_iter: int = 60):
        """Batched hyperbolic position solve (rmx_solve_batch), host arrays in and out.
        buoy_xyz [B][3] ECEF metres; lag_int/lag_frac [W][P] as returned by correlate().
        weight: None (every measurement counts 1), float [W][P], or 1-D of length P = one row for all windows, broadcast
        to [W][P].  pairs: None (all i < j in nested-loop order, P = B (B - 1) / 2) or int [P][2].
        Returns (pos float64 [W][3], cost float64 [W], iters int32 [W]).
        The C entry reads W * P elements from each of lag_int, lag_frac and weight, so every shape is checked here first:
        a ValueError that names the argument, before any C call."""
        bx, li, lf, wgt, pairs = self._solve_request(buoy_xyz, lag_int, lag_frac, sample_rate_hz, weight, pairs, max_iter)
        W, P = li.shape
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
        pos = np.zeros((W, 3), np.float64)
        cost = np.zeros(W, np.float64)
        iters = np.zeros(W, np.int32)
        if W == 0:
            return pos, cost, iters
        self._check(self._lib.rmx_solve_batch(
            self._ctx, vp(bx), bx.shape[0], vp(pairs), P, vp(li), vp(lf), vp(wgt), float(sample_rate_hz), W, int(max_iter),
            vp(pos), vp(cost), vp(iters), 0))
        return pos, cost, iters

    def solve_fix(self, buoy_xyz, lag_int, lag_frac, sample_rate_hz: float, weight=None,
                  pairs: Optional[np.ndarray] = None, max_iter: int = 60, plane=None, residuals: bool = False) -> SolveFix:
        """solve() with a surface constraint and the information at the fix (rmx_solve_batch_fix), host arrays in and out.
        buoy_xyz, lag_int, lag_frac, weight, pairs, max_iter: as for solve(); with plane=None pos, cost and iters are
        solve()'s bit for bit.  plane: None (three unknowns) or 9 floats = origin, e1, e2 in ECEF, e1 and e2 orthonormal to
        1e-9 (GeodeticCalculator.tangent_plane): the fix is held to that plane, two unknowns.  residuals=True also returns
        every pair's residual in metres.
        Returns SolveFix(pos [W][3], cost [W], iters [W], info, cov [W][6] (xx xy xz yy yz zz, ECEF) or, with a plane,
        [W][3] (11 12 22, plane coordinates), resid [W][P] or None).  Where the information is singular cov is inf on its
        diagonal and 0 off it.  With weight = lag_weight(lag_sigma(quality), ...) cov is the covariance of the fix under
        independent pair errors (error_ellipse draws it) and cost a chi-square; all pairs of B stations share receivers, so
        that covariance is optimistic.  Every shape is checked here first, as in solve(): a ValueError that names the
        argument, before any C call."""
        bx, li, lf, wgt, pairs = self._solve_request(buoy_xyz, lag_int, lag_frac, sample_rate_hz, weight, pairs, max_iter)
        W, P = li.shape
        pl = None
        if plane is not None:
            pl = np.ascontiguousarray(plane, dtype=np.float64).reshape(-1)
            if pl.size != 9:
                raise ValueError(f"plane must be None or 9 values (origin, e1, e2), got shape {np.shape(plane)}")
            if not np.all(np.isfinite(pl)):
                raise ValueError("plane must be finite")
            e1, e2 = pl[3:6], pl[6:9]
            if abs(math.sqrt(e1 @ e1) - 1.0) > 1e-9 or abs(math.sqrt(e2 @ e2) - 1.0) > 1e-9 or abs(e1 @ e2) > 1e-9:
                raise ValueError("plane: e1 and e2 must be orthonormal to 1e-9")
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
        n_sym = 6 if pl is None else 3
        out = SolveFix(np.zeros((W, 3), np.float64), np.zeros(W, np.float64), np.zeros(W, np.int32),
                       np.zeros((W, n_sym), np.float64), np.zeros((W, n_sym), np.float64),
                       np.zeros((W, P), np.float64) if residuals else None)
        if W == 0:
            return out
        self._check(self._lib.rmx_solve_batch_fix(
            self._ctx, vp(bx), bx.shape[0], vp(pairs), P, vp(li), vp(lf), vp(wgt), float(sample_rate_hz), vp(pl), W,
            int(max_iter), vp(out.pos), vp(out.cost), vp(out.iters), vp(out.info), vp(out.cov), vp(out.resid), 0))
        return out

    def detect(self, iq: np.ndarray, threshold_db: float = -70.0, distance: int = 10, dc_exclude_bins: float = 0.0,
               min_confidence: float = 0.3, max_peaks: int = 2048):
        """Spectral detection (rmx_detect_batch), host arrays in and out.  iq: complex64 [W][N] (or uint8
        [W][2N]).  Returns a list of W tuples (bins int32, power_db, snr_db, confidence float32 arrays,
        noise_floor_db float).  distance is rounded up, as scipy.signal.find_peaks does, and must be >= 1."""
        if not distance >= 1:
            raise ValueError(f"distance must be >= 1, got {distance}")
        # (any distance >= n_samples acts as n_samples; beyond the int range of the ABI the value is capped there)
        dist = math.ceil(distance) if distance < 2**31 - 1 else 2**31 - 1
        iq = np.asarray(iq)
        flags = 0
        if iq.dtype == np.uint8:
            flags |= RMX_IN_U8
            W, N = iq.shape[0], iq.shape[1] // 2
        else:
            iq = np.ascontiguousarray(iq, dtype=np.complex64)
            W, N = iq.shape
        iq = np.ascontiguousarray(iq)
        cnt = np.zeros(W, np.int32)
        bins = np.zeros((W, max_peaks), np.int32)
        pw = np.zeros((W, max_peaks), np.float32)
        snr = np.zeros((W, max_peaks), np.float32)
        conf = np.zeros((W, max_peaks), np.float32)
        floor = np.zeros(W, np.float32)
        if W == 0:
            return []
        vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        self._check(self._lib.rmx_detect_batch(self._ctx, vp(iq), W, N, float(threshold_db), dist,
                                               float(dc_exclude_bins), float(min_confidence), int(max_peaks), vp(cnt),
                                               vp(bins), vp(pw), vp(snr), vp(conf), vp(floor), flags))
        out = []
        for w in range(W):
            n = min(int(cnt[w]), max_peaks)
            out.append((bins[w, :n].copy(), pw[w, :n].copy(), snr[w, :n].copy(), conf[w, :n].copy(), float(floor[w])))
        return out

    def caf_device(self, iq_ptr: int, n_windows: int, doppler_cps, dop_ptr: int, lag_int_ptr: int,
                   lag_frac_ptr: int, peak_ptr: int, pairs: Optional[np.ndarray] = None, u8: bool = False, lag_bounds=None,
                   band=None, whiten: bool = False, dop_frac_ptr: int = 0, refine: int = 0, quality_ptr: int = 0, integrate=None):
        """rmx_caf_batch / rmx_caf_batch_request / rmx_caf_batch_quality with device pointers in and out (the Doppler grid,
        the pair list, the bounds and the bands stay host arrays; the library keeps its own copies); asynchronous on the
        ctx stream.  dop_frac_ptr: 0, or a device buffer of [n_windows][P] float32 for the sub-grid Doppler estimate.
        refine: as for caf(); quality_ptr: 0, or a device buffer of [n_windows][P][4] float32 for the quality figures.
        integrate: as for caf() (rmx_caf_batch_integrated): every output buffer is then [n_windows // K][P] (quality
        [n_windows // K][P][4]) and per-group lag_bounds are [n_windows // K][P][2]."""
        U = check_refine(refine) if refine else 0   # (in front of integrate here; the search without it pays for no check)
        vp, flags = C.c_void_p, _DEVICE | (RMX_IN_U8 if u8 else 0)
        if integrate is None and not U and lag_bounds is None and band is None and not whiten and not dop_frac_ptr \
                and not quality_ptr:   # the plain call, as ever, pays for no request: bench.py times it on a 13 us kernel
            pairs, pp, P = self._pairs_arg(pairs)
            dc = np.ascontiguousarray(doppler_cps, dtype=np.float64).reshape(-1)
            self._check(self._lib.rmx_caf_batch(self._ctx, vp(iq_ptr), n_windows, pp, P, dc.ctypes.data_as(vp), dc.shape[0],
                                                vp(dop_ptr), vp(lag_int_ptr), vp(lag_frac_ptr), vp(peak_ptr), flags))
            return
        req = lag_request("caf", self.n_buoys, n_windows, pairs, lag_bounds, band, whiten, integrate, U, bool(quality_ptr),
                          doppler_cps, bool(dop_frac_ptr))
        self._call(req, vp(iq_ptr), (vp(dop_ptr), vp(dop_frac_ptr) if dop_frac_ptr else None, vp(lag_int_ptr), vp(lag_frac_ptr),
                                     vp(peak_ptr), vp(quality_ptr) if quality_ptr else None), flags)

    def caf_bands_device(self, iq_ptr: int, n_windows: int, doppler_cps, bands, dop_ptr: int, lag_int_ptr: int, lag_frac_ptr: int,
                         peak_ptr: int, pairs: Optional[np.ndarray] = None, u8: bool = False, lag_bounds=None,
                         whiten: bool = False, dop_frac_ptr: int = 0):
        """caf_bands() with device pointers in and out (the Doppler grid, the bands, the pair list and the bounds stay host
        arrays; the library keeps its own copies); asynchronous on the ctx stream.  Every output buffer is
        [n_windows][M][P]; dop_frac_ptr: 0, or a device buffer of that many float32 for the sub-grid Doppler estimate."""
        req = lag_request("caf_bands", self.n_buoys, n_windows, pairs, lag_bounds, bands, whiten, doppler_cps=doppler_cps,
                          fine=bool(dop_frac_ptr))
        vp = C.c_void_p
        self._call(req, vp(iq_ptr), (vp(dop_ptr), vp(dop_frac_ptr) if dop_frac_ptr else None, vp(lag_int_ptr), vp(lag_frac_ptr),
                                     vp(peak_ptr), None), _DEVICE | (RMX_IN_U8 if u8 else 0))

    def correlate_device(self, iq_ptr: int, n_windows: int, lag_int_ptr: int, lag_frac_ptr: int,
                         peak_ptr: int, pairs: Optional[np.ndarray] = None, u8: bool = False, lag_bounds=None,
                         band=None, whiten: bool = False, integrate: int = 1, refine: int = 0, quality_ptr: int = 0):
        """Device pointers in and out (inputs already resident in HBM); asynchronous on the ctx
        stream.  lag_bounds, band, whiten, integrate, refine: as for correlate() (host arrays; the library keeps its own
        copies; with integrate = K the three outputs are [n_windows // K][P]).  quality_ptr: 0, or a device buffer of
        [n_windows // K][P][4] float32 for the quality figures (rmx_xcorr_batch_quality)."""
        vp, flags = C.c_void_p, _DEVICE | (RMX_IN_U8 if u8 else 0)
        if pairs is None and lag_bounds is None and band is None and not whiten and not quality_ptr \
                and integrate.__class__ is int and integrate == 1 and refine.__class__ is int and refine == 0:
            # the plain call pays for no request either (an int 1 and an int 0 pass their checks for any batch)
            self._check(self._lib.rmx_xcorr_batch(self._ctx, vp(iq_ptr), n_windows, None, self.n_buoys * (self.n_buoys - 1) // 2,
                                                  vp(lag_int_ptr), vp(lag_frac_ptr), vp(peak_ptr), flags))
            return
        req = lag_request("xcorr", self.n_buoys, n_windows, pairs, lag_bounds, band, whiten, integrate, refine, bool(quality_ptr))
        self._call(req, vp(iq_ptr), (None, None, vp(lag_int_ptr), vp(lag_frac_ptr), vp(peak_ptr),
                                     vp(quality_ptr) if quality_ptr else None), flags)
