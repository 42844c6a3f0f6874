"""Host-side mirror of the reference's ``tdoa_processor.py`` interface, with the pair loop's time
difference measured from IQ on the GPU.

Same public names, argument meaning and error behaviour as the reference module so that
``central_processor.py`` / the reference's tests can switch imports:

  reference item (tdoa_processor.py)                      here
  -----------------------------------------------------  ------------------------------------------
  BuoyPosition / SignalDetection / TDoAMeasurement /      same field names and order (:24-69);
  TriangulationResult dataclasses                          SignalDetection gains two OPTIONAL trailing
                                                           fields (iq_samples, sample_rate_hz,
                                                           center_freq_hz, bandwidth_hz)
  GeodeticCalculator (:71-136)                             same statics (spherical ECEF, R=6378137)
  TDoACalculator.calculate_tdoa_measurements (:146-198)    same pair order / skips / confidence;
                                                           ``time_diff_ns`` (:166) becomes
                                                           window-start difference + xcorr lag when
                                                           every detection carries IQ
  HyperbolicPositioning.triangulate_position (:218-328)    same objective, BFGS, result fields
  TDoAProcessor (:330-465)                                 same ctor / register_buoy /
                                                           process_signal_detections / status

Without IQ on the detections every number equals the reference's (pinned by
tests/golden/tdoa_conventions.json).  With IQ the lag comes from ``xcorr.XcorrEngine`` (HIP, gfx950);
there is no CPU fallback and no silent degradation to timestamps: if IQ is supplied and the HIP library
or a GPU is missing -- or only some detections of a group carry IQ, or their windows differ in length, dtype or
sample rate -- the seam logs the error on ``...TDoACalculator`` and yields no measurements for that group (the reference's log-and-return convention, tdoa_processor.py:151-153);
``TDoACalculator.measure_lags`` itself raises (ImportError / RmxError).
"""
from __future__ import annotations

import logging
import math
from dataclasses import dataclass
from datetime import datetime, timezone
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

logger = logging.getLogger(__name__)

_C = 299792458.0


# --------------------------------------------------------------------------------------------------
# data model (field names/order: tdoa_processor.py:24-69; tests construct these positionally)
# --------------------------------------------------------------------------------------------------
@dataclass
class BuoyPosition:
    buoy_id: str
    lat: float
    lng: float
    altitude: float = 0.0
    timing_accuracy_ns: int = 100000


@dataclass
class SignalDetection:
    buoy_id: str
    frequency_mhz: float
    signal_strength_dbm: float
    timestamp_utc: str
    gps_timestamp_ns: int
    lat: float
    lng: float
    confidence: float
    signal_type: str = "unknown"
    # extension (not in the reference): the capture window this detection was made on.
    # gps_timestamp_ns is then the time tag of the window's first sample.
    iq_samples: Optional[Any] = None          # np.ndarray complex64 [N] or raw uint8 [2N]
    sample_rate_hz: Optional[float] = None
    # the capture's tuning (its centre frequency) and the emitter's bandwidth (the reference's wire records carry
    # bandwidth_hz, iq_stream_client.py:46-60): what TDoACalculator(band_limit=True) derives a group's band from
    center_freq_hz: Optional[float] = None
    bandwidth_hz: Optional[float] = None


@dataclass
class TDoAMeasurement:
    buoy1_id: str
    buoy2_id: str
    time_difference_ns: int        # buoy2 - buoy1; > 0 when buoy2 received later
    distance_difference_m: float
    confidence: float
    frequency_mhz: float
    # extension: TDoACalculator(doppler_search_hz=...) -- the estimated frequency offset of buoy2's copy of the signal
    # against buoy1's, in hertz (the two receivers' oscillator difference plus any Doppler); None without the search
    frequency_offset_hz: Optional[float] = None


@dataclass
class TriangulationResult:
    estimated_lat: float
    estimated_lng: float
    estimated_altitude: float
    accuracy_meters: float
    confidence: float
    frequency_mhz: float
    signal_type: str
    timestamp_utc: str
    contributing_buoys: List[str]
    tdoa_measurements: List[TDoAMeasurement]
    method: str

    @property
    def accuracy_estimate_meters(self) -> float:
        """Name central_processor.py:434 reads (absent in the reference: SURVEY.md section 0.2)."""
        return self.accuracy_meters


class GeodeticCalculator:
    """Spherical-earth helpers with the reference's constants (tdoa_processor.py:71-136)."""

    EARTH_RADIUS_M = 6378137.0

    @staticmethod
    def lat_lng_to_xyz(lat: float, lng: float, alt: float = 0.0) -> Tuple[float, float, float]:
        phi, lam = math.radians(lat), math.radians(lng)
        r = GeodeticCalculator.EARTH_RADIUS_M + alt
        c = math.cos(phi)
        return r * c * math.cos(lam), r * c * math.sin(lam), r * math.sin(phi)

    @staticmethod
    def xyz_to_lat_lng(x: float, y: float, z: float) -> Tuple[float, float, float]:
        rho = math.sqrt(x * x + y * y)
        return (math.degrees(math.atan2(z, rho)), math.degrees(math.atan2(y, x)),
                math.sqrt(x * x + y * y + z * z) - GeodeticCalculator.EARTH_RADIUS_M)

    @staticmethod
    def tangent_plane(lat: float, lng: float, alt: float = 0.0):
        """(origin, east, north) in ECEF of the plane that touches this class's sphere, lifted to `alt`, at (lat, lng):
        three 3-tuples, east and north unit vectors.  origin + east + north, flattened, is the `plane` of
        XcorrEngine.solve_fix, with u1 metres east and u2 metres north of the origin.
        The sphere sags below the plane by d^2 / 2R at distance d from the origin: 0.7 m at 3 km, 7.8 m at 10 km, 80 m at
        32 km.  A fix held to the plane is that much too high there.  For stations near the surface that is harmless: a
        range difference between two of them barely moves when the emitter's altitude does (the lines of sight are nearly
        horizontal, so the altitude column of the Jacobian is nearly zero), which is the same fact that makes altitude
        unobservable for such a fleet and the reason to hold it fixed at all."""
        phi, lam = math.radians(lat), math.radians(lng)
        sp, cp, sl, cl = math.sin(phi), math.cos(phi), math.sin(lam), math.cos(lam)
        return (GeodeticCalculator.lat_lng_to_xyz(lat, lng, alt), (-sl, cl, 0.0), (-sp * cl, -sp * sl, cp))

    @staticmethod
    def distance_3d(lat1, lng1, alt1, lat2, lng2, alt2) -> float:
        a = GeodeticCalculator.lat_lng_to_xyz(lat1, lng1, alt1)
        b = GeodeticCalculator.lat_lng_to_xyz(lat2, lng2, alt2)
        return math.sqrt(sum((q - p) ** 2 for p, q in zip(a, b)))

    @staticmethod
    def bearing_distance(lat1, lng1, lat2, lng2) -> Tuple[float, float]:
        p1, p2 = math.radians(lat1), math.radians(lat2)
        dl = math.radians(lng2 - lng1)
        h = math.sin((p2 - p1) / 2) ** 2 + math.cos(p1) * math.cos(p2) * math.sin(dl / 2) ** 2
        dist = GeodeticCalculator.EARTH_RADIUS_M * 2 * math.atan2(math.sqrt(h), math.sqrt(1 - h))
        brg = math.atan2(math.sin(dl) * math.cos(p2),
                         math.cos(p1) * math.sin(p2) - math.sin(p1) * math.cos(p2) * math.cos(dl))
        return (math.degrees(brg) + 360) % 360, dist


_DEFAULTS = {"lag_bounds": None, "band": None, "whiten": False, "integrate": 1, "refine": 0, "quality": False}


def _named(**options) -> dict:
    """Only the options that are not at their defaults, as keywords: an engine (or measure_lags, or a stub of either) that
    does not know an option still serves every call that does not ask for it."""
    return {k: v for k, v in options.items() if v is not None and (isinstance(v, np.ndarray) or v != _DEFAULTS[k])}


# --------------------------------------------------------------------------------------------------
# the seam: pairwise TDoA
# --------------------------------------------------------------------------------------------------
class TDoACalculator:
    SPEED_OF_LIGHT = _C  # tdoa_processor.py:141
    MAX_ENGINES = 4      # engines kept alive (one rmx_ctx each: device scratch), least recently used evicted

    LAG_GUARD_SAMPLES = 2   # bound_lags: samples added on either side of the physical lag interval
    DEFAULT_BANDWIDTH_HZ = 10e3   # band_limit: a detection without bandwidth_hz (the reference's default, central_processor.py:52)

    def __init__(self, device: int = 0, devices: Optional[Sequence[int]] = None, min_cut_samples: int = 128,
                 bound_lags: bool = False, band_limit: bool = False, whiten: bool = False, integrate: int = 1,
                 refine: int = 0, min_psr: Optional[float] = None, correlation_confidence: bool = False,
                 doppler_search_hz: Optional[Tuple[float, float]] = None, share_captures: bool = False,
                 share_qualified: bool = False, share_integrated: bool = False, share_doppler: bool = False):
        """device: the GPU of a single-device calculator (the default).  devices: a list of GPUs, or "all" for every
        visible one -- with more than one entry a batch of windows / frequency groups is block-sharded over them by
        `multi.MultiXcorrEngine` (one rmx_ctx and one host thread per device, no collective).  min_cut_samples: the
        shortest window a group may be CUT to when its windows differ in length (see _group_windows); 128 is the
        shortest cut the reference's own clipping can produce.  bound_lags: search each pair's peak only over the lags
        a geometry can produce (lag_bounds below: |dt| <= baseline / c + rss of the two timing accuracies, plus a guard
        of LAG_GUARD_SAMPLES); a plain attribute, so `TDoAProcessor().tdoa_calculator.bound_lags = True` works too.
        band_limit: correlate each group over its emitter's band only (band() below: the detections' frequencies and
        bandwidths around the capture's centre frequency), so that two transmitters heard in one capture each get their
        own lags.  whiten: PHAT weighting of every group with IQ (no strong spectral line -- the receivers' DC offset, LO
        leakage -- dominates the peak).  Both plain attributes, off by default.
        integrate: K > 1 cuts every group's [B][N] windows into K consecutive segments of N // K samples and measures ONE
        lag per pair on the sum of the segments' squared correlation magnitudes (noncoherent integration,
        rmx_xcorr_batch_integrated): receivers with free-running oscillators stay coherent over a short segment only.
        The segments of one capture share its start tag, so they share the lag; bound_lags and band_limit derive their
        values for N // K.  A group whose segments cannot be formed (segment_length below) yields no measurements.  A
        plain attribute, 1 (off) by default.
        refine: U in (0, 2, 4, 8, 16); U > 0 takes every lag's sub-sample part from the band-limited interpolant of the
        correlation on a grid of 1 / U samples around the integer peak (rmx_xcorr_batch_refined) instead of the
        three-point parabola, whose bias on a band-limited peak is up to 0.15 samples.  The refined lag flows into
        time_difference_ns unchanged in meaning.  A plain attribute, 0 (off) by default.
        min_psr, correlation_confidence: qualify every measured lag by the correlation itself (rmx_xcorr_batch_quality).
        min_psr: a pair whose peak-to-floor ratio lies below it is dropped and logged -- a dead or drowned receiver's lag
        is noise (xcorr.psr_threshold gives the value for a false-alarm rate).  correlation_confidence: the measurement's
        confidence, built from the detector's confidence and a timing term only, is additionally multiplied by the pair's
        coherence in [0, 1].  Plain attributes; None and False (off) by default: the engine is then called exactly as
        before.  Neither applies to groups without IQ (the time-tag arithmetic has no correlation).
        doppler_search_hz: (max_hz, step_hz); every group with IQ goes through the Doppler search (rmx_caf_batch_request)
        on the symmetric grid 0, +-step_hz, ... up to max_hz instead of the plain correlation: receivers with free-running
        oscillators decorrelate over a long window unless the later buoy's copy is de-rotated first.  bound_lags,
        band_limit and whiten apply as they do without it, and every measurement carries the estimated offset
        (frequency_offset_hz: the winning hypothesis plus the sub-grid parabola).  The search has no integration,
        refinement or quality: together with integrate > 1, refine > 0, min_psr or correlation_confidence the
        construction raises ValueError.  None (off) by default: every other path is then as before.
        share_captures: together with band_limit, TDoAProcessor.process_signal_detections correlates frequency groups
        that were cut from ONE capture (byte-identical windows, identical lag bounds) as one window under several bands
        (rmx_xcorr_batch_bands: one upload and one forward transform per buoy instead of one per emitter); the lags are
        those of the separate calls.  Not for groups under integrate, refine, min_psr / correlation_confidence or
        doppler_search_hz, which go the usual way (share_qualified, share_integrated and share_doppler, below, admit them).  A plain attribute, False (off) by default: the engine is then called
        exactly as before.
        share_qualified: together with share_captures, shared captures are also correlated as one window under several
        bands when refine > 0, min_psr or correlation_confidence is set (rmx_xcorr_batch_bands_quality: the fine lag search
        and the quality figures per (capture, band, pair), still one forward transform per buoy); min_psr and the
        correlation confidence are applied per (capture, band, pair), and the measurements are those of the separate
        calls, in the same order.  Groups under integrate > 1 or doppler_search_hz still go the usual way.  A plain
        attribute, False (off) by default: nothing changes then.
        share_integrated: together with share_captures, shared captures are correlated as one window under several bands
        under integrate > 1 too (rmx_xcorr_batch_bands_integrated): the capture is cut ONCE into its K segments, exactly as
        the separate calls cut it, each member's band is repeated over its K segments, and lag bounds and the
        segment_length checks are as without sharing.  With refine > 0, min_psr or correlation_confidence it needs
        share_qualified as well.  The Doppler search stays out.  A plain attribute, False (off) by default: share_captures
        and share_qualified alone still stand back for integration.
        share_doppler: together with band_limit, share_captures and doppler_search_hz, shared captures go through ONE Doppler
        search under several bands (rmx_caf_batch_bands: one upload, and the forward transforms of every hypothesis once
        per buoy instead of once per emitter); the measurements, frequency_offset_hz included, are those of the separate
        searches, in the same order.  A plain attribute, False (off) by default: groups under doppler_search_hz then go
        the usual way, one full search per emitter."""
        from .xcorr import check_refine
        self.logger = logging.getLogger(__name__ + ".TDoACalculator")
        self.device = device
        self.devices = devices
        self.min_cut_samples = int(min_cut_samples)
        self.bound_lags = bool(bound_lags)
        self.band_limit = bool(band_limit)
        self.whiten = bool(whiten)
        self.share_captures = bool(share_captures)
        self.share_qualified = bool(share_qualified)
        self.share_integrated = bool(share_integrated)
        self.share_doppler = bool(share_doppler)
        self.integrate = int(integrate)
        self.refine = check_refine(refine)
        self.min_psr = None if min_psr is None else float(min_psr)
        self.correlation_confidence = bool(correlation_confidence)
        self.doppler_search_hz = None
        if doppler_search_hz is not None:
            try:
                max_hz, step_hz = (float(v) for v in doppler_search_hz)
            except (TypeError, ValueError):
                raise ValueError(f"doppler_search_hz must be (max_hz, step_hz), got {doppler_search_hz!r}") from None
            if not (step_hz > 0.0 and max_hz >= step_hz and math.isfinite(max_hz)):
                raise ValueError(f"doppler_search_hz = (max_hz, step_hz) needs 0 < step_hz <= max_hz, got {doppler_search_hz!r}")
            if 2 * int(math.floor(max_hz / step_hz + 1e-9)) + 1 > 4096:
                raise ValueError(f"doppler_search_hz = {doppler_search_hz!r} asks for more than 4096 hypotheses")
            for name, on in (("integrate", self.integrate > 1), ("refine", self.refine > 0), ("min_psr", self.min_psr is not None),
                             ("correlation_confidence", self.correlation_confidence)):
                if on:
                    raise ValueError(f"doppler_search_hz and {name} cannot be combined: the Doppler search has no "
                                     f"integration, refinement or quality")
            self.doppler_search_hz = (max_hz, step_hz)
        self._engines: Dict[Tuple[int, int], Any] = {}   # insertion order = recency
        self._tconf: Dict[Tuple[int, int], float] = {}

    # -- GPU engine cache ------------------------------------------------------------------------
    def _engine(self, n_buoys: int, n_samples: int, n_windows: int = 1):
        from . import xcorr  # raises ImportError loudly if the HIP library is not built
        key = (n_buoys, n_samples)
        eng = self._engines.pop(key, None)
        if eng is None or eng.max_windows < n_windows:
            if eng is not None:
                eng.close()
            # head room: the number of frequency groups varies from call to call at the seam, and an engine is only
            # rebuilt (milliseconds: tables, scratch) when a batch exceeds every earlier one by a power of two
            cap = 8
            while cap < n_windows:
                cap *= 2
            n_windows = cap
            devs = self.devices
            if isinstance(devs, str):
                if devs != "all":
                    raise ValueError('devices must be a list of device indices or "all"')
                devs = list(range(xcorr.device_count()))
            if devs is not None and len(devs) > 1:
                from . import multi
                eng = multi.MultiXcorrEngine(n_buoys, n_samples, max(n_windows, 1), devices=devs)
            else:
                eng = xcorr.XcorrEngine(n_buoys, n_samples, max(n_windows, 1),
                                        device=self.device if not devs else int(devs[0]))
        self._engines[key] = eng                         # most recently used last
        while len(self._engines) > self.MAX_ENGINES:
            old = next(iter(self._engines))
            self._engines.pop(old).close()
        return eng

    def close(self):
        for eng in self._engines.values():
            eng.close()
        self._engines.clear()

    def _wants_quality(self) -> bool:
        return self.min_psr is not None or self.correlation_confidence

    def doppler_grid(self, fs: float) -> np.ndarray:
        """doppler_search_hz: the symmetric grid of hypotheses at sample rate fs, float64 in cycles per sample"""
        max_hz, step_hz = self.doppler_search_hz
        n = int(math.floor(max_hz / step_hz + 1e-9))
        return np.arange(-n, n + 1, dtype=np.float64) * (step_hz / float(fs))

    def measure_lags(self, iq, pairs=None, lag_bounds=None, band=None, whiten=False, integrate=1, refine=0, quality=False,
                     doppler_cps=None, bands=None):
        """Batched hot path.  iq: complex64 [W][B][N] (or uint8 [W][B][2N]) ->
        (lag_int [W][P], lag_frac [W][P], peak [W][P]); lag = delay(j) - delay(i) in samples.
        A leading channel axis is a batch axis: [C][W][B][N] -> three [C][W][P] arrays (channels and
        windows are independent units, tdoa_processor.py:363).  lag_bounds: None, or int [P][2] / [W][P][2] (with a
        channel axis: [C][W][P][2]) = the lag window [lo, hi] each pair's peak is searched in.  band: None, or float [2] /
        [W][2] (with a channel axis: [C][W][2]) = the band [lo, hi] in cycles per sample kept of the cross-spectrum;
        whiten: PHAT weighting (rmx_xcorr_batch_weighted).  integrate: K >= 1 consecutive windows per group, one lag
        per pair and group (rmx_xcorr_batch_integrated): W must be a multiple of K, the results and per-window lag_bounds
        have W // K rows where they have W otherwise; band stays per window.  refine: U of the fine lag search
        (rmx_xcorr_batch_refined), 0 for none.  quality: True returns a fourth array [W][P][4] (with a channel axis:
        [C][W][P][4]), the quality figures of every lag (rmx_xcorr_batch_quality).
        doppler_cps: None, or the hypotheses of a Doppler search in cycles per sample (a uniformly spaced grid): the call
        goes to caf() (rmx_caf_batch_request) with the same lag_bounds, band and whiten, and returns (lag_int, lag_frac,
        peak, dop_idx int32, doppler float64 in cycles per sample = xcorr.doppler_estimate of the winner and its sub-grid
        part).  Not together with integrate > 1, refine > 0 or quality (ValueError).
        bands: None, or float [W][M][2] (with a channel axis: [C][W][M][2]): every window under M bands with one forward
        transform per buoy (rmx_xcorr_batch_bands); the three results are then [W][M][P] ([C][W][M][P]), lag_bounds stay
        per (window, pair).  Not together with band, integrate > 1, refine > 0, quality or doppler_cps (ValueError)."""
        from .xcorr import check_refine
        refine = check_refine(refine)
        if bands is not None:
            for name, on in (("band", band is not None), ("integrate", integrate != 1), ("refine", refine > 0),
                             ("quality", bool(quality)), ("doppler_cps", doppler_cps is not None)):
                if on:
                    raise ValueError(f"bands and {name} cannot be combined: the multi-band correlation takes one band set "
                                     f"and has no integration, refinement, quality or Doppler search")
            return self.measure_band_lags(iq, bands, pairs, lag_bounds, whiten, integrate=integrate)
        if doppler_cps is not None:
            for name, on in (("integrate", integrate != 1), ("refine", refine > 0), ("quality", bool(quality))):
                if on:
                    raise ValueError(f"doppler_cps and {name} cannot be combined: the Doppler search has no integration, "
                                     f"refinement or quality")
        iq, integrate, fold, unfold = self._channels(iq, integrate)
        eng = self._engine(iq.shape[1], iq.shape[2] // 2 if iq.dtype == np.uint8 else iq.shape[2], iq.shape[0])
        lb, bd = fold(lag_bounds, 4, True), fold(band, 3)
        if doppler_cps is not None:
            from .xcorr import doppler_estimate
            dop, dfrac, li, lf, pk = eng.caf(iq, doppler_cps, pairs, lag_bounds=lb, band=bd, whiten=bool(whiten), fine=True)
            return unfold((li, lf, pk, dop, doppler_estimate(doppler_cps, dop, dfrac)))
        if band is not None or whiten or integrate > 1 or refine > 0 or quality:
            return unfold(eng.correlate(iq, pairs, lag_bounds=lb, band=bd, whiten=bool(whiten),
                                        **_named(integrate=integrate, refine=refine, quality=bool(quality))))
        return unfold(eng.correlate(iq, pairs, **_named(lag_bounds=lb)))

    def measure_band_lags(self, iq, bands, pairs=None, lag_bounds=None, whiten=False, refine=0, quality=False, integrate=1,
                          doppler_cps=None):
        """measure_lags(bands=...) with the fine lag search and the quality figures (rmx_xcorr_batch_bands_quality): iq
        complex64 [W][B][N] (or uint8 [W][B][2N]) under bands [W][M][2] -> (lag_int, lag_frac, peak), each [W][M][P], and
        with quality=True a fourth array [W][M][P][4]; one forward transform per (window, buoy).  A leading channel axis is
        a batch axis, as in measure_lags: [C][W][B][N] with bands [C][W][M][2] (and lag_bounds [C][W][P][2]) -> [C][W][M][P]
        ([C][W][M][P][4]).  refine: U in (0, 2, 4, 8, 16).  With refine=0 and quality=False it is measure_lags(bands=...).
        integrate: K >= 1 consecutive windows per group, one lag per (group, band, pair) (rmx_xcorr_batch_bands_integrated):
        W must be a multiple of K -- with a channel axis, every channel's W --, the results and per-group lag_bounds are
        [W // K][.], the bands stay per window.
        doppler_cps: None, or the hypotheses of a Doppler search in cycles per sample (a uniformly spaced grid): the call
        goes to caf_bands() (rmx_caf_batch_bands) with the same lag_bounds and whiten, and returns (lag_int, lag_frac, peak,
        dop_idx int32, doppler float64 in cycles per sample), each [W][M][P], as measure_lags(doppler_cps=...) returns them
        per band.  Not together with integrate > 1, refine > 0 or quality (ValueError)."""
        from .xcorr import check_refine
        refine = check_refine(refine)
        if doppler_cps is not None:
            for name, on in (("integrate", integrate != 1), ("refine", refine > 0), ("quality", bool(quality))):
                if on:
                    raise ValueError(f"doppler_cps and {name} cannot be combined: the Doppler search under several bands has "
                                     f"no integration, refinement or quality")
        iq, integrate, fold, unfold = self._channels(iq, integrate)
        eng = self._engine(iq.shape[1], iq.shape[2] // 2 if iq.dtype == np.uint8 else iq.shape[2], iq.shape[0])
        lb, bs = fold(lag_bounds, 4, True), fold(np.asarray(bands), 4)
        if bs.ndim != 3 or bs.shape[0] != iq.shape[0] or bs.shape[2] != 2:
            raise ValueError(f"bands must be [W][M][2] or [C][W][M][2] for {iq.shape[0]} windows, got shape {np.shape(bands)}")
        if doppler_cps is not None:
            from .xcorr import doppler_estimate
            dop, dfrac, li, lf, pk = eng.caf_bands(iq, doppler_cps, bs, pairs, lag_bounds=lb, whiten=bool(whiten), fine=True)
            return unfold((li, lf, pk, dop, doppler_estimate(doppler_cps, dop, dfrac)))
        return unfold(eng.correlate_bands(iq, bs, pairs, lag_bounds=lb, whiten=bool(whiten),
                                          **_named(refine=refine, quality=bool(quality), integrate=integrate)))

    @staticmethod
    def _channels(iq, integrate):
        """The channel axis of measure_lags and measure_band_lags as a batch axis: iq [W][B][N] or [C][W][B][N] ->
        (iq [W][B][N] or [C W][B][N], K = integrate checked against one channel's W -- groups never straddle two channels --,
        fold, unfold).  fold(value, ndim, exact=False): a per-row option with the channel axis in front (`ndim` dimensions)
        -> [C W]... (exact: [C (W // K)]..., the rows of the results), anything else as an array, None as None.
        unfold(out): every [C (W // K)]... array of a result -> [C][W // K]...; without a channel axis, out itself."""
        from .xcorr import check_integrate
        iq = np.asarray(iq)
        chan = iq.shape[:2] if iq.ndim == 4 else None
        if chan is not None:
            iq = iq.reshape((chan[0] * chan[1],) + iq.shape[2:])
        if iq.ndim != 3:
            raise ValueError(f"iq must be [W][B][N] or [C][W][B][N], got shape {iq.shape}")
        k = check_integrate(integrate, iq.shape[0] if chan is None else chan[1])
        lead = None if chan is None else (chan[0], chan[1] // k)

        def fold(value, ndim, exact=False):
            if value is None:
                return None
            a = np.asarray(value)
            return a.reshape((lead[0] * lead[1] if exact else -1,) + a.shape[2:]) if lead is not None and a.ndim == ndim else a

        def unfold(out):
            return out if lead is None else tuple(a.reshape(lead + a.shape[1:]) for a in out)
        return iq, k, fold, unfold

    @staticmethod
    def _iq_of(det: SignalDetection):
        s = det.iq_samples
        if s is None or det.sample_rate_hz is None:
            return None
        if isinstance(s, (list, tuple)) and len(s) and isinstance(s[0], (str, list, tuple)):
            # the reference's wire form: NumpyEncoder turns every complex into str(obj) (iq_stream_client.py:31-44)
            from .iq_wire import parse_complex_list
            return parse_complex_list(s)
        a = np.asarray(s)
        if a.dtype == np.uint8:
            return a
        return np.ascontiguousarray(a, dtype=np.complex64)

    def _iq_batch_key(self, detections: Sequence[SignalDetection]):
        """(key, stacked [B][N] windows) when every detection of the group carries an IQ window of one
        shape, dtype and sample rate; (None, None) when none does; (False, None) when they disagree."""
        try:
            iqs = [self._iq_of(d) for d in detections]
        except ValueError as e:      # wire data that does not parse (iq_wire.IqWireError): logged, no measurements
            self.logger.error(f"IQ samples of the group cannot be decoded: {e}")
            return False, None
        if all(a is None for a in iqs):
            return None, None
        # IQ was supplied for this group: from here on the time tags alone are never used for it.  A group that
        # cannot be correlated as one [B][N] batch yields no measurements (logged), as an engine failure does.
        if any(a is None for a in iqs):
            self.logger.error("Only some detections of the group carry IQ windows; no TDoA measurements for it")
            return False, None
        rates = {float(d.sample_rate_hz) for d in detections}
        kinds = {(a.dtype.str, a.ndim) for a in iqs}
        if len(kinds) != 1 or len(rates) != 1 or iqs[0].ndim != 1:
            self.logger.error("IQ windows of the group differ in dtype/sample rate; no TDoA measurements for it")
            return False, None
        # Windows that differ in length, or whose length is not a power of two: the reference clips an excerpt at the
        # end of the capture buffer (iq_stream_client.py:306-313: start = max(0, peak - 128), end = min(len, start + 256)),
        # so a peak in the last 128 bins gives e.g. 130 samples beside the other buoys' 256.  Every window keeps its
        # START -- under this build's extension the time tag of a detection that carries IQ dates its window's first
        # sample (SignalDetection above; the reference's own tag is time.time_ns() at detection time,
        # iq_stream_client.py:221, and dates no sample) -- so the group is cut to the largest power of two that every
        # window holds -- the engine's window lengths -- instead of being dropped.  The reference's clipping
        # never leaves fewer than 129 samples, so a cut below min_cut_samples (128) is not one of its excerpts: such a
        # group is refused rather than correlated on a noise-dominated stub.  Windows of one equal
        # power-of-two length >= 16 are the caller's own choice and are not cut.
        per = 2 if iqs[0].dtype == np.uint8 else 1          # uint8: interleaved I, Q
        nmin = min(a.shape[0] // per for a in iqs)
        n = 1 << (max(nmin, 1).bit_length() - 1)
        if nmin < 16:
            self.logger.error(f"IQ windows of the group are too short to correlate ({nmin} samples); no TDoA measurements for it")
            return False, None
        if any(a.shape[0] != n * per for a in iqs):
            if n < self.min_cut_samples:
                self.logger.error(f"IQ windows of the group hold {sorted({a.shape[0] // per for a in iqs})} samples: their "
                                  f"common cut of {n} is below {self.min_cut_samples}; no TDoA measurements for it")
                return False, None
            self.logger.warning(f"IQ windows of the group hold {sorted({a.shape[0] // per for a in iqs})} samples; "
                                f"correlating their first {n}")
            iqs = [a[:n * per] for a in iqs]
        return (len(iqs), iqs[0].dtype.str, iqs[0].shape, next(iter(rates))), np.stack(iqs)

    def lag_bounds(self, detections: Sequence[SignalDetection], buoy_positions: Dict[str, BuoyPosition], n: int,
                   fs: float):
        """bound_lags: the lag window of every pair (i < j, nested-loop order) of one group of windows of n samples at
        fs.  A lag is physical when dt = (d_j.gps_timestamp_ns - d_i.gps_timestamp_ns) / 1e9 + lag / fs satisfies
        |dt| <= D / c + u, D the 3-D distance of the two buoys, u the rss of their timing accuracies (the quantity the
        reference's confidence uses, tdoa_processor.py:200-210); hence
            lo = ceil(fs (-D/c - u - ds)) - g,   hi = floor(fs (D/c + u - ds)) + g,   g = LAG_GUARD_SAMPLES,
        clipped to +-(n - 1).  Returns (bounds int32 [P][2], empty bool [P]): an empty pair (no lag of the window is
        physical) gets the full interval and is flagged; a pair with an unknown buoy position gets the full interval."""
        nd = len(detections)
        nm1 = n - 1
        bounds, empty = [], []
        xyz = {}
        g = self.LAG_GUARD_SAMPLES
        for i in range(nd):
            for j in range(i + 1, nd):
                d1, d2 = detections[i], detections[j]
                p1, p2 = buoy_positions.get(d1.buoy_id), buoy_positions.get(d2.buoy_id)
                if not p1 or not p2:
                    bounds.append((-nm1, nm1))
                    empty.append(False)
                    continue
                for p in (p1, p2):
                    if p.buoy_id not in xyz:
                        xyz[p.buoy_id] = GeodeticCalculator.lat_lng_to_xyz(p.lat, p.lng, p.altitude)
                a, b = xyz[p1.buoy_id], xyz[p2.buoy_id]
                dist = math.sqrt((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 + (a[2] - b[2]) ** 2)
                reach = dist / self.SPEED_OF_LIGHT + math.hypot(p1.timing_accuracy_ns, p2.timing_accuracy_ns) * 1e-9
                ds = (d2.gps_timestamp_ns - d1.gps_timestamp_ns) * 1e-9
                lo = math.ceil(fs * (-reach - ds)) - g
                hi = math.floor(fs * (reach - ds)) + g
                lo, hi = max(lo, -nm1), min(hi, nm1)
                if lo > hi:
                    bounds.append((-nm1, nm1))
                    empty.append(True)
                else:
                    bounds.append((lo, hi))
                    empty.append(False)
        return np.asarray(bounds, np.int32).reshape(-1, 2), np.asarray(empty, bool)

    def band(self, detections: Sequence[SignalDetection], n: int, fs: float):
        """band_limit: the band of one group of windows of n samples at fs, as (band float [2] in cycles per sample or
        None, reason or None).  With every detection's centre frequency fc known:
            [(min(f - bw/2) - fc) / fs, (max(f + bw/2) - fc) / fs]   clipped to +-0.5,
        f = frequency_mhz * 1e6, bw = bandwidth_hz or DEFAULT_BANDWIDTH_HZ (for one bandwidth: f_min - bw/2 .. f_max + bw/2).
        (None, None) when no detection carries a centre frequency (the full band, as without band_limit); (None, reason)
        when the group cannot be band limited: only some detections carry a centre frequency, they disagree, the band
        misses the capture, or it keeps no bin of the 2n-point transform."""
        fcs = [d.center_freq_hz for d in detections]
        if all(f is None for f in fcs):
            return None, None
        if any(f is None for f in fcs):
            return None, "only some detections of the group carry a centre frequency"
        fcs = [float(f) for f in fcs]
        if max(fcs) - min(fcs) > 1.0:
            return None, f"the group's centre frequencies disagree ({min(fcs):.0f} .. {max(fcs):.0f} Hz)"
        fc = fcs[0]
        bws = [self.DEFAULT_BANDWIDTH_HZ if d.bandwidth_hz is None else float(d.bandwidth_hz) for d in detections]
        lo = (min(d.frequency_mhz * 1e6 - bw / 2 for d, bw in zip(detections, bws)) - fc) / fs
        hi = (max(d.frequency_mhz * 1e6 + bw / 2 for d, bw in zip(detections, bws)) - fc) / fs
        if not (math.isfinite(lo) and math.isfinite(hi)) or hi < -0.5 or lo > 0.5 or lo > hi:
            return None, (f"the group's band [{lo:.4f}, {hi:.4f}] cycles per sample misses the capture "
                          f"(centre {fc:.0f} Hz, {fs:.0f} samples/s)")
        lo, hi = max(lo, -0.5), min(hi, 0.5)
        L = 2 * n
        if math.ceil(lo * L) > min(math.floor(hi * L), n - 1):
            return None, f"the group's band [{lo:.6f}, {hi:.6f}] cycles per sample keeps no bin of a {L}-point transform"
        return np.array([lo, hi], np.float64), None

    def segment_length(self, n: int):
        """integrate: the segment length of windows of n samples, as (n // K, None), or (None, reason) when the segments
        cannot be formed: K is not a power of two, does not divide n, or leaves fewer than max(min_cut_samples, 16)
        samples (a segment is a cut of the window, and the engine's shortest window is 16)."""
        k = self.integrate
        if k < 1 or k & (k - 1):
            return None, f"integrate = {k} is not a power of two"
        if n % k:
            return None, f"integrate = {k} does not divide the window length {n}"
        if n // k < max(self.min_cut_samples, 16):
            return None, (f"integrate = {k} leaves segments of {n // k} samples out of {n}, below "
                          f"{max(self.min_cut_samples, 16)}")
        return n // k, None

    def _measure_groups(self, stacked: np.ndarray, lag_bounds=None, band=None, with_quality: bool = False, fs=None):
        """[G][B][N] -> lag [G][P] float64, or None after logging: the reference's seam never raises
        (tdoa_processor.py:151-153) and there is no fallback to time tags once IQ was supplied.  lag_bounds: None, or
        int [G][P][2] (bound_lags); band: None, or float [G][2] (band_limit); whiten applies to every group.
        with_quality: -> (lag [G][P], quality [G][P][4]) instead (min_psr / correlation_confidence), None all the same.
        doppler_search_hz (fs, the groups' sample rate, must be given): -> (lag [G][P], offset in hertz [G][P]) instead."""
        stacked, band, k = self._segments(stacked, band)
        kw = _named(lag_bounds=lag_bounds, integrate=k, band=band, whiten=bool(self.whiten), refine=self.refine)

        def measure():
            if self.doppler_search_hz is not None:
                li, lf, _, _, dop = self.measure_lags(stacked, doppler_cps=self.doppler_grid(fs), **kw)
                return li.astype(np.float64) + lf.astype(np.float64), np.asarray(dop, np.float64) * float(fs)
            if with_quality:
                li, lf, _, qual = self.measure_lags(stacked, quality=True, **kw)
                return li.astype(np.float64) + lf.astype(np.float64), np.asarray(qual)
            li, lf, _ = self.measure_lags(stacked, **kw)
            return li.astype(np.float64) + lf.astype(np.float64)
        return self._logged(measure)

    def _measure_shared(self, stacked: np.ndarray, lag_bounds, bands: np.ndarray, with_quality: bool = False, fs=None):
        """share_captures: [G][B][N] captures, each under the M bands of bands [G][M][2] -> lag [G][M][P] float64, or None
        after logging, as _measure_groups does.  lag_bounds: None, or int [G][P][2].  share_qualified: the calculator's
        refine goes along, and with_quality -> (lag [G][M][P], quality [G][M][P][4]) instead.  share_integrated: under
        integrate = K > 1 every capture is cut into its K segments as _measure_groups cuts it and every band is repeated
        over its capture's segments (the callers checked segment_length and derived lag_bounds and bands for N // K).
        share_doppler (doppler_search_hz; fs, the captures' sample rate, must be given): -> (lag [G][M][P], offset in hertz
        [G][M][P]) instead, from one Doppler search under the M bands."""
        stacked, bands, k = self._segments(stacked, bands)
        more = _named(integrate=k)

        def measure():
            if self.doppler_search_hz is not None:
                li, lf, _, _, dop = self.measure_band_lags(stacked, bands, lag_bounds=lag_bounds, whiten=self.whiten,
                                                           doppler_cps=self.doppler_grid(fs))
                return li.astype(np.float64) + lf.astype(np.float64), np.asarray(dop, np.float64) * float(fs)
            if with_quality:
                li, lf, _, qual = self.measure_band_lags(stacked, bands, lag_bounds=lag_bounds, whiten=self.whiten,
                                                         refine=self.refine, quality=True, **more)
                return li.astype(np.float64) + lf.astype(np.float64), np.asarray(qual)
            if self.refine > 0 or more:
                li, lf, _ = self.measure_band_lags(stacked, bands, lag_bounds=lag_bounds, whiten=self.whiten, refine=self.refine,
                                                   **more)
            else:
                li, lf, _ = self.measure_lags(stacked, lag_bounds=lag_bounds, bands=bands, whiten=self.whiten)
            return li.astype(np.float64) + lf.astype(np.float64)
        return self._logged(measure)

    def _segments(self, stacked: np.ndarray, band):
        """integrate = K > 1: [G][B][N] -> [G K][B][N // K], window g K + s segment s of group g, and the band(s) [G]... repeated
        over each group's K segments (the callers checked segment_length and derived lag_bounds and band(s) for N // K; one
        lag per pair and group comes back, as without integration) -> (stacked, band(s), K); K = 1: as they are."""
        k = self.integrate
        if k <= 1:
            return stacked, band, 1
        g, b, nn = stacked.shape
        stacked = np.ascontiguousarray(stacked.reshape(g, b, k, nn // k).transpose(0, 2, 1, 3)).reshape(g * k, b, nn // k)
        return stacked, None if band is None else np.repeat(np.asarray(band), k, axis=0), k

    def _logged(self, measure):
        """measure(), or None after logging when the library is not built or not loadable (ImportError, OSError) or the
        engine refused the batch or found no device (RmxError): the reference's seam never raises (tdoa_processor.py:151-153).
        Everything else -- programming errors: shapes, types -- surfaces."""
        from .xcorr import RmxError
        try:
            return measure()
        except (ImportError, OSError, RmxError) as e:
            self.logger.error(f"Cross-correlation engine failed: {e}")
            return None

    def _timing_confidence(self, b1: BuoyPosition, b2: BuoyPosition) -> float:
        # exp(-rss(timing accuracies) / 100 us), capped at 1 (tdoa_processor.py:200-210); a handful of distinct values
        key = (b1.timing_accuracy_ns, b2.timing_accuracy_ns)
        c = self._tconf.get(key)
        if c is None:
            if len(self._tconf) > 4096:
                self._tconf.clear()
            c = self._tconf[key] = min(math.exp(-math.hypot(key[0], key[1]) / 100000), 1.0)
        return c

    _calculate_timing_confidence = _timing_confidence  # reference's private name

    _NO_LAG = object()      # calculate_tdoa_measurements inspects the detections itself
    _TIME_TAGS = object()   # the caller already did and found no IQ: the reference's arithmetic (:166)

    def calculate_tdoa_measurements(self, detections: List[SignalDetection],
                                    buoy_positions: Dict[str, BuoyPosition],
                                    _lag=_NO_LAG) -> List[TDoAMeasurement]:
        """The reference's pair loop (tdoa_processor.py:146-198).  `_lag` (private): (lags [P], sample rate) of this
        group, already measured in a batch with other groups by TDoAProcessor; None when that batch failed or the
        group's IQ could not be batched; `_TIME_TAGS` when TDoAProcessor found no IQ on the group.  The tuple may go on
        with the empty-interval flags [P] (or None), the quality figures [P][4] of the group (or None) and the frequency
        offsets in hertz [P] of a Doppler search."""
        out: List[TDoAMeasurement] = []
        nd = len(detections)
        if nd < 2:
            self.logger.warning("Need at least 2 detections for TDoA calculation")
            return out
        lag = None
        fs = None
        empty = None   # bound_lags: pairs whose lag window is empty (skipped below)
        qual = None    # min_psr / correlation_confidence: the quality figures [P][4] of the group's lags
        dop_hz = None  # doppler_search_hz: the estimated frequency offset of every pair [P]
        if _lag is self._NO_LAG:
            key, stacked = self._iq_batch_key(detections)
            if key is False:
                return out
            if key:
                lb = None
                per = 2 if stacked.dtype == np.uint8 else 1
                n_samp = stacked.shape[-1] // per
                if self.integrate != 1:   # the engine sees segments of n_samp // K samples
                    n_samp, why = self.segment_length(n_samp)
                    if why:
                        self.logger.error(f"Cannot integrate the group: {why}; no TDoA measurements for it")
                        return out
                if self.bound_lags:
                    lb, empty = self.lag_bounds(detections, buoy_positions, n_samp, key[3])
                    lb = lb[None]
                band = None
                if self.band_limit:
                    band, why = self.band(detections, n_samp, key[3])
                    if why:
                        self.logger.error(f"Cannot band limit the group: {why}; no TDoA measurements for it")
                        return out
                if self.doppler_search_hz is not None:
                    res = self._measure_groups(stacked[None], lb, None if band is None else band[None], fs=key[3])
                    if res is None:
                        return out
                    res, dop_hz = res[0], res[1][0]
                elif self._wants_quality():
                    res = self._measure_groups(stacked[None], lb, None if band is None else band[None], with_quality=True)
                    if res is None:
                        return out
                    res, qual = res[0], res[1][0]
                else:
                    res = self._measure_groups(stacked[None], lb, None if band is None else band[None])
                    if res is None:
                        return out
                lag, fs = res[0], key[3]
        elif _lag is None:
            return out
        elif _lag is not self._TIME_TAGS:
            lag, fs = _lag[0], _lag[1]
            empty = _lag[2] if len(_lag) > 2 else None
            qual = _lag[3] if len(_lag) > 3 else None
            dop_hz = _lag[4] if len(_lag) > 4 else None
        q = -1
        if lag is not None:
            # the same float64 arithmetic as `round(lag[q] / fs * 1e9)` per pair, done once for the group (numpy scalars make
            # the pair loop four times slower than it needs to be; np.rint and round() both round half to even)
            lag_s = np.asarray(lag, np.float64) / fs
            if not np.all(np.isfinite(lag_s)):           # (a NaN would become INT64_MIN in the cast below)
                self.logger.error("Cross-correlation returned a non-finite lag; no TDoA measurements for the group")
                return out
            lag_ns = np.rint(lag_s * 1e9).astype(np.int64).tolist()
        debug = self.logger.isEnabledFor(logging.DEBUG)
        for i in range(nd):
            for j in range(i + 1, nd):
                q += 1
                d1, d2 = detections[i], detections[j]
                if abs(d1.frequency_mhz - d2.frequency_mhz) > 0.01:
                    continue
                if empty is not None and empty[q]:
                    self.logger.warning("TDoA %s-%s skipped: no lag of the window is physical for this baseline and "
                                        "window-start difference", d1.buoy_id, d2.buoy_id)
                    continue
                dt_ns = d2.gps_timestamp_ns - d1.gps_timestamp_ns
                if lag is not None:
                    dt_ns += lag_ns[q]
                dist_m = dt_ns / 1e9 * self.SPEED_OF_LIGHT
                p1, p2 = buoy_positions.get(d1.buoy_id), buoy_positions.get(d2.buoy_id)
                if not p1 or not p2:
                    continue
                conf = min(d1.confidence, d2.confidence) * self._timing_confidence(p1, p2)
                if qual is not None:
                    if self.min_psr is not None and not float(qual[q][1]) >= self.min_psr:   # (RMX_Q_PSR)
                        self.logger.warning("TDoA %s-%s dropped: peak-to-floor ratio %.1f below min_psr %.1f", d1.buoy_id,
                                            d2.buoy_id, float(qual[q][1]), self.min_psr)
                        continue
                    if self.correlation_confidence:
                        conf *= float(qual[q][0])   # (RMX_Q_COHERENCE)
                if dop_hz is not None:
                    out.append(TDoAMeasurement(d1.buoy_id, d2.buoy_id, dt_ns, dist_m, conf, d1.frequency_mhz, float(dop_hz[q])))
                else:
                    out.append(TDoAMeasurement(d1.buoy_id, d2.buoy_id, dt_ns, dist_m, conf, d1.frequency_mhz))
                if debug:
                    self.logger.debug("TDoA %s-%s dT=%.1f us dD=%.1f m", d1.buoy_id, d2.buoy_id, dt_ns / 1000, dist_m)
        return out


# --------------------------------------------------------------------------------------------------
# consumer: hyperbolic fix (unchanged semantics; tdoa_processor.py:218-328)
# --------------------------------------------------------------------------------------------------
class HyperbolicPositioning:
    def __init__(self):
        self.logger = logging.getLogger(__name__ + ".HyperbolicPositioning")

    def triangulate_position(self, measurements: List[TDoAMeasurement],
                             buoy_positions: Dict[str, BuoyPosition]) -> Optional[TriangulationResult]:
        if len(measurements) < 2:
            self.logger.warning("Need at least 2 TDoA measurements for triangulation")
            return None
        ids = set()
        for m in measurements:
            ids.update((m.buoy1_id, m.buoy2_id))
        if len(ids) < 3:
            self.logger.warning("Need at least 3 buoys for 2D triangulation")
            return None
        xyz = {}
        for b in ids:
            if b not in buoy_positions:
                self.logger.error(f"Missing position for buoy {b}")
                return None
            pos = buoy_positions[b]
            xyz[b] = GeodeticCalculator.lat_lng_to_xyz(pos.lat, pos.lng, pos.altitude)
        # the objective in the reference's own scalar arithmetic (math.sqrt, one division per term,
        # left-to-right sum: tdoa_processor.py:249-273): BFGS with finite-difference gradients stops on
        # "precision loss" or not depending on the last bits of this function, so a vectorised sum
        # (different rounding order) changes which calls return None
        terms = [(xyz[m.buoy1_id], xyz[m.buoy2_id], m.distance_difference_m, m.confidence + 0.1)
                 for m in measurements]

        def cost(tx):
            x, y, z = tx
            total = 0
            for a, b, meas_m, den in terms:
                d1 = math.sqrt((x - a[0]) ** 2 + (y - a[1]) ** 2 + (z - a[2]) ** 2)
                d2 = math.sqrt((x - b[0]) ** 2 + (y - b[1]) ** 2 + (z - b[2]) ** 2)
                total = total + ((d2 - d1) - meas_m) ** 2 / den
            return total

        pts = list(xyz.values())
        x0 = [sum(q[k] for q in pts) / len(pts) for k in range(3)]
        try:
            import scipy.optimize
            res = scipy.optimize.minimize(cost, x0, method="BFGS", options={"maxiter": 1000})
            if not res.success:
                self.logger.warning(f"Optimization failed: {res.message}")
                return None
            lat, lng, alt = GeodeticCalculator.xyz_to_lat_lng(*res.x)
            acc = math.sqrt(res.fun / len(measurements))
            conf = sum(m.confidence for m in measurements) / len(measurements)
            self.logger.info(f"Triangulation successful: ({lat:.6f}, {lng:.6f}) ±{acc:.1f}m, confidence: {conf:.2f}")
            return TriangulationResult(lat, lng, alt, acc, conf, measurements[0].frequency_mhz, "unknown",
                                       datetime.now(timezone.utc).isoformat(), list(ids), measurements,
                                       "hyperbolic")
        except Exception as e:  # reference convention: log, never raise (:326-328)
            self.logger.error(f"Triangulation failed: {e}")
            return None


    def triangulate_batch(self, engine, buoys: List[BuoyPosition], lag_int, lag_frac, sample_rate_hz: float,
                          confidence=None, max_iter: int = 60, lag_sigma=None, sigma_floor=None, altitude_m=None):
        """Batched form of triangulate_position on the GPU (rmx_solve_batch): one solve per window
        from the lag arrays XcorrEngine.correlate returned for `buoys` (detection-list order, all
        pairs i<j).  Same objective, start point and accuracy formula as the reference
        (tdoa_processor.py:249-300).  confidence: None (every measurement counts 1), [W][P] as the lag arrays, or
        1-D of length P = one confidence row for all windows (XcorrEngine.solve broadcasts the weight row to [W][P]);
        any other shape is a ValueError.  Returns a list of (lat, lng, altitude, accuracy_meters).

        lag_sigma, sigma_floor, altitude_m: with none of them given the call is the one above.  With any of them the
        solve is XcorrEngine.solve_fix (rmx_solve_batch_fix) and every tuple gains a fifth element (below).
        lag_sigma (samples, [W][P] or [P], xcorr.lag_sigma of the lags' quality) with sigma_floor (samples, the stations'
        clock-sync uncertainty, > 0) weights every pair by xcorr.lag_weight = 1 / sigma_d^2 instead of by confidence: the
        two go together, and lag_sigma with confidence is a ValueError.
        altitude_m holds the fix to the tangent plane at the fleet's centroid, lifted to that altitude
        (GeodeticCalculator.tangent_plane): two unknowns, for stations that float on one surface, whose lags do not
        observe altitude.
        The fifth element is a dict: ellipse_m = (semi-major, semi-minor in metres at 95 %, azimuth of the major axis in
        degrees from north through east, in [0, 180)), or None with three unknowns; drms_m = sqrt of the trace of the
        horizontal 2 x 2 covariance (with three unknowns: the east/north block of cov at the fix); chi2 = the cost, a
        chi-square where the weights are 1 / sigma_d^2; dof = the pairs of weight > 0 less the unknowns.
        accuracy_meters is then drms_m (inf where the information is singular), not sqrt(cost / P)."""
        xyz = np.array([GeodeticCalculator.lat_lng_to_xyz(b.lat, b.lng, b.altitude) for b in buoys])
        if lag_sigma is None and sigma_floor is None and altitude_m is None:
            weight = None if confidence is None else 1.0 / (np.asarray(confidence, np.float64) + 0.1)
            pos, cost, _ = engine.solve(xyz, lag_int, lag_frac, sample_rate_hz, weight=weight, max_iter=max_iter)
            n_meas = np.asarray(lag_int).shape[1]
            return [GeodeticCalculator.xyz_to_lat_lng(*p) + (math.sqrt(max(c, 0.0) / n_meas),)
                    for p, c in zip(pos, cost)]
        from .xcorr import error_ellipse, lag_weight
        if (lag_sigma is None) != (sigma_floor is None):
            raise ValueError("lag_sigma and sigma_floor go together: give both or neither")
        if lag_sigma is not None and confidence is not None:
            raise ValueError("lag_sigma and confidence both weight the pairs: give one of them")
        if lag_sigma is not None:
            weight = lag_weight(lag_sigma, sample_rate_hz, sigma_floor)
        else:
            weight = None if confidence is None else 1.0 / (np.asarray(confidence, np.float64) + 0.1)
        plane = None
        if altitude_m is not None:
            c = xyz.mean(axis=0)
            lat0, lng0, _ = GeodeticCalculator.xyz_to_lat_lng(*c)
            plane = np.array(GeodeticCalculator.tangent_plane(lat0, lng0, float(altitude_m))).reshape(-1)
        fix = engine.solve_fix(xyz, lag_int, lag_frac, sample_rate_hz, weight=weight, max_iter=max_iter, plane=plane)
        W, P = np.asarray(lag_int).shape
        n_unknowns = 3 if plane is None else 2
        if weight is None:
            used = np.full(W, P)
        else:
            used = np.count_nonzero(np.broadcast_to(np.asarray(weight, np.float32), (W, P)) > 0, axis=1)
        out = []
        for w in range(W):
            lat, lng, alt = GeodeticCalculator.xyz_to_lat_lng(*fix.pos[w])
            if plane is not None:
                c2 = fix.cov[w]
                major, minor, ang = error_ellipse(c2)
                ellipse = (float(major), float(minor), (90.0 - math.degrees(float(ang))) % 180.0)
            else:
                xx, xy, xz, yy, yz, zz = fix.cov[w]
                if math.isfinite(xx) and math.isfinite(yy) and math.isfinite(zz):
                    _, e, n = GeodeticCalculator.tangent_plane(lat, lng)
                    full = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
                    en = np.array([e, n])
                    h = en @ full @ en.T
                    c2 = (h[0, 0], h[0, 1], h[1, 1])
                else:
                    c2 = (math.inf, 0.0, math.inf)
                ellipse = None
            drms = math.sqrt(c2[0] + c2[2])
            out.append((lat, lng, alt, drms, dict(ellipse_m=ellipse, drms_m=drms, chi2=float(fix.cost[w]),
                                                  dof=int(used[w]) - n_unknowns)))
        return out


# --------------------------------------------------------------------------------------------------
# orchestrator (tdoa_processor.py:330-465)
# --------------------------------------------------------------------------------------------------
class TDoAProcessor:
    def __init__(self, band_limit: bool = False, whiten: bool = False, integrate: int = 1, refine: int = 0,
                 min_psr: Optional[float] = None, correlation_confidence: bool = False,
                 doppler_search_hz: Optional[Tuple[float, float]] = None, share_captures: bool = False,
                 share_qualified: bool = False, share_integrated: bool = False, share_doppler: bool = False):
        """band_limit, whiten, integrate, refine, min_psr, correlation_confidence, doppler_search_hz, share_captures,
        share_qualified, share_integrated, share_doppler: the TDoACalculator settings of the same names (off by default)."""
        self.logger = logging.getLogger(__name__ + ".TDoAProcessor")
        self.tdoa_calculator = TDoACalculator(band_limit=band_limit, whiten=whiten, integrate=integrate, refine=refine,
                                              min_psr=min_psr, correlation_confidence=correlation_confidence,
                                              doppler_search_hz=doppler_search_hz, share_captures=share_captures,
                                              share_qualified=share_qualified, share_integrated=share_integrated,
                                              share_doppler=share_doppler)
        self.hyperbolic_positioner = HyperbolicPositioning()
        self.buoy_positions: Dict[str, BuoyPosition] = {}
        self.correlation_window_s = 10.0
        self.min_buoys_for_triangulation = 3

    def register_buoy(self, buoy_position: BuoyPosition):
        self.buoy_positions[buoy_position.buoy_id] = buoy_position
        self.logger.info(f"Registered buoy {buoy_position.buoy_id} at "
                         f"({buoy_position.lat:.6f}, {buoy_position.lng:.6f})")

    def _group_by_frequency(self, detections: Sequence[SignalDetection],
                            frequency_tolerance_mhz: float = 0.01) -> Dict[float, List[SignalDetection]]:
        """First-fit grouping on the group's first frequency (tdoa_processor.py:405-425)."""
        groups: Dict[float, List[SignalDetection]] = {}
        for d in detections:
            key = next((f for f in groups if abs(d.frequency_mhz - f) <= frequency_tolerance_mhz), None)
            if key is None:
                groups[d.frequency_mhz] = [d]
            else:
                groups[key].append(d)
        return groups

    def _filter_by_time_window(self, detections: Sequence[SignalDetection]) -> List[SignalDetection]:
        """Keep detections no older than correlation_window_s before the newest, sorted by time
        (tdoa_processor.py:427-445)."""
        if not detections:
            return []
        ordered = sorted(detections, key=lambda d: d.gps_timestamp_ns)
        cutoff = ordered[-1].gps_timestamp_ns - int(self.correlation_window_s * 1e9)
        return [d for d in ordered if d.gps_timestamp_ns >= cutoff]

    def process_signal_detections(self, detections: List[SignalDetection]) -> List[TriangulationResult]:
        if not detections:
            return []
        self.logger.info(f"Processing {len(detections)} signal detections")
        # frequency groups are independent units (tdoa_processor.py:363-377): all groups whose
        # detections carry IQ windows of one shape go to the GPU as ONE [groups][B][N] batch
        work = []
        for freq, group in self._group_by_frequency(detections).items():
            recent = self._filter_by_time_window(group)
            if len(recent) < self.min_buoys_for_triangulation:
                self.logger.debug(f"Insufficient detections for {freq} MHz ({len(recent)} < "
                                  f"{self.min_buoys_for_triangulation})")
                continue
            key, stacked = self.tdoa_calculator._iq_batch_key(recent)   # inspected (and logged) once per group
            work.append([freq, recent, key, stacked, TDoACalculator._TIME_TAGS if key is None else None])
        batches: Dict[Any, List[int]] = {}
        for n, item in enumerate(work):
            if item[2]:
                batches.setdefault(item[2], []).append(n)
        calc = self.tdoa_calculator
        for key, members in batches.items():
            n_samp = work[members[0]][3].shape[-1] // (2 if work[members[0]][3].dtype == np.uint8 else 1)
            if calc.integrate != 1:   # the engine sees segments of n_samp // K samples; a batch shares one window length
                n_samp, why = calc.segment_length(n_samp)
                if why:
                    for n in members:
                        calc.logger.error(f"Cannot integrate the group at {work[n][0]} MHz: {why}; no TDoA measurements for it")
                        work[n][4] = None
                    continue
            band = None
            if calc.band_limit:   # one band per group: [G][2]; a group that cannot be band limited gets no measurements
                bands = {}
                for n in list(members):
                    b, why = calc.band(work[n][1], n_samp, key[3])
                    if why:
                        calc.logger.error(f"Cannot band limit the group at {work[n][0]} MHz: {why}; no TDoA measurements for it")
                        work[n][4] = None
                        members.remove(n)
                    else:
                        bands[n] = b
                if not members:
                    continue
                # (refine, min_psr / correlation_confidence: only with share_qualified; integrate: only with share_integrated;
                # the Doppler search only with share_doppler -- it has none of the three)
                if calc.share_captures and (calc.integrate == 1 or calc.share_integrated) \
                        and (calc.doppler_search_hz is None or calc.share_doppler) \
                        and (calc.share_qualified or (calc.refine == 0 and not calc._wants_quality())):
                    members = self._measure_shared_captures(work, members, bands, n_samp, key[3])
                    if not members:
                        continue
                if any(bands[n] is not None for n in members):
                    band = np.stack([np.array([-0.5, 0.5]) if bands[n] is None else bands[n] for n in members])
            stacked = np.stack([work[n][3] for n in members])
            # (min_psr / correlation_confidence: the quality figures ride along as the tuple's fourth entry)
            more = {"with_quality": True} if calc._wants_quality() else {}
            if calc.doppler_search_hz is not None:   # (lag, offset in hertz) per group; the offsets ride as the fifth entry
                per = [calc.lag_bounds(work[n][1], self.buoy_positions, n_samp, key[3]) for n in members] if calc.bound_lags else None
                res = calc._measure_groups(stacked, None if per is None else np.stack([b for b, _ in per]), band, fs=key[3])
                for k, n in enumerate(members):
                    work[n][4] = None if res is None else (res[0][k], key[3], None if per is None else per[k][1], None, res[1][k])
                continue
            if calc.bound_lags:   # per-window bounds [G][P][2]: each group has its own buoys and window starts
                per = [calc.lag_bounds(work[n][1], self.buoy_positions, n_samp, key[3]) for n in members]
                lags = calc._measure_groups(stacked, np.stack([b for b, _ in per]), band, **more)
                qual = None
                if more and lags is not None:
                    lags, qual = lags
                for k, n in enumerate(members):
                    work[n][4] = None if lags is None else ((lags[k], key[3], per[k][1]) + (() if qual is None else (qual[k],)))
                continue
            lags = calc._measure_groups(stacked, None, band, **more)
            qual = None
            if more and lags is not None:
                lags, qual = lags
            for k, n in enumerate(members):
                work[n][4] = None if lags is None else ((lags[k], key[3]) + (() if qual is None else (None, qual[k])))
        results: List[TriangulationResult] = []
        for freq, recent, key, _, lag in work:
            meas = self.tdoa_calculator.calculate_tdoa_measurements(recent, self.buoy_positions, _lag=lag)
            if len(meas) < 2:
                self.logger.debug(f"Insufficient TDoA measurements for {freq} MHz")
                continue
            fix = self.hyperbolic_positioner.triangulate_position(meas, self.buoy_positions)
            if fix:
                kinds = [d.signal_type for d in recent]
                fix.signal_type = max(set(kinds), key=kinds.count)
                results.append(fix)
                if fix.signal_type == "emergency":
                    self.logger.warning(f"EMERGENCY SIGNAL TRIANGULATED: {freq} MHz at "
                                        f"({fix.estimated_lat:.6f}, {fix.estimated_lng:.6f}) "
                                        f"±{fix.accuracy_meters:.1f}m")
        return results

    def _measure_shared_captures(self, work, members, bands, n_samp: int, fs: float):
        """share_captures: the members of one batch whose stacked windows are byte-identical to another member's -- frequency
        groups cut from ONE capture -- and whose lag bounds (bound_lags) are identical too are correlated as one window under
        several bands (TDoACalculator._measure_shared); their work items get their lags as the separate calls would have
        set them.  A row with fewer bands than the widest is padded by repeating its last band, and the padded outputs
        are dropped.  share_qualified: the quality figures of every (capture, band) ride along as the work item's fourth
        entry, as _measure_groups' do.  share_doppler: one Doppler search under the bands; every member's work item is the
        search's own (lag, fs, window starts, None, offsets in hertz).  Returns the members that are left for the usual call."""
        calc = self.tdoa_calculator
        per = {n: calc.lag_bounds(work[n][1], self.buoy_positions, n_samp, fs) for n in members} if calc.bound_lags else {}
        rows: Dict[Any, List[int]] = {}
        for n in members:
            sig = (work[n][3].tobytes(),) + ((per[n][0].tobytes(), per[n][1].tobytes()) if per else ())
            rows.setdefault(sig, []).append(n)
        shared = [r for r in rows.values() if len(r) > 1]
        if not shared:
            return members
        full = np.array([-0.5, 0.5])
        width = max(len(r) for r in shared)
        band_set = np.stack([np.stack([full if bands[n] is None else bands[n] for n in r + [r[-1]] * (width - len(r))])
                             for r in shared])
        stacked = np.stack([work[r[0]][3] for r in shared])
        more = {"with_quality": True} if calc._wants_quality() else {}
        doppler = calc.doppler_search_hz is not None
        if doppler:
            more = {"fs": fs}
        lags = calc._measure_shared(stacked, np.stack([per[r[0]][0] for r in shared]) if per else None, band_set, **more)
        qual = dop = None
        if doppler and lags is not None:
            lags, dop = lags
        elif more and lags is not None:
            lags, qual = lags
        for g, r in enumerate(shared):
            for m, n in enumerate(r):
                if lags is None:
                    work[n][4] = None
                elif doppler:
                    work[n][4] = (lags[g, m], fs, per[n][1] if per else None, None, dop[g, m])
                elif qual is None:
                    work[n][4] = (lags[g, m], fs) + ((per[n][1],) if per else ())
                else:
                    work[n][4] = (lags[g, m], fs, per[n][1] if per else None, qual[g, m])
        taken = {n for r in shared for n in r}
        return [n for n in members if n not in taken]

    def triangulate_signal(self, detections: List[SignalDetection]) -> Optional[TriangulationResult]:
        """What central_processor.py:418 calls (missing in the reference): first fix or None."""
        res = self.process_signal_detections(detections)
        return res[0] if res else None

    def get_buoy_network_status(self) -> Dict:
        return {
            "registered_buoys": len(self.buoy_positions),
            "buoy_list": [{"buoy_id": p.buoy_id, "lat": p.lat, "lng": p.lng,
                           "timing_accuracy_ns": p.timing_accuracy_ns}
                          for p in self.buoy_positions.values()],
            "min_buoys_required": self.min_buoys_for_triangulation,
            "correlation_window_s": self.correlation_window_s,
            "triangulation_ready": len(self.buoy_positions) >= self.min_buoys_for_triangulation,
        }
