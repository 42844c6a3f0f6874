"""Multi-device dispatch INSIDE the package: one `rmx_ctx` + one host thread per device, capture windows
block-sharded over them, host-side gather of the 12-byte-per-pair-window results.

The path shards by window (tdoa_processor.py:363 loops the frequency groups independently,
no state crosses windows), so there is no collective: the caller -- the server's single asyncio thread,
central_processor.py:335 -> 397 -> 418 -- hands over one `[W][B][N]` batch, every device gets a contiguous block
of windows (`shard.window_shard`), and the lags come back concatenated in window order.  ctypes releases the GIL
for the duration of `rmx_xcorr_batch`, so plain threads drive the devices concurrently (no torchrun, no process
group); `bench.py --gpus N` remains the one-process-per-GPU harness the driver measures.

An engine is single-owner (include/rmx.h): each `XcorrEngine` here is only ever touched by its own worker thread.
Measured on one MI355X only (devices=[0] and the same-device rehearsal devices=[0, 0]): the scaling beyond one GPU
is unmeasured.
"""
from __future__ import annotations

import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from .shard import window_shard
from .xcorr import LagRequest, check_refine, lag_request


def _more(req: LagRequest, name_refine: bool) -> dict:
    """The keywords a block's call names beyond its arrays: an option at its default is left out, so that an engine that
    does not know it still serves (name_refine: refine = 0 is named all the same)."""
    more = {"refine": req.U} if req.U or name_refine else {}
    if req.quality:
        more["quality"] = True
    if req.K > 1:
        more["integrate"] = req.K
    return more


class MultiXcorrEngine:
    """`XcorrEngine.correlate` / `.correlate_bands` / `.caf` / `.caf_bands` over several devices.

    devices=None -> every visible device (`rmx_device_count`).  A device may be listed more than once (two
    contexts on one GPU: the rehearsal mode of the tests).  `engine_factory(n_buoys, n_samples, max_windows,
    device)` exists for the CPU tests of the split / gather logic (a stub engine); the default builds the HIP
    engine and raises, as `XcorrEngine` does, when the library or a GPU is missing.
    """

    def __init__(self, n_buoys: int, n_samples: int, max_windows: int, devices: Optional[Sequence[int]] = None,
                 engine_factory: Optional[Callable] = None):
        if engine_factory is None:
            from . import xcorr

            def engine_factory(b, n, w, device):
                return xcorr.XcorrEngine(b, n, w, device=device)

            if devices is None:
                devices = list(range(xcorr.device_count()))
                if not devices:
                    raise xcorr.RmxError(-2, "no device visible")
        elif devices is None:
            raise ValueError("devices must be given with an engine_factory")
        self.devices = [int(d) for d in devices]
        if not self.devices:
            raise ValueError("devices is empty")
        self.n_buoys, self.n_samples, self.max_windows = n_buoys, n_samples, max_windows
        g = len(self.devices)
        # every worker gets the largest block a batch of max_windows can hand it (rank 0's)
        per_dev = max(window_shard(max_windows, 0, g)[1], 1)
        self._engines = []
        try:
            for d in self.devices:
                self._engines.append(engine_factory(n_buoys, n_samples, per_dev, d))
        except Exception:
            self.close()
            raise
        # one thread per engine, and work item r always runs on thread r's engine: an engine never changes hands
        self._pools = [ThreadPoolExecutor(max_workers=1, thread_name_prefix=f"rmx-dev{d}-{r}")
                       for r, d in enumerate(self.devices)]
        self._lock = threading.Lock()            # one batch at a time (the engines are stateful)

    # -- plumbing ------------------------------------------------------------------------------------
    def close(self):
        for p in getattr(self, "_pools", []):
            p.shutdown(wait=True)
        self._pools = []
        for e in getattr(self, "_engines", []):
            try:
                e.close()
            except Exception:
                pass
        self._engines = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def blocks(self, n_windows: int) -> List[Tuple[int, int]]:
        """(start, count) of every device's block, in device order (empty blocks included)."""
        return [window_shard(n_windows, r, len(self.devices)) for r in range(len(self.devices))]

    def _n_pairs(self, pairs) -> int:
        return self.n_buoys * (self.n_buoys - 1) // 2 if pairs is None else np.asarray(pairs).reshape(-1, 2).shape[0]

    def _shard(self, req: LagRequest, iq: np.ndarray, call: Callable):
        """The one sharding routine.  The request's rows -- the windows, or whole groups of K -- are block-sharded over the
        devices; every block walks steps of whole groups that its engine holds and makes call(eng, the step's windows, its
        lag bounds, its band(s)) (LagRequest.cut); the parts are gathered into outputs of the request's shapes and dtypes."""
        if req.n_windows > self.max_windows:
            raise ValueError(f"n_windows {req.n_windows} > max_windows {self.max_windows}")
        K = req.K
        outs = [np.zeros(shape, dt) for _, dt, shape in req.outputs()]

        def block(eng, gs, gc):
            # the engines are sized for an even split of the WINDOWS; a block of whole groups may be a little larger
            step = gc if K == 1 else getattr(eng, "max_windows", gc * K) // K
            if step < 1:
                raise ValueError(f"integrate = {K} windows per group is more than one device's engine holds "
                                 f"({eng.max_windows} windows)")
            parts = [call(eng, iq[g0 * K:g1 * K], *req.cut(g0, g1))
                     for g0, g1 in ((g, min(g + step, gs + gc)) for g in range(gs, gs + gc, step))]
            return parts[0] if len(parts) == 1 else [np.concatenate([p[k] for p in parts]) for k in range(len(outs))]
        with self._lock:
            futs = []
            for r, (s, c) in enumerate(self.blocks(req.rows)):
                if c:
                    futs.append((s, c, self._pools[r].submit(block, self._engines[r], s, c)))
            err = None
            for s, c, f in futs:                 # wait for ALL workers before raising: no engine is left mid-call
                try:
                    res = f.result()
                    for k, out in enumerate(outs):
                        out[s:s + c] = res[k]
                except Exception as e:           # noqa: BLE001  (re-raised below)
                    err = err or e
            if err is not None:
                raise err
        return tuple(outs)

    # -- the hot path --------------------------------------------------------------------------------
    def correlate(self, iq: np.ndarray, pairs: Optional[np.ndarray] = None, lag_bounds=None, band=None,
                  whiten: bool = False, integrate: int = 1, refine: int = 0, quality: bool = False):
        """iq: complex64 [W][B][N] or uint8 [W][B][2N] -> (lag_int [W][P], lag_frac [W][P], peak [W][P]).
        lag_bounds: None, [P][2] (every block gets it whole) or [W][P][2] (each block gets its own windows' rows).
        band: None, [2] (every block gets it whole) or [W][2] (each block its own windows' rows); whiten: PHAT.
        integrate: K windows per group (XcorrEngine.correlate): whole groups are sharded over the devices, the results and
        per-group lag_bounds are [W // K][.]; a block larger than its engine holds runs as several calls of whole groups.
        refine: U of the fine lag search (XcorrEngine.correlate), handed to every block's call.
        quality: True gathers a fourth array, the blocks' quality figures [W // K][P][4] (XcorrEngine.correlate)."""
        iq = np.asarray(iq)
        if iq.ndim != 3:
            raise ValueError(f"iq must be [W][B][N], got shape {iq.shape}")
        req = lag_request("xcorr", self.n_buoys, iq.shape[0], None, lag_bounds, band, whiten, integrate, refine, quality,
                          n_pairs=self._n_pairs(pairs))
        more = _more(req, req.quality and req.K == 1)   # (a quality call names refine = 0 too, but not under integration)

        def call(eng, x, lb, bd):
            if more or bd is not None or whiten:
                return eng.correlate(x, pairs, lb, band=bd, whiten=whiten, **more)
            return eng.correlate(x, pairs) if lb is None else eng.correlate(x, pairs, lb)
        return self._shard(req, iq, call)

    def correlate_bands(self, iq: np.ndarray, bands, pairs: Optional[np.ndarray] = None, lag_bounds=None,
                        whiten: bool = False, refine: int = 0, quality: bool = False, integrate: int = 1):
        """XcorrEngine.correlate_bands over the devices -> three [W][M][P] arrays.  The windows are sharded as correlate()
        shards them: bands [M][2] and lag_bounds [P][2] go to every block whole, [W][M][2] and [W][P][2] are cut into each
        block's own windows' rows.  refine and quality are handed to every block's call (quality: a fourth array,
        [W][M][P][4]); with neither, every block makes exactly the call it made without them.
        integrate: K windows per group (XcorrEngine.correlate_bands): whole groups are sharded over the devices, as
        correlate() shards them; the results and per-group lag_bounds are [W // K][.], the bands stay per window."""
        iq = np.asarray(iq)
        if iq.ndim != 3:
            raise ValueError(f"iq must be [W][B][N], got shape {iq.shape}")
        # (the bands and the bounds are checked in front of refine here)
        req = lag_request("bands", self.n_buoys, iq.shape[0], None, lag_bounds, bands, whiten, integrate, 0, quality,
                          n_pairs=self._n_pairs(pairs))._replace(U=check_refine(refine))
        more = _more(req, req.quality)
        return self._shard(req, iq, lambda eng, x, lb, bd: eng.correlate_bands(x, bd, pairs, lag_bounds=lb, whiten=whiten, **more))

    def caf(self, iq: np.ndarray, doppler_cps, pairs: Optional[np.ndarray] = None, lag_bounds=None, band=None,
            whiten: bool = False, fine: bool = False, refine: int = 0, quality: bool = False, integrate=None):
        """Cross-ambiguity search -> (doppler_idx, lag_int, lag_frac, peak), each [W][P]; with fine=True (doppler_idx,
        dop_frac, lag_int, lag_frac, peak) (XcorrEngine.caf).  lag_bounds [P][2] and band [2] go to every block whole,
        [W][P][2] and [W][2] are cut into each block's own windows' rows, as correlate() cuts them.  refine and quality
        are handed to every block's call (quality: the blocks' figures [W][P][4] as the last array); with neither, every
        block makes exactly the call it made without them.
        integrate: K windows per group (XcorrEngine.caf): whole groups are sharded over the devices, as correlate() shards
        them; the results and per-group lag_bounds are [W // K][.], the band stays per window."""
        iq = np.asarray(iq)
        if iq.ndim != 3:
            raise ValueError(f"iq must be [W][B][N], got shape {iq.shape}")
        # (the engines see the caller's own grid and check it themselves, as they do the pairs)
        req = lag_request("caf", self.n_buoys, iq.shape[0], None, lag_bounds, band, whiten, integrate, refine, quality, (), fine,
                          n_pairs=self._n_pairs(pairs))
        more = _more(req, req.quality)

        def call(eng, x, lb, bd):
            if more or lb is not None or bd is not None or whiten or fine:
                return eng.caf(x, doppler_cps, pairs, lag_bounds=lb, band=bd, whiten=whiten, fine=fine, **more)
            return eng.caf(x, doppler_cps, pairs)
        return self._shard(req, iq, call)

    def caf_bands(self, iq: np.ndarray, doppler_cps, bands, pairs: Optional[np.ndarray] = None, lag_bounds=None,
                  whiten: bool = False, fine: bool = False):
        """XcorrEngine.caf_bands over the devices -> (doppler_idx, lag_int, lag_frac, peak), each [W][M][P]; with fine=True
        (doppler_idx, dop_frac, lag_int, lag_frac, peak).  The windows are sharded as caf() shards them: bands [M][2] and
        lag_bounds [P][2] go to every block whole, [W][M][2] and [W][P][2] are cut into each block's own windows' rows; the
        grid goes to every block whole."""
        iq = np.asarray(iq)
        if iq.ndim != 3:
            raise ValueError(f"iq must be [W][B][N], got shape {iq.shape}")
        # (the engines see the caller's own grid and check it themselves, as they do the pairs)
        req = lag_request("caf_bands", self.n_buoys, iq.shape[0], None, lag_bounds, bands, whiten, doppler_cps=(), fine=fine,
                          n_pairs=self._n_pairs(pairs))
        return self._shard(req, iq, lambda eng, x, lb, bd: eng.caf_bands(x, doppler_cps, bd, pairs, lag_bounds=lb, whiten=whiten,
                                                                          fine=fine))
