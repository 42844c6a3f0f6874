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
from .xcorr import check_band, check_bands, check_integrate, check_lag_bounds, check_refine


class MultiXcorrEngine:
    """`XcorrEngine.correlate` / `.caf` over several devices.

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

    def _run(self, n_windows: int, call: Callable, n_out: int, dtypes, n_pairs: int, n_rows: Optional[int] = None,
             tails=None):
        """n_rows: the items that are sharded and the rows of the results (the groups of an integrated call); default: the
        windows.  tails: per output, the trailing shape behind [rows][P] (the 4 of the quality array); default: none"""
        if n_windows > self.max_windows:
            raise ValueError(f"n_windows {n_windows} > max_windows {self.max_windows}")
        n_windows = n_windows if n_rows is None else n_rows
        tails = tails or [()] * len(dtypes)
        outs = [np.zeros((n_windows, n_pairs) + tuple(t), dt) for dt, t in zip(dtypes, tails)]
        with self._lock:
            futs = []
            for r, (s, c) in enumerate(self.blocks(n_windows)):
                if c:
                    futs.append((s, c, self._pools[r].submit(call, self._engines[r], s, c)))
            err = None
            for s, c, f in futs:                 # wait for ALL workers before raising: no engine is left mid-call
                try:
                    res = f.result()
                    for k in range(n_out):
                        outs[k][s:s + c] = res[k]
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
        P = self.n_buoys * (self.n_buoys - 1) // 2 if pairs is None else np.asarray(pairs).reshape(-1, 2).shape[0]
        K = check_integrate(integrate, iq.shape[0])
        U = check_refine(refine)
        n_out = 4 if quality else 3
        dtypes = (np.int32, np.float32, np.float32, np.float32)[:n_out]
        tails = [(), (), (), (4,)][:n_out]
        if K > 1:
            return self._correlate_integrated(iq, pairs, lag_bounds, band, whiten, K, P, U, bool(quality))
        lb, per_window = check_lag_bounds(lag_bounds, iq.shape[0], P)

        bd, band_pw = check_band(band, iq.shape[0])

        def block_bounds(s, c):
            return lb[s:s + c] if per_window else lb

        def block_call(eng, s, c):
            if quality:
                return eng.correlate(iq[s:s + c], pairs, None if lb is None else block_bounds(s, c),
                                     band=None if bd is None else (bd[s:s + c] if band_pw else bd), whiten=whiten, refine=U,
                                     quality=True)
            if U > 0:
                return eng.correlate(iq[s:s + c], pairs, None if lb is None else block_bounds(s, c),
                                     band=None if bd is None else (bd[s:s + c] if band_pw else bd), whiten=whiten, refine=U)
            if bd is not None or whiten:
                return eng.correlate(iq[s:s + c], pairs, None if lb is None else block_bounds(s, c),
                                     band=None if bd is None else (bd[s:s + c] if band_pw else bd), whiten=whiten)
            if lb is not None:
                return eng.correlate(iq[s:s + c], pairs, block_bounds(s, c))
            return eng.correlate(iq[s:s + c], pairs)
        return self._run(iq.shape[0], block_call, n_out, dtypes, P, tails=tails)

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
        W = iq.shape[0]
        P = self.n_buoys * (self.n_buoys - 1) // 2 if pairs is None else np.asarray(pairs).reshape(-1, 2).shape[0]
        K = check_integrate(integrate, W)
        bd, bands_pw = check_bands(bands, W)
        lb, per_window = check_lag_bounds(lag_bounds, W // K, P)
        U = check_refine(refine)
        more = {"refine": U, "quality": True} if quality else ({"refine": U} if U else {})
        n_out = 4 if quality else 3
        if K > 1:
            def group_call(eng, gs, gc):
                # (as _correlate_integrated: a block of whole groups may be a little larger than its engine)
                step = getattr(eng, "max_windows", gc * K) // K
                if step < 1:
                    raise ValueError(f"integrate = {K} windows per group is more than one device's engine holds "
                                     f"({eng.max_windows} windows)")
                parts = []
                for g0 in range(gs, gs + gc, step):
                    g1 = min(g0 + step, gs + gc)
                    parts.append(eng.correlate_bands(iq[g0 * K:g1 * K], bd[g0 * K:g1 * K] if bands_pw else bd, pairs,
                                                     lag_bounds=None if lb is None else (lb[g0:g1] if per_window else lb),
                                                     whiten=whiten, integrate=K, **more))
                return tuple(np.concatenate([p[k] for p in parts]) for k in range(n_out))
            return self._run(W, group_call, n_out, (np.int32, np.float32, np.float32, np.float32)[:n_out], bd.shape[-2],
                             n_rows=W // K, tails=[(P,), (P,), (P,), (P, 4)][:n_out])

        def block_call(eng, s, c):
            return eng.correlate_bands(iq[s:s + c], bd[s:s + c] if bands_pw else bd, pairs,
                                       lag_bounds=None if lb is None else (lb[s:s + c] if per_window else lb), whiten=whiten, **more)
        # (_run's rows are [W][n_pairs] + tail: here [W][M] + (P,))
        return self._run(W, block_call, n_out, (np.int32, np.float32, np.float32, np.float32)[:n_out], bd.shape[-2],
                         tails=[(P,), (P,), (P,), (P, 4)][:n_out])

    def _correlate_integrated(self, iq, pairs, lag_bounds, band, whiten, K, P, U=0, quality=False):
        W = iq.shape[0]
        G = W // K
        lb, per_group = check_lag_bounds(lag_bounds, G, P)
        bd, band_pw = check_band(band, W)

        kw = {"refine": U} if U > 0 else {}
        if quality:
            kw["quality"] = True
        n_out = 4 if quality else 3

        def block_call(eng, gs, gc):
            # the engines are sized for an even split of the WINDOWS; a block of whole groups may be a little larger
            step = getattr(eng, "max_windows", gc * K) // K
            if step < 1:
                raise ValueError(f"integrate = {K} windows per group is more than one device's engine holds "
                                 f"({eng.max_windows} windows)")
            parts = []
            for g0 in range(gs, gs + gc, step):
                g1 = min(g0 + step, gs + gc)
                parts.append(eng.correlate(iq[g0 * K:g1 * K], pairs,
                                           None if lb is None else (lb[g0:g1] if per_group else lb),
                                           band=None if bd is None else (bd[g0 * K:g1 * K] if band_pw else bd),
                                           whiten=whiten, integrate=K, **kw))
            return tuple(np.concatenate([p[k] for p in parts]) for k in range(n_out))
        return self._run(W, block_call, n_out, (np.int32, np.float32, np.float32, np.float32)[:n_out], P, n_rows=G,
                         tails=[(), (), (), (4,)][:n_out])

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
        P = self.n_buoys * (self.n_buoys - 1) // 2 if pairs is None else np.asarray(pairs).reshape(-1, 2).shape[0]
        K = 1 if integrate is None else check_integrate(integrate, iq.shape[0])
        U = check_refine(refine)
        more = {"refine": U, "quality": True} if quality else ({"refine": U} if U else {})
        if K > 1:
            return self._caf_integrated(iq, doppler_cps, pairs, lag_bounds, band, whiten, fine, more, K, P)
        lb, per_window = check_lag_bounds(lag_bounds, iq.shape[0], P)
        bd, band_pw = check_band(band, iq.shape[0])
        if lb is None and bd is None and not whiten and not fine and not more:
            return self._run(iq.shape[0], lambda eng, s, c: eng.caf(iq[s:s + c], doppler_cps, pairs), 4,
                             (np.int32, np.int32, np.float32, np.float32), P)

        def block_call(eng, s, c):
            return eng.caf(iq[s:s + c], doppler_cps, pairs,
                           lag_bounds=None if lb is None else (lb[s:s + c] if per_window else lb),
                           band=None if bd is None else (bd[s:s + c] if band_pw else bd), whiten=whiten, fine=fine, **more)
        dtypes = (np.int32, np.float32, np.int32, np.float32, np.float32) if fine else (np.int32, np.int32, np.float32, np.float32)
        tails = [()] * len(dtypes)
        if quality:
            dtypes, tails = dtypes + (np.float32,), tails + [(4,)]
        return self._run(iq.shape[0], block_call, len(dtypes), dtypes, P, tails=tails)

    def _caf_integrated(self, iq, doppler_cps, pairs, lag_bounds, band, whiten, fine, more, K, P):
        """caf(integrate=K > 1): whole groups per device, as _correlate_integrated"""
        W = iq.shape[0]
        G = W // K
        lb, per_group = check_lag_bounds(lag_bounds, G, P)
        bd, band_pw = check_band(band, W)
        dtypes = (np.int32, np.float32, np.int32, np.float32, np.float32) if fine else (np.int32, np.int32, np.float32, np.float32)
        tails = [()] * len(dtypes)
        if more.get("quality"):
            dtypes, tails = dtypes + (np.float32,), tails + [(4,)]

        def block_call(eng, gs, gc):
            # the engines are sized for an even split of the WINDOWS; a block of whole groups may be a little larger
            step = getattr(eng, "max_windows", gc * K) // K
            if step < 1:
                raise ValueError(f"integrate = {K} windows per group is more than one device's engine holds "
                                 f"({eng.max_windows} windows)")
            parts = []
            for g0 in range(gs, gs + gc, step):
                g1 = min(g0 + step, gs + gc)
                parts.append(eng.caf(iq[g0 * K:g1 * K], doppler_cps, pairs,
                                     lag_bounds=None if lb is None else (lb[g0:g1] if per_group else lb),
                                     band=None if bd is None else (bd[g0 * K:g1 * K] if band_pw else bd),
                                     whiten=whiten, fine=fine, integrate=K, **more))
            return tuple(np.concatenate([p[k] for p in parts]) for k in range(len(dtypes)))
        return self._run(W, block_call, len(dtypes), dtypes, P, n_rows=G, tails=tails)
