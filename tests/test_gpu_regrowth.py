"""A ctx that has grown, shrunk and grown further answers as a fresh one does.  Every work buffer of a ctx is a growable
buffer that reallocates when a call needs more than it holds (radio-mapper_amd/csrc/dev_buf.hpp) and keeps its block
when a call needs less; the cached ones (pair plan, pair lists, Doppler phasors, detection twiddles) refill when their key
changes.  Per entry family ONE ctx takes a sequence of host-pointer calls whose window and pair counts go up, down and
further up; every output of every call must be byte for byte that of the same call on a ctx created for it alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DOP = np.array([-2e-4, -1e-4, 0.0, 1e-4, 2e-4])
ONE, TWO, BACK = [[0, 2]], [[0, 2], [1, 2]], [[1, 2], [0, 1], [0, 2]]


@pytest.fixture(scope="module")
def rm():
    import __graft_entry__ as g
    g.build()
    import radio_mapper_amd as rm
    from radio_mapper_amd import xcorr
    assert xcorr.device_count() > 0, "no MI355X visible"
    return rm


_iq = {}


def windows(rm, B, N, W):
    if (B, N) not in _iq or _iq[B, N].shape[0] < W:
        _iq[B, N] = np.ascontiguousarray(rm.synth.make_windows(W, B, N, 10e6, seed=3)[0])
    return _iq[B, N]


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, k)


def replay(rm, shape, calls, run, peak=2):
    """calls: [(n_windows, arguments)]; run(engine, iq[:n_windows], arguments) -> tuple of arrays, the peaks at [peak]"""
    from radio_mapper_amd import xcorr
    B, N, W = shape
    iq = windows(rm, B, N, W)
    with xcorr.XcorrEngine(B, N, W) as kept:
        for k, (w, args) in enumerate(calls):
            got = run(kept, iq[:w], args)
            assert got[peak].shape[0] == w and np.all(got[peak] > 0), "the call found nothing: not a comparison"
            with xcorr.XcorrEngine(B, N, W) as fresh:
                want = run(fresh, iq[:w], args)
            same(got, want, (shape, k, w, args))


# grow, shrink, grow further: windows and pairs, the default list (the fused kernels) and custom ones (the per-transform kernels)
SEQ8 = [(2, ONE), (8, TWO), (1, None), (4, BACK), (8, None), (8, BACK)]


@pytest.mark.parametrize("shape,calls", [
    ((3, 4096, 264), [(8, None), (264, TWO), (4, ONE), (264, None), (264, BACK)]),
    ((3, 1024, 8), SEQ8),
    ((3, 8192, 8), SEQ8),
    ((3, 65536, 2), [(1, ONE), (2, None), (1, TWO), (2, BACK)]),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_correlation(rm, shape, calls):
    replay(rm, shape, calls, lambda e, iq, pairs: e.correlate(iq, pairs=pairs))


@pytest.mark.parametrize("shape", [(3, 4096, 8), (3, 1024, 8), (3, 65536, 2)], ids=lambda v: "x".join(map(str, v)))
def test_correlation_with_quality(rm, shape):
    calls = SEQ8 if shape[2] == 8 else [(1, ONE), (2, None), (1, TWO), (2, BACK)]
    # (every other call with a band and lag bounds: one pass through the per-transform kernels, both stages in use)
    def run(e, iq, a):
        k, pairs = a
        P = 3 if pairs is None else len(pairs)
        extra = dict(band=[-0.2, 0.3], whiten=True, lag_bounds=[[-40 - k, 40 + k]] * P, refine=4) if k % 2 else {}
        return e.correlate(iq, pairs=pairs, quality=True, **extra)
    replay(rm, shape, [(w, (k, p)) for k, (w, p) in enumerate(calls)], run)


@pytest.mark.parametrize("shape", [(3, 4096, 8), (3, 1024, 8), (3, 65536, 2)], ids=lambda v: "x".join(map(str, v)))
def test_doppler_search_with_dop_frac(rm, shape):
    ws = (2, 8, 1, 4, 8, 8) if shape[2] == 8 else (1, 2, 1, 2, 2, 2)
    grids = (DOP[1:4], DOP, DOP[2:3], DOP[::2], DOP, DOP[::-1].copy())   # the grid grows, shrinks, and changes at equal length
    pairs = (ONE, TWO, None, BACK, None, BACK)
    if shape[1] == 65536:
        ws, grids, pairs = ws[:4], [g[:3] for g in grids[:4]], pairs[:4]
    replay(rm, shape, [(w, (g, p)) for w, g, p in zip(ws, grids, pairs)], lambda e, iq, a: e.caf(iq, a[0], pairs=a[1], fine=True), peak=4)


def test_solve(rm):
    from radio_mapper_amd import xcorr
    rng = np.random.default_rng(5)
    xyz = rng.normal(0.0, 3000.0, (5, 3))
    with xcorr.XcorrEngine(3, 1024, 8) as kept:
        for w, b in [(3, 4), (200, 5), (1, 3), (64, 4), (500, 5)]:
            P = b * (b - 1) // 2
            src = rng.normal(0.0, 2000.0, (w, 3))
            d = np.linalg.norm(src[:, None, :] - xyz[None, :b, :], axis=2) / 299792458.0 * 10e6
            i, j = np.triu_indices(b, 1)
            lag = d[:, j] - d[:, i]
            li = np.floor(lag).astype(np.int32)
            lf = (lag - li).astype(np.float32)
            for weight, pairs in ((None, None), (rng.random((w, P)).astype(np.float32), np.stack([i, j], 1))):
                got = kept.solve(xyz[:b], li, lf, 10e6, weight=weight, pairs=pairs)
                with xcorr.XcorrEngine(3, 1024, 8) as fresh:
                    want = fresh.solve(xyz[:b], li, lf, 10e6, weight=weight, pairs=pairs)
                same(got, want, ("solve", w, b, pairs is None))


def test_detect_alternating_window_lengths(rm):
    from radio_mapper_amd import xcorr
    long_, short = windows(rm, 3, 4096, 8).reshape(-1, 4096), windows(rm, 3, 1024, 8).reshape(-1, 1024)
    with xcorr.XcorrEngine(3, 1024, 8) as kept:
        for k, (iq, w, peaks) in enumerate([(short, 2, 16), (long_, 6, 64), (short, 1, 8), (long_, 3, 256), (short, 24, 64), (long_, 24, 512)]):
            args = dict(threshold_db=-200.0, distance=3 + k, min_confidence=0.0, max_peaks=peaks)
            got = kept.detect(iq[:w], **args)
            with xcorr.XcorrEngine(3, 1024, 8) as fresh:
                want = fresh.detect(iq[:w], **args)
            assert len(got) == len(want) == w and all(len(x[0]) > 0 for x in got), "no peaks: not a comparison"
            for x, y in zip(got, want):
                same(x[:4], y[:4], ("detect", k))
                assert np.float32(x[4]).tobytes() == np.float32(y[4]).tobytes()
