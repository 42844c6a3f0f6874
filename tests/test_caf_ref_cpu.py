"""tests/caf_ref.py, the reference side of tests/test_gpu_caf.py, checked on the CPU alone: it restates the oracle's
caf_pair hypothesis by hypothesis, its selection rule keeps the lowest index on ties, the phasor table of rmx_caf_batch
holds the oracle's values, and every seeded scene of the GPU tests separates its hypotheses by more than the bar under
which "dop_idx exact" is demanded."""
import os

import numpy as np
import pytest

import caf_ref as cr
from oracle import xcorr_ref as orc


@pytest.mark.parametrize("name", ["caf_b3_n4096", "caf_b3_n1024", "caf_b4_n2048_d21"])
def test_bin_peaks_and_first_max_reproduce_the_fixtures(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    iq = orc.decode_u8_iq(g["raw_u8"])
    pk, li, lf = cr.bin_peaks(iq, g["doppler_cps"])
    assert np.array_equal(pk, g["bin_peak"]) and np.array_equal(li, g["bin_lag"])
    dop = cr.first_max(pk)
    assert np.array_equal(dop, g["dop_idx"])
    rd, ri, rf, rp = orc.caf_batch(iq, g["doppler_cps"])
    assert np.array_equal(dop, rd) and np.array_equal(cr.take(li, dop), ri)
    assert np.array_equal(cr.take(lf, dop), rf) and np.array_equal(cr.take(pk, dop), rp)
    # a custom list with a reversed and a repeated pair, through reference(): still caf_batch
    sel = cr.custom_pairs(iq.shape[1])
    ref = cr.reference(iq[:1], g["doppler_cps"], sel)
    rd, ri, rf, rp = orc.caf_batch(iq[:1], g["doppler_cps"], sel)
    assert np.array_equal(ref["dop"], rd) and np.array_equal(ref["lag_int"], ri)
    assert np.array_equal(ref["lag_frac"], rf) and np.array_equal(ref["peak"], rp)
    assert np.array_equal(ref["hyp_margin"], cr.hypothesis_margin(ref["bin_peak"])) and ref["hyp_margin"].min() > cr.MARGIN_BAR


def test_first_max_keeps_the_lowest_index_on_ties():
    a, b = np.float32(3.0), np.float32(5.0)
    peaks = np.array([[[a, b, a, b, a], [b, a, b, a, b], [a, a, a, a, a], [a, b, np.float32(7.0), np.float32(7.0), b]]])
    assert np.array_equal(cr.first_max(peaks), [[1, 0, 0, 2]])
    assert cr.first_max(np.zeros((2, 3, 4), np.float32)).any() == 0
    # the same rule as caf_pair on windows that tie exactly: a repeated hypothesis repeats its peak bit for bit
    iq, _, grid, _ = cr.scene(1, 2, 64, 3, seed=5)
    tiled = np.array([grid[2], grid[0], grid[2], grid[0], grid[2]])
    pk, _, _ = cr.bin_peaks(iq, tiled)
    assert np.array_equal(pk[..., 0], pk[..., 2]) and np.array_equal(pk[..., 0], pk[..., 4])
    assert np.array_equal(cr.first_max(pk), orc.caf_batch(iq, tiled)[0])
    assert np.array_equal(cr.first_max(pk), cr.first_max(pk[..., :2]))
    m = cr.hypothesis_margin(pk)
    assert np.all(m == 0.0) and np.all(cr.hypothesis_margin(pk[..., :1]) == np.inf)


def _grids():
    """every nu that tests/test_gpu_caf.py hands to the library, with its window length"""
    out = []
    for W, B, N, D, seed in cr.SCENES.values():
        out += [(nu, N) for nu in (np.arange(D) - D // 2) * (0.5 / N)]
    for N in (256, 1024, 4096, 8192):                       # the D = 1, 2, 3, 9 grids of the exact / state / door tests
        out += [(k * 0.5 / N, N) for k in range(-4, 5)]
    grid = cr.limit_scene()[2]
    out += [(nu, 256) for nu in grid[::37]] + [(grid[0], 256), (grid[-1], 256)]
    return out


def test_libm_phasor_holds_the_oracles_values():
    """cos / sin of the C library in double against numpy's complex exp: equal as VALUES for every hypothesis in use (the
    two may differ in the sign of a zero, which no product with a finite sample can show in |c|)."""
    seen = set()
    for nu, N in _grids():
        if (nu, N) in seen:
            continue
        seen.add((nu, N))
        a, b = cr.libm_phasor(nu, N), orc.doppler_phasor(nu, N)
        assert a.dtype == np.complex64 and a.shape == (N,)
        assert np.array_equal(a.real, b.real) and np.array_equal(a.imag, b.imag), (nu, N)
    assert len(seen) > 100


def test_rot_mul_is_the_unfused_product():
    """four products, a difference and a sum, each rounded to float32: checked against exact rational arithmetic on the
    doubles (a float32 product is exact in double), and within one float32 ulp of numpy's own complex64 product."""
    rng = np.random.default_rng(7)
    x = ((rng.integers(0, 256, 4096) - 127.5) + 1j * (rng.integers(0, 256, 4096) - 127.5)).astype(np.complex64)
    r = cr.libm_phasor(0.000123, 4096)
    got = cr.rot_mul(x, r)
    xr, xi, rr, ri = (v.astype(np.float64) for v in (x.real, x.imag, r.real, r.imag))
    f32 = lambda v: v.astype(np.float32).astype(np.float64)   # noqa: E731
    assert np.array_equal(got.real, (f32(xr * rr) - f32(xi * ri)).astype(np.float32))
    assert np.array_equal(got.imag, (f32(xr * ri) + f32(xi * rr)).astype(np.float32))
    ref = (x * r).astype(np.complex64)
    assert np.all(np.abs(got.real - ref.real) <= np.spacing(np.maximum(np.abs(ref.real), np.abs(x.real * r.real))))
    assert np.all(np.abs(got.imag - ref.imag) <= np.spacing(np.maximum(np.abs(ref.imag), np.abs(x.real * r.imag))))


@pytest.mark.parametrize("name", sorted(cr.SCENES))
def test_every_scene_separates_its_hypotheses(name):
    """a condition on the INPUTS of the GPU tests: best against second-best hypothesis above 1e-3 in every pair-window,
    for the default and for the custom pair list; offsets on the grid, different from window to window, and the uint8 form
    decodes to the complex64 one"""
    W, B, N, D, seed = cr.SCENES[name]
    iq, raw, grid, k = cr.scene_of(name)
    assert iq.shape == (W, B, N) and raw.shape == (W, B, 2 * N) and np.array_equal(orc.decode_u8_iq(raw), iq)
    assert grid.shape == (D,) and np.all(np.diff(grid) == 0.5 / N) and grid[D // 2] == 0.0
    assert k.min() >= 0 and k.max() <= D // 2 and all(not np.array_equal(k[w], k[w - 1]) for w in range(1, W))
    for pl in (None, cr.custom_pairs(B)):
        pk, _, _ = cr.bin_peaks(iq, grid, pl)
        assert cr.hypothesis_margin(pk).min() > cr.MARGIN_BAR, (name, cr.hypothesis_margin(pk).min())
        assert len({tuple(row) for row in cr.first_max(pk).tolist()}) > 1    # not the same row of hypotheses in every window


def test_the_limit_scene_separates_its_hypotheses():
    iq, raw, grid, at = cr.limit_scene()
    assert grid.shape == (4096,) and len(set(grid.tolist())) == 4096 and np.array_equal(orc.decode_u8_iq(raw), iq)
    pk, _, _ = cr.bin_peaks(iq, grid)
    assert cr.first_max(pk)[0, 0] == at and cr.hypothesis_margin(pk).min() > cr.MARGIN_BAR
