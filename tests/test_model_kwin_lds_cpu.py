"""tools/model_kwin_lds.py executes the index maps of k_win's LDS exchanges (fft_r16.hpp) with symbolic payloads.  Here:
the forward-only image [k0][n1][n0 >> 3][p][n0 & 7] delivers role A's sixteen stores to the role-B thread that needs them,
inside the k0 row's own region, with ZERO bank conflicts on both sides under the lane-group rules of the instructions
(ds_write_b64: four groups of 16 consecutive lanes over 32 banks; ds_read_b64: two groups of 32 lanes over 64 banks) -- and
the model's other checks (data flow of both directions, the banks of the images the inverse transforms keep) still hold."""
import importlib.util
import os

from conftest import ROOT


def _model():
    spec = importlib.util.spec_from_file_location("model_kwin_lds", os.path.join(ROOT, "tools", "model_kwin_lds.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_forward_image_is_conflict_free_on_both_sides():
    m = _model()
    res = m.check_forward_image()
    assert set(res) == {"A write (b64, forward image)", "B read  (b64, forward image)"}
    assert all(v == 1 for v in res.values()), res


def test_forward_image_matches_the_kernel_index_functions():
    """the two bases as fft_r16.hpp computes them from the thread index (xa2f_base, xb2f_base), against the model's digits"""
    m = _model()
    for t in range(512):
        p, u = t & 1, t >> 1
        assert m.xa2f(t, 0) == 32 * (u >> 4) + 16 * ((u >> 3) & 1) + 8 * p + (u & 7)
        assert m.xb2f(t, 0) == (t >> 5) * m.K_BC_HALF + 16 * ((t >> 3) & 1) + 8 * ((t >> 4) & 1) + (t & 7)
        assert m.xa2f(t, 5) - m.xa2f(t, 0) == 5 * m.K_BC_HALF and m.xb2f(t, 5) - m.xb2f(t, 0) == 5 * 32


def test_the_other_exchanges_are_what_they_were():
    m = _model()
    m.check_dataflow()
    m.check_banks()     # asserts 1-way everywhere but role A's stores into the inverse layout (2-way: the image fwd left)
