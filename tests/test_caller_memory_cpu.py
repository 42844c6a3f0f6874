"""tests/caller_memory_ref.py tested on the CPU: the layout has exactly the residues and guard sizes it states, and the
checker says nothing about a correctly written slab and exactly one thing about one altered word in each place a kernel
could wrongly touch -- so tests/test_gpu_caller_memory.py, which asserts "no finding", can fail."""
import numpy as np
import pytest

import caller_memory_ref as cm

P, R = 3, 6
OUTS = [("lag_int", np.int32, R * P), ("lag_frac", np.float32, R * P), ("peak", np.float32, R * P),
        ("quality", np.float32, 4 * R * P)]
BIG = [("lag_int", np.int32, 521 * 3), ("lag_frac", np.float32, 521 * 3), ("peak", np.float32, 521 * 3)]
IN_C64 = [("iq", np.complex64, 6 * 3 * 256)]
IN_U8 = [("iq", np.uint8, 6 * 3 * 2 * 256)]


@pytest.mark.parametrize("arrays", [OUTS, BIG, IN_C64, IN_U8, OUTS[:3] + [("dop_idx", np.int32, R * P)]],
                         ids=["outs4", "outs_big", "c64", "u8", "caf"])
@pytest.mark.parametrize("placement", cm.PLACEMENTS)
def test_layout_guards_and_residues(arrays, placement):
    lay = cm.layout(arrays, placement)
    assert list(lay.entries) == [a[0] for a in arrays] and lay.nbytes % cm.BASE_ALIGN == 0
    prev_end = 0
    for name, dtype, n in arrays:
        e = lay.entries[name]
        size = np.dtype(dtype).itemsize
        assert e.guard == max(256, n) and e.n == n and e.dtype == np.dtype(dtype)
        assert e.offset - e.front == e.guard * size == e.end - e.back        # both guards whole, directly at the body
        assert e.back - e.offset == n * size
        assert prev_end <= e.front                                           # a neighbour's guard is not shared
        assert e.offset % size == 0 or size == 8 and e.offset % 4 == 0
        prev_end = e.end
    assert prev_end <= lay.nbytes
    want = {"lag_int": 4, "lag_frac": 8, "peak": 12, "quality": 4, "dop_idx": 4}
    for name, dtype, _ in arrays:
        off = lay.entries[name].offset
        if placement == "aligned":
            assert off % 256 == 0
        elif name == "iq":
            assert off % 16 == (8 if np.dtype(dtype) == np.complex64 else 2)
        else:
            assert off % 16 == want[name]


def test_layout_refuses_what_it_cannot_place():
    with pytest.raises(ValueError):
        cm.layout(OUTS, "packed")
    with pytest.raises(ValueError):
        cm.layout([("x", np.int16, 4)], "natural")
    with pytest.raises(ValueError):
        cm.layout([("x", np.int32, 4), ("x", np.int32, 4)], "aligned")


def test_fill_is_a_value_no_entry_produces():
    lay = cm.layout(OUTS, "natural")
    slab = cm.fill(lay)
    assert slab.ctypes.data % cm.BASE_ALIGN == 0 and slab.size == lay.nbytes
    assert np.all(slab.view(np.uint32) == cm.FILL_WORD)
    li, pk = cm.cut(slab, lay, "lag_int"), cm.cut(slab, lay, "peak")
    assert li.dtype == np.int32 and np.all(li == -1515870811) and abs(int(li[0])) > 4194304
    assert pk.dtype == np.float32 and np.all(pk < 0) and np.all(np.abs(pk) < 2.0 ** -51)   # negative and tiny: no magnitude


def _written(lay, before, names):
    after = before.copy()
    rng = np.random.default_rng(5)
    for name in names:
        e = lay.entries[name]
        v = rng.integers(-4095, 4096, e.n).astype(np.int32) if e.dtype == np.int32 else rng.random(e.n).astype(e.dtype)
        cm.put(after, lay, name, v)
        assert np.array_equal(cm.cut(after, lay, name), v)
    return after


@pytest.mark.parametrize("placement", cm.PLACEMENTS)
def test_checker_on_an_output_slab(placement):
    lay = cm.layout(OUTS, placement)
    before = cm.fill(lay)
    names = [a[0] for a in OUTS]
    good = _written(lay, before, names)
    assert cm.check(before, good, lay, names) == []
    # three arrays written where four were asked for: every element of the fourth is reported, nothing else
    three = _written(lay, before, names[:3])
    assert cm.check(before, three, lay, names) == [cm.Finding("quality", "body", i) for i in range(4 * R * P)]
    assert cm.check(before, three, lay, names[:3]) == []
    # ... and a written array that was not to be written ("nothing written" of a refused call) is reported whole
    assert cm.check(before, three, lay, []) == [cm.Finding(n, "body", i) for n in names[:3] for i in range(R * P)]
    for name in names:
        e = lay.entries[name]
        places = {"last front-guard word": (e.offset - 4, "front", -1), "first back-guard word": (e.back, "back", e.n),
                  "far end of the front guard": (e.front, "front", -e.guard),
                  "far end of the back guard": (e.end - 4, "back", e.n + e.guard - 1)}
        for what, (byte, side, index) in places.items():
            bad = good.copy()
            bad[byte:byte + 4] = np.frombuffer(np.float32(1.5).tobytes(), np.uint8)
            assert cm.check(before, bad, lay, names) == [cm.Finding(name, side, index)], what
            one = good.copy()
            one[byte + 3] ^= 1                                              # a single bit of the word
            assert cm.check(before, one, lay, names) == [cm.Finding(name, side, index)], what
        # an unwritten body element: the fill left in the middle and at either end of a written array
        for i in (0, e.n // 2, e.n - 1):
            bad = good.copy()
            bad[e.offset + 4 * i:e.offset + 4 * i + 4] = cm.FILL_BYTE
            assert cm.check(before, bad, lay, names) == [cm.Finding(name, "body", i)]


@pytest.mark.parametrize("arrays", [IN_C64, IN_U8], ids=["c64", "u8"])
@pytest.mark.parametrize("placement", cm.PLACEMENTS)
def test_checker_on_an_input_slab(arrays, placement):
    lay = cm.layout(arrays, placement)
    e = lay.entries["iq"]
    before = cm.fill(lay)
    rng = np.random.default_rng(7)
    cm.put(before, lay, "iq", rng.integers(0, 256, e.n * e.dtype.itemsize).astype(np.uint8).view(e.dtype))
    assert np.all(before[e.front:e.offset] == cm.FILL_BYTE) and np.all(before[e.back:e.end] == cm.FILL_BYTE)
    assert cm.check(before, before.copy(), lay, []) == []
    size = e.dtype.itemsize
    for byte, want in ((e.offset, ("body", 0)), (e.back - 1, ("body", e.n - 1)), (e.offset + 5 * size + size - 1, ("body", 5)),
                       (e.offset - 1, ("front", -1)), (e.front, ("front", -e.guard)), (e.back, ("back", e.n)),
                       (e.end - 1, ("back", e.n + e.guard - 1))):
        after = before.copy()
        after[byte] ^= 0x10                                                 # one input or guard byte
        assert cm.check(before, after, lay, []) == [cm.Finding("iq", *want)], byte


def test_checker_names_the_neighbour_a_wrong_slot_index_lands_in():
    """a store one whole row (P slots) behind the end of lag_frac lands in lag_frac's back guard, not in peak"""
    lay = cm.layout(OUTS, "natural")
    before = cm.fill(lay)
    names = [a[0] for a in OUTS]
    after = _written(lay, before, names)
    e = lay.entries["lag_frac"]
    after[e.back:e.back + 4 * P] = np.frombuffer(np.arange(1, P + 1, dtype=np.float32).tobytes(), np.uint8)
    assert cm.check(before, after, lay, names) == [cm.Finding("lag_frac", "back", e.n + i) for i in range(P)]
    with pytest.raises(ValueError):
        cm.check(before, after, lay, ["lag_frak"])


@pytest.mark.parametrize("placement", cm.PLACEMENTS)
def test_checker_sees_the_padding_between_the_guards(placement):
    """every byte of the slab is somebody's: one changed byte anywhere gives exactly one finding"""
    lay = cm.layout(OUTS, placement)
    before = cm.fill(lay)
    names = [a[0] for a in OUTS]
    good = _written(lay, before, names)
    entries = list(lay.entries.values())
    covered = np.zeros(lay.nbytes, bool)
    for e in entries:
        covered[e.front:e.end] = True
    padding = np.nonzero(~covered)[0]
    assert padding.size > 0
    for byte in (int(padding[0]), int(padding[padding.size // 2]), int(padding[-1])):
        bad = good.copy()
        bad[byte] ^= 0x80
        found = cm.check(before, bad, lay, names)
        assert len(found) == 1 and found[0].side in ("front", "back"), (byte, found)
        e = lay.entries[found[0].array]
        assert found[0].index < -e.guard if found[0].side == "front" else found[0].index >= e.n + e.guard
    outside = np.ones(lay.nbytes, bool)                                     # (a written body may hold anything but the fill)
    for e in entries:
        outside[e.offset:e.back] = False
    rng = np.random.default_rng(9)
    for byte in rng.choice(np.nonzero(outside)[0], 200, replace=False):
        bad = good.copy()
        bad[byte] ^= 0x01
        assert len(cm.check(before, bad, lay, names)) == 1, int(byte)
