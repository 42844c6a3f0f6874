"""Guarded slabs for the caller's buffers (numpy only): tests/test_gpu_caller_memory.py lays the input of a call in one slab
and all its outputs in another, every array between two guards, fills guards and outputs with a pattern no entry can
produce, and after the call asks check() what changed where.  tests/test_caller_memory_cpu.py tests this file itself.

layout(arrays, placement): arrays = [(name, dtype, n_elems), ...] -> a Layout of byte offsets inside ONE slab whose base is
  aligned to 256 bytes or better (what torch.empty returns; numpy_slab() gives the same for numpy).  Every array has a guard
  of g = max(256, n_elems) elements of its own dtype directly in front of it and directly behind it, and the guards of
  neighbouring arrays do not overlap: an output slot index wrong by a whole window, band or chunk still lands in a guard.
  placement "aligned": every array starts on a 256-byte boundary of the slab.
  placement "natural": every array starts at its element alignment and nothing more --
      4-byte elements (the outputs): the k-th such array of the list at 4 (k mod 3 + 1) mod 16, so lag_int, lag_frac, peak
          sit at 4, 8, 12 mod 16 and a fourth array (quality; dop_idx where it is listed last) at 4 mod 16;
      8-byte elements (complex64 input): at 8 mod 16;
      1-byte elements (uint8 I,Q input): at 2 mod 16 -- one I,Q pair, the element the kernels load.
fill(layout): the slab as uint8, every byte 0xA5: every 32-bit word of outputs and guards holds 0xA5A5A5A5, a negative
  float of magnitude 2.9e-16 (no peak, lag_frac or quality figure is negative) and the integer -1515870811, far outside
  +-(N - 1) for every N the library takes.  put() then writes the input windows into their body.
check(before, after, layout, written): a list of Finding(array, side, index) --
  every guard element that changed (side "front" or "back"), every element of an array NOT in `written` that changed and
  every element of an array in `written` that still holds the fill (side "body").  index counts elements of the array's
  dtype from the array's first element: a front guard has -g .. -1, the body 0 .. n - 1, a back guard n .. n + g - 1.
  A changed byte of the alignment padding between two arrays' guards is reported with the array behind it, side "front" and
  an index below -g (behind the last array: side "back", an index from n + g on)."""
from collections import namedtuple

import numpy as np

FILL_BYTE = 0xA5
FILL_WORD = 0xA5A5A5A5
BASE_ALIGN = 256
PLACEMENTS = ("aligned", "natural")

Entry = namedtuple("Entry", "name dtype n guard front offset back end")   # bytes: front guard, body, back guard, its end
Layout = namedtuple("Layout", "entries nbytes placement")
Finding = namedtuple("Finding", "array side index")


def _residue(itemsize, k4):
    if itemsize == 4:
        return 4 * (k4 % 3 + 1)
    if itemsize == 8:
        return 8
    if itemsize == 1:
        return 2
    raise ValueError(f"no natural placement for elements of {itemsize} bytes")


def layout(arrays, placement):
    if placement not in PLACEMENTS:
        raise ValueError(f"placement must be one of {PLACEMENTS}, got {placement!r}")
    entries, pos, k4 = {}, 0, 0
    for name, dtype, n in arrays:
        dt = np.dtype(dtype)
        n = int(n)
        if name in entries or n < 1:
            raise ValueError(f"bad array {name!r} of {n} elements")
        g = max(256, n)
        start = pos + g * dt.itemsize                    # the earliest body behind a whole guard of its own
        if placement == "aligned":
            off = -(-start // BASE_ALIGN) * BASE_ALIGN
        else:
            off = start + (_residue(dt.itemsize, k4) - start) % 16
        k4 += dt.itemsize == 4
        end = off + (n + g) * dt.itemsize
        entries[name] = Entry(name, dt, n, g, off - g * dt.itemsize, off, off + n * dt.itemsize, end)
        pos = end
    return Layout(entries, -(-pos // BASE_ALIGN) * BASE_ALIGN, placement)


def numpy_slab(nbytes):
    """nbytes of uint8, uninitialised, whose first byte is aligned to BASE_ALIGN (numpy itself promises 16 or 64)"""
    raw = np.empty(nbytes + BASE_ALIGN, np.uint8)
    skip = -raw.ctypes.data % BASE_ALIGN
    out = raw[skip:skip + nbytes]
    assert out.ctypes.data % BASE_ALIGN == 0
    return out


def fill(lay, slab=None):
    if slab is None:
        slab = numpy_slab(lay.nbytes)
    assert slab.dtype == np.uint8 and slab.shape == (lay.nbytes,)
    slab[:] = FILL_BYTE
    return slab


def put(slab, lay, name, values):
    e = lay.entries[name]
    v = np.ascontiguousarray(values).reshape(-1).view(e.dtype)
    assert v.size == e.n, (name, v.size, e.n)
    slab[e.offset:e.back] = v.view(np.uint8)


def cut(slab, lay, name, shape=None):
    """a copy of the body of `name` in its dtype (the slab's own bytes may be aligned to the element only)"""
    e = lay.entries[name]
    a = slab[e.offset:e.back].copy().view(e.dtype)
    return a if shape is None else a.reshape(shape)


def _elements(slab, lo, hi, dt):
    return slab[lo:hi].copy().view(dt) if dt.itemsize > 1 else slab[lo:hi]


def check(before, after, lay, written):
    written = set(written)
    unknown = written - set(lay.entries)
    if unknown:
        raise ValueError(f"written names arrays the layout does not have: {sorted(unknown)}")
    assert before.shape == after.shape == (lay.nbytes,) and before.dtype == after.dtype == np.uint8
    out = []
    for e in lay.entries.values():
        bits = np.dtype(f"u{e.dtype.itemsize}")
        for side, lo, hi, first in (("front", e.front, e.offset, -e.guard), ("back", e.back, e.end, e.n)):
            changed = _elements(before, lo, hi, bits) != _elements(after, lo, hi, bits)
            out += [Finding(e.name, side, first + int(i)) for i in np.nonzero(changed)[0]]
        body = _elements(after, e.offset, e.back, bits)
        if e.name in written:
            pattern = np.frombuffer(bytes([FILL_BYTE]) * e.dtype.itemsize, bits)[0]
            bad = body == pattern
        else:
            bad = body != _elements(before, e.offset, e.back, bits)
        out += [Finding(e.name, "body", int(i)) for i in np.nonzero(bad)[0]]
    # the alignment padding between one array's back guard and the next one's front guard (and at either end of the slab)
    # belongs to nobody and must not change either: reported with the array it lies in front of (behind the last one),
    # the index continuing that guard's count
    entries = list(lay.entries.values())
    gaps = [(p.end if p else 0, e.front, e, "front") for p, e in zip([None] + entries[:-1], entries)]
    gaps.append((entries[-1].end, lay.nbytes, entries[-1], "back"))
    for lo, hi, e, side in gaps:
        for i in np.nonzero(before[lo:hi] != after[lo:hi])[0]:
            out.append(Finding(e.name, side, (lo + int(i) - e.offset) // e.dtype.itemsize))
    return out
