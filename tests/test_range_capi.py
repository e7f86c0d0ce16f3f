"""CPU-side checks of the random-access entry points (sfh_decompress_range*): exported, declared, listed, and refusing bad
arguments before any device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import starflate_amd
from starflate_amd import _capi, build

NEW = ("sfh_decompress_ranges_device_async", "sfh_decompress_range_device", "sfh_decompress_ranges")


def test_range_symbols_exported_declared_listed():
    build.build()
    lib = _capi.lib()
    with open(os.path.join(os.path.dirname(build.PKG_DIR), "include", "starflate_hip.h")) as f:
        header = f.read()
    for s in NEW:
        assert s in _capi.EXPORTS and hasattr(lib, s)
        assert f"{s}(" in header
    for name in ("decompress_range", "decompress_ranges"):
        assert name in starflate_amd.__all__ and callable(getattr(starflate_amd, name))
        assert callable(getattr(starflate_amd.Compressor, name))
    assert callable(starflate_amd.Compressor.decompress_ranges_tensors)


def test_range_refusals_without_a_device():
    lib = _capi.lib()
    k = 2
    buf = np.zeros(64, np.uint8)
    idx = np.zeros(2, np.uint64)
    off = (C.c_uint64 * k)(0, 4)
    ln = (C.c_uint64 * k)(4, 4)
    dsts = (C.c_void_p * k)(buf.ctypes.data, buf.ctypes.data + 8)
    st = (C.c_uint32 * k)()
    src, ix = buf.ctypes.data + 16, idx.ctypes.data
    # a null context, whatever else is passed: sound arguments ...
    assert lib.sfh_decompress_ranges(None, src, 16, ix, None, 1, 8, 0, k, off, ln, dsts, st) == -1
    assert lib.sfh_decompress_ranges_device_async(None, src, 16, ix, None, 1, 8, 0, k, off, ln, dsts, st, None) == -1
    assert lib.sfh_decompress_range_device(None, src, 16, ix, None, 1, 8, 0, 0, 4, buf.ctypes.data, st, None) == -1
    # ... no ranges at all ...
    assert lib.sfh_decompress_ranges(None, src, 16, ix, None, 1, 8, 0, 0, None, None, None, None) == -1
    assert lib.sfh_decompress_ranges_device_async(None, src, 16, ix, None, 1, 8, 0, 0, None, None, None, None, None) == -1
    # ... null arrays with count > 0, a null destination with a length
    assert lib.sfh_decompress_ranges(None, None, 0, None, None, 1, 8, 0, k, None, None, None, None) == -1
    assert lib.sfh_decompress_ranges_device_async(None, None, 0, None, None, 1, 8, 0, k, None, None, None, None, None) == -1
    assert lib.sfh_decompress_range_device(None, src, 16, ix, None, 1, 8, 0, 0, 4, None, st, None) == -1
    # ... a range behind total_n, one that overflows, nseg not matching total_n, a bad block_bytes
    bad = (C.c_uint64 * k)(6, 4)
    assert lib.sfh_decompress_ranges(None, src, 16, ix, None, 1, 8, 0, k, bad, ln, dsts, st) == -1
    huge = (C.c_uint64 * k)((1 << 64) - 2, 4)
    assert lib.sfh_decompress_ranges(None, src, 16, ix, None, 1, 8, 0, k, huge, ln, dsts, st) == -1
    assert lib.sfh_decompress_ranges(None, src, 16, ix, None, 2, 8, 0, k, off, ln, dsts, st) == -1
    assert lib.sfh_decompress_ranges(None, src, 16, ix, None, 1, 8, 1000, k, off, ln, dsts, st) == -1
    assert lib.sfh_decompress_ranges(None, src, 16, ix, None, 1, 8, 1 << 25, k, off, ln, dsts, st) == -1
    # ... misaligned device pointers (source 4, index 8, sub-index 4, status 4)
    assert lib.sfh_decompress_ranges_device_async(None, src + 1, 15, ix, None, 1, 8, 0, k, off, ln, dsts, st, None) == -1
    assert lib.sfh_decompress_ranges_device_async(None, src, 16, ix + 4, None, 1, 8, 0, k, off, ln, dsts, st, None) == -1
    assert lib.sfh_decompress_ranges_device_async(None, src, 16, ix, src + 2, 1, 8, 0, k, off, ln, dsts, st, None) == -1
    assert lib.sfh_decompress_ranges_device_async(None, src, 16, ix, None, 1, 8, 0, k, off, ln, dsts, C.addressof(st) + 1, None) == -1
    # ... overlapping destinations
    over = (C.c_void_p * k)(buf.ctypes.data, buf.ctypes.data + 3)
    assert lib.sfh_decompress_ranges(None, src, 16, ix, None, 1, 8, 0, k, off, ln, over, st) == -1
    assert lib.sfh_decompress_ranges_device_async(None, src, 16, ix, None, 1, 8, 0, k, off, ln, over, st, None) == -1


IX2 = [0, 10, 20]  # a stream of two segments


@pytest.mark.parametrize("kw, what", [
    (dict(total_n=40000, offsets=[39000], lengths=[1001]), "does not lie inside"),
    (dict(total_n=40000, offsets=[40001], lengths=[0]), "does not lie inside"),
    (dict(total_n=40000, offsets=[-1], lengths=[4]), "does not lie inside"),
    (dict(total_n=40000, offsets=[0, 4], lengths=[4]), "offsets but"),
    (dict(total_n=70000, offsets=[0], lengths=[4]), "entries"),
    (dict(total_n=40000, offsets=[0], lengths=[4], subindex=[0] * 64), "words"),
    (dict(total_n=40000, offsets=[0], lengths=[4], block_bytes=1000), "block_bytes"),
    (dict(total_n=-1, offsets=[0], lengths=[0]), "total_n"),
])
def test_range_python_validation(kw, what):
    # raised by the argument check, before a context (and so a device) is asked for
    kw.setdefault("block_bytes", 32768)
    with pytest.raises(ValueError, match=what):
        starflate_amd.decompress_ranges(b"x" * 20, IX2, **kw)


def test_range_python_validation_single():
    with pytest.raises(ValueError, match="does not lie inside"):
        starflate_amd.decompress_range(b"x" * 20, IX2, 40000, 39999, 2, block_bytes=32768)
    with pytest.raises(ValueError, match="entries"):
        starflate_amd.decompress_range(b"x" * 20, [0, 10], 40000, 0, 2, block_bytes=32768)
