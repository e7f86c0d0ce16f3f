"""CPU-side checks of the batched index-free decoder (sfh_recover_index_batch*, sfh_decompress_any_batch*): exported,
declared, listed, and refusing bad arguments before any device is touched; the Python front end checks its arguments before
it creates a context.  (The refusals that need a context -- alignment, sizes, overlap -- are test_gpu_any_batch.py's.)"""
import ctypes as C
import os

import pytest

import starflate_amd
from starflate_amd import _capi, build

NEW = ("sfh_recover_index_batch_device", "sfh_recover_index_batch", "sfh_decompress_any_batch_device", "sfh_decompress_any_batch")
TRAILER = _capi.SIZE_FROM_TRAILER


def test_any_batch_symbols_exported_declared_listed():
    build.build()
    lib = _capi.lib()
    with open(os.path.join(os.path.dirname(build.PKG_DIR), "include", "starflate_hip.h")) as f:
        header = f.read()
    for s in NEW:
        assert s in _capi.EXPORTS and hasattr(lib, s)
        assert f"{s}(" in header
    assert "#define SFH_ITEM_NOT_INDEXABLE 0xFFFFFFF8u" in header
    assert _capi.ITEM_NOT_INDEXABLE == starflate_amd.ITEM_NOT_INDEXABLE == (-8) & 0xFFFFFFFF


def test_any_batch_refusals_without_a_device():
    lib = _capi.lib()
    k = 2
    buf = (C.c_uint8 * 256)()
    base = C.addressof(buf)
    srcs = (C.c_void_p * k)(base, base + 64)
    dsts = (C.c_void_p * k)(base + 128, base + 192)
    n = (C.c_uint64 * k)(8, 8)
    cap = (C.c_uint64 * k)(16, 16)
    want = (C.c_uint64 * k)(16, 16)
    out = (C.c_uint64 * k)()
    ix = (C.c_uint64 * (2 * k))()
    st = (C.c_uint32 * k)()

    def calls(count, srcs, n, container, dsts, cap, want, out, ix, st):
        return (lib.sfh_decompress_any_batch(None, count, srcs, n, container, dsts, cap, want, out, st),
                lib.sfh_decompress_any_batch_device(None, count, srcs, n, container, dsts, cap, want, out, st, None),
                lib.sfh_recover_index_batch(None, count, srcs, n, container, want, ix, st),
                lib.sfh_recover_index_batch_device(None, count, srcs, n, container, want, ix, st, None))

    # a null context: with good arguments, with count == 0, with an unknown container
    assert calls(k, srcs, n, 0, dsts, cap, want, out, ix, st) == (-1,) * 4
    assert calls(0, None, None, 0, None, None, None, None, None, None) == (-1,) * 4
    assert calls(0, None, None, 3, None, None, None, None, None, None) == (-1,) * 4
    # null arrays with count > 0
    assert calls(k, None, None, 1, None, None, None, None, None, None) == (-1,) * 4
    # a misaligned source, destination and index; sizes above 2^44; the trailer's size without gzip; overlapping destinations
    assert calls(k, (C.c_void_p * k)(base + 1, base + 64), n, 0, (C.c_void_p * k)(base + 129, base + 192), cap, want, out, ix, st) == (-1,) * 4
    assert lib.sfh_recover_index_batch_device(None, k, srcs, n, 0, want, C.c_void_p(C.addressof(ix) + 4), st, None) == -1
    big = (C.c_uint64 * k)((1 << 44) + 1, 16)
    assert calls(k, srcs, n, 0, dsts, big, big, out, ix, st) == (-1,) * 4
    assert calls(k, srcs, n, 1, dsts, cap, (C.c_uint64 * k)(TRAILER, 16), out, ix, st) == (-1,) * 4
    assert calls(k, srcs, n, 0, (C.c_void_p * k)(base + 128, base + 136), cap, want, out, ix, st) == (-1,) * 4
    assert not any(st) and not any(out) and not any(buf)  # nothing was written


@pytest.mark.parametrize("args, kw", [
    ((b"\x78\x9c",), {}),                                 # one bytes object, not a sequence of streams
    (([b"a", b"b"], [1]), {}),                            # a size per stream
    (([b"a"], [1, 2]), {}),
    (([b"a"], [-1]), {}),                                 # a negative size
    (([b"a"], [(1 << 44) + 1]), {}),                      # above 2^44
    (([b"a"],), {}),                                      # sizes=None: gzip only
    (([b"a"], None), {"container": "zlib"}),
    (([b"a"], [1]), {"container": "deflate64"}),          # an unknown container
    (([b"a"], [1]), {"container": 1}),                    # containers by name
])
@pytest.mark.parametrize("fallback", [True, False])
def test_module_level_value_errors(monkeypatch, args, kw, fallback):
    def no_context(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")

    monkeypatch.setattr(starflate_amd.compressor, "Compressor", no_context)
    monkeypatch.setattr(starflate_amd.compressor, "_DEFAULT", {})
    with pytest.raises(ValueError):
        starflate_amd.decompress_any_batch(*args, fallback=fallback, **kw)


def test_method_value_errors_before_the_device():
    """The Compressor methods check the same arguments before any library call (an object without a context)"""
    c = starflate_amd.Compressor.__new__(starflate_amd.Compressor)
    with pytest.raises(ValueError):
        c.decompress_any_batch([b"a", b"b"], [1, 2, 3], "zlib")
    with pytest.raises(ValueError):
        c.decompress_any_batch([b"a"], None, "raw")
    with pytest.raises(ValueError):
        c.decompress_any_batch([b"a"], [5], "lz4")
    with pytest.raises(ValueError):
        c.decompress_any_batch_tensors([], None, "zlib")
    with pytest.raises(ValueError):
        c.decompress_any_batch_tensors([], [1], "raw")
    with pytest.raises(ValueError):
        c.recover_index_batch([], [-1], "raw")


def test_indexed_batch_call_still_refuses_large_index_free_items():
    with pytest.raises(ValueError, match="at most 32768"):
        starflate_amd.decompress_batch(streams=[b"a"], sizes=[40000])
