"""CPU-side checks of the batched stream decoder (sfh_inflate_stream_batch*): exported, declared, listed, and refusing bad
arguments before any device is touched; the Python front end checks its arguments before it creates a context."""
import ctypes as C
import os

import pytest

import starflate_amd
from starflate_amd import _capi, build

NEW = ("sfh_inflate_stream_batch_device", "sfh_inflate_stream_batch")


def test_stream_batch_symbols_exported_declared_listed():
    build.build()
    lib = _capi.lib()
    with open(os.path.join(os.path.dirname(build.PKG_DIR), "include", "starflate_hip.h")) as f:
        header = f.read()
    for s in NEW:
        assert s in _capi.EXPORTS and hasattr(lib, s)
        assert f"{s}(" in header


def test_stream_batch_refusals_without_a_device():
    lib = _capi.lib()
    k = 2
    srcs = (C.c_void_p * k)(None, None)
    dsts = (C.c_void_p * k)(None, None)
    n = (C.c_uint64 * k)(0, 0)
    out = (C.c_uint64 * k)()
    st = (C.c_uint32 * k)()
    # a null context
    assert lib.sfh_inflate_stream_batch(None, k, srcs, n, 0, dsts, n, out, st) == -1
    assert lib.sfh_inflate_stream_batch_device(None, k, srcs, n, 0, dsts, n, out, st, None) == -1
    assert lib.sfh_inflate_stream_batch(None, 0, None, None, 0, None, None, None, None) == -1
    # null arrays with count > 0
    assert lib.sfh_inflate_stream_batch(None, k, None, None, 1, None, None, None, None) == -1
    assert lib.sfh_inflate_stream_batch_device(None, k, None, None, 2, None, None, None, None, None) == -1
    # an unknown container, also with count == 0
    assert lib.sfh_inflate_stream_batch(None, 0, None, None, 3, None, None, None, None) == -1
    assert lib.sfh_inflate_stream_batch_device(None, 0, None, None, 3, None, None, None, None, None) == -1


@pytest.mark.parametrize("args, kw", [
    ((b"\x78\x9c",), {}),                                 # one bytes object, not a sequence of streams
    (([b"a", b"b"], [1]), {}),                            # a size per stream
    (([b"a"], [-1]), {}),                                 # a negative size
    (([b"a"], [(1 << 44) + 1]), {}),                      # above 2^44
    (([b"a"],), {"container": "deflate64"}),              # an unknown container
    (([b"a"],), {"container": 1}),                        # containers by name
])
def test_module_level_value_errors(monkeypatch, args, kw):
    def no_context(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")

    monkeypatch.setattr(starflate_amd.compressor, "Compressor", no_context)
    monkeypatch.setattr(starflate_amd.compressor, "_DEFAULT", {})
    with pytest.raises(ValueError):
        starflate_amd.decompress_stream_batch(*args, **kw)


def test_method_value_errors_before_the_device():
    """Compressor.decompress_stream_batch checks the same arguments before any library call (an object without a context)"""
    c = starflate_amd.Compressor.__new__(starflate_amd.Compressor)
    with pytest.raises(ValueError):
        c.decompress_stream_batch([b"a", b"b"], [1, 2, 3], "zlib")
    with pytest.raises(ValueError):
        c.decompress_stream_batch([b"a"], None, "lz4")
