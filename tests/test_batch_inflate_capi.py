"""CPU-side checks of the batched decompression entry points: exported, declared, listed, and refusing bad arguments before
any device is touched."""
import ctypes as C
import os

import pytest

import starflate_amd
from starflate_amd import _capi, build

NEW = ("sfh_batch_index_size", "sfh_copy_batch_index", "sfh_decompress_batch_device_async", "sfh_decompress_batch")


def test_batch_inflate_symbols_exported_declared_listed():
    build.build()
    lib = _capi.lib()
    with open(os.path.join(os.path.dirname(build.PKG_DIR), "include", "starflate_hip.h")) as f:
        header = f.read()
    for s in NEW:
        assert s in _capi.EXPORTS and hasattr(lib, s)
        assert f"{s}(" in header


def test_batch_inflate_refusals_without_a_device():
    lib = _capi.lib()
    k = 2
    srcs = (C.c_void_p * k)(None, None)
    dsts = (C.c_void_p * k)(None, None)
    n = (C.c_uint64 * k)(0, 0)
    st = (C.c_uint32 * k)()
    # a null context
    assert lib.sfh_decompress_batch(None, k, srcs, n, None, None, dsts, n, None, 0, st) == -1
    assert lib.sfh_decompress_batch_device_async(None, k, srcs, n, None, None, dsts, n, None, 0, None, None) == -1
    # null arrays with count > 0
    assert lib.sfh_decompress_batch(None, k, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.sfh_decompress_batch_device_async(None, k, None, None, None, None, None, None, None, 0, None, None) == -1
    # an unknown container, also with count == 0
    assert lib.sfh_decompress_batch(None, k, srcs, n, None, None, dsts, n, None, 3, st) == -1
    assert lib.sfh_decompress_batch_device_async(None, 0, None, None, None, None, None, None, None, 3, None, None) == -1
    # the batch index of a context that is not there
    items, entries = C.c_size_t(0), C.c_size_t(0)
    assert lib.sfh_batch_index_size(None, C.byref(items), C.byref(entries)) == -1
    assert lib.sfh_copy_batch_index(None, None, None, None, 0, None) == -1


@pytest.mark.parametrize("kw, what", [
    (dict(streams=[b"a", b"b"], sizes=[1]), "sizes"),
    (dict(streams=[b"a"], sizes=[40000]), "at most 32768"),
    (dict(streams=[b"a"], sizes=[10], index=[0, 1, 2]), "entries"),
    (dict(streams=[b"a", b"b"], sizes=[10, 70000], index=[0, 1, 0, 1, 2]), "entries"),
    (dict(streams=[b"a"], sizes=[10], index=[0, 1], subindex=[0] * 63), "words"),
    (dict(streams=[b"a"], sizes=[10], subindex=[0] * 64), "needs an index"),
    (dict(streams=[b"a"], sizes=[10], block_bytes=[0, 0]), "one value per item"),
    (dict(streams=[b"a"], sizes=[10], container="lz4"), "container"),
])
def test_batch_inflate_python_validation(kw, what):
    # raised by the argument check, before a context (and so a device) is asked for
    with pytest.raises(ValueError, match=what):
        starflate_amd.decompress_batch(**kw)
