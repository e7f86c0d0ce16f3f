"""CPU-side checks of the batched compression entry points: exported, declared, listed, and refusing bad arguments
before any device is touched."""
import ctypes as C

from starflate_amd import _capi, build


def test_batch_symbols_exported_and_listed():
    build.build()
    lib = _capi.lib()
    for s in ("sfh_compress_batch", "sfh_compress_batch_device_async"):
        assert s in _capi.EXPORTS and hasattr(lib, s)


def test_batch_refusals_without_a_device():
    lib = _capi.lib()
    k = 2
    srcs = (C.c_void_p * k)(None, None)
    dsts = (C.c_void_p * k)(None, None)
    n = (C.c_uint64 * k)(0, 0)
    cap = (C.c_uint64 * k)(1 << 20, 1 << 20)
    out = (C.c_uint64 * k)()
    good = _capi.make_options()
    bad = _capi.make_options(container="zlib", final_stream=False)
    # a null context
    assert lib.sfh_compress_batch(None, k, srcs, n, dsts, cap, out, C.byref(good)) == -1
    assert lib.sfh_compress_batch_device_async(None, k, srcs, n, dsts, cap, None, C.byref(good), None) == -1
    # null arrays with count > 0
    assert lib.sfh_compress_batch(None, k, None, None, None, None, None, C.byref(good)) == -1
    assert lib.sfh_compress_batch_device_async(None, k, None, None, None, None, None, C.byref(good), None) == -1
    # bad options
    assert lib.sfh_compress_batch(None, k, srcs, n, dsts, cap, out, C.byref(bad)) == -1
    assert lib.sfh_compress_batch_device_async(None, 0, None, None, None, None, None, C.byref(bad), None) == -1
