"""CPU-side checks of the BGZF entry points (sfh_compress_bgzf*, sfh_bgzf_*, sfh_decompress_bgzf*): exported, declared, listed
and bound in Python; sfh_bgzf_bound's arithmetic; the host walk through the library on Python-made files; refusals before any
device is touched."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import bgzf_files as BZ
import starflate_amd
from starflate_amd import _capi, build

NEW = ("sfh_bgzf_bound", "sfh_compress_bgzf_device_async", "sfh_compress_bgzf_device", "sfh_compress_bgzf", "sfh_bgzf_read_index",
       "sfh_bgzf_read_index_device", "sfh_decompress_bgzf_device", "sfh_decompress_bgzf")


def test_bgzf_symbols_exported_declared_listed():
    build.build()
    lib = _capi.lib()
    with open(os.path.join(os.path.dirname(build.PKG_DIR), "include", "starflate_hip.h")) as f:
        header = f.read()
    for s in NEW:
        assert s in _capi.EXPORTS and hasattr(lib, s)
        assert f"{s}(" in header
    assert "typedef struct sfh_bgzf_info" in header and C.sizeof(_capi.BgzfInfo) == 24
    assert "bgzf" not in _capi.CONTAINER and "bgzf" not in _capi.COMPRESS_CONTAINER  # entry points, not a container value
    for name in ("compress_bgzf", "decompress_bgzf", "bgzf_index"):
        assert name in starflate_amd.__all__ and callable(getattr(starflate_amd, name))
        assert callable(getattr(starflate_amd.Compressor, name))
    assert "sf_bgzf.hip" in build.SOURCES


def test_bound_arithmetic():
    lib = _capi.lib()
    per = lib.sfh_compress_bound(32768, 0) + 26
    for n, members in ((0, 1), (1, 1), (32768, 1), (32769, 2), (3 * 32768 + 5, 4)):
        assert lib.sfh_bgzf_bound(n) == members * per + 28 == starflate_amd.Compressor.bgzf_bound(n)
    assert per <= 65536  # a member of one chunk always fits BSIZE


def test_refusals_with_a_null_context_or_null_pointers():
    lib = _capi.lib()
    buf = np.zeros(256, np.uint8)
    idx = np.zeros(16, np.uint64)
    info = _capi.BgzfInfo()
    n64, st, out_n = C.c_uint64(0), C.c_uint32(0), C.c_size_t(0)
    p, a, b = buf.ctypes.data, idx.ctypes.data, idx.ctypes.data + 64
    opt = _capi.make_options()
    assert lib.sfh_compress_bgzf(None, p, 64, p + 128, 128, C.byref(out_n), C.byref(opt)) == -1
    assert lib.sfh_compress_bgzf_device(None, p, 64, p + 128, 128, C.byref(out_n), C.byref(opt), None) == -1
    assert lib.sfh_compress_bgzf_device_async(None, p, 64, p + 128, 128, p, C.byref(opt), None) == -1
    assert lib.sfh_bgzf_read_index_device(None, p, 64, C.byref(info), a, b, 8, None) == -1
    assert lib.sfh_decompress_bgzf_device(None, p, 64, p + 128, 64, C.byref(n64), C.byref(st), None) == -1
    assert lib.sfh_decompress_bgzf(None, p, 64, p + 128, 64, C.byref(n64), C.byref(st)) == -1
    # the host reader: null pointers
    assert lib.sfh_bgzf_read_index(p, 64, None, a, b, 8) == -1
    assert lib.sfh_bgzf_read_index(None, 64, C.byref(info), a, b, 8) == -1
    assert lib.sfh_bgzf_read_index(p, 64, C.byref(info), None, b, 8) == -1
    assert lib.sfh_bgzf_read_index(p, 64, C.byref(info), a, None, 8) == -1


def test_host_walk_through_the_library():
    lib = _capi.lib()
    for name, (data, blob, want_m, want_o, eof) in BZ.good_files().items():
        src = np.frombuffer(blob, np.uint8)
        m = len(want_m) - 1
        moff, ooff = np.full(m + 2, 7, np.uint64), np.full(m + 2, 7, np.uint64)
        info = _capi.BgzfInfo(1, 2, 3, 4, 5)
        assert lib.sfh_bgzf_read_index(src.ctypes.data, src.size, C.byref(info), moff.ctypes.data, ooff.ctypes.data, m) == -2, name
        assert np.all(moff == 7) and np.all(ooff == 7) and info.members == m, name
        assert lib.sfh_bgzf_read_index(src.ctypes.data, src.size, C.byref(info), moff.ctypes.data, ooff.ctypes.data, m + 1) == 0, name
        assert (info.total_n, info.members, info.has_eof, info.status) == (len(data), m, int(eof), 0), name
        assert [int(v) for v in moff[: m + 1]] == want_m and [int(v) for v in ooff[: m + 1]] == want_o and moff[m + 1] == 7, name
        # the Python spelling, against the pure-Python walker
        pm, po, pinfo = starflate_amd.bgzf_index(blob)
        wm, wo, widest, weof = BZ.walk(blob)
        assert ([int(v) for v in pm], [int(v) for v in po]) == (wm, wo), name
        assert pinfo == {"total_n": len(data), "members": m, "max_isize": widest, "has_eof": weof}, name
        assert gzip.decompress(blob) == data, name
    for name, bad, want in BZ.damaged():
        src = np.frombuffer(bad, np.uint8)
        info = _capi.BgzfInfo(1, 2, 3, 4, 0)
        moff = np.full(64, 7, np.uint64)
        assert lib.sfh_bgzf_read_index(src.ctypes.data, src.size, C.byref(info), moff.ctypes.data, moff.ctypes.data + 256, 32) == 0, name
        assert (info.total_n, info.members, info.max_isize, info.has_eof, info.status) == (0, 0, 0, 0, want) and np.all(moff == 7), name
        with pytest.raises(starflate_amd.StarflateError) as e:
            starflate_amd.bgzf_index(bad)
        assert e.value.code == want, name
    m, o, info = starflate_amd.bgzf_index(b"")
    assert list(m) == [0] and list(o) == [0] and info == {"total_n": 0, "members": 0, "max_isize": 0, "has_eof": False}
