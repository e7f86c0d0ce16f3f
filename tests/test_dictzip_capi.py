"""CPU-side checks of the seekable-gzip entry points (SFH_DICTZIP, sfh_dz_*, sfh_decompress_dz*): exported, declared, listed,
their host arithmetic, the table reader through the library on a host-made file, and refusals before any device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import dictzip_files as DZ
import starflate_amd
from starflate_amd import _capi, build

NEW = ("sfh_dz_header_bytes", "sfh_compress_bound_container", "sfh_dz_read_index", "sfh_dz_read_index_device",
       "sfh_decompress_dz_device", "sfh_decompress_dz", "sfh_decompress_dz_ranges")
LIMIT = 32762 * 32768
DICTZIP = 3


def test_dictzip_symbols_exported_declared_listed():
    build.build()
    lib = _capi.lib()
    with open(os.path.join(os.path.dirname(build.PKG_DIR), "include", "starflate_hip.h")) as f:
        header = f.read()
    for s in NEW:
        assert s in _capi.EXPORTS and hasattr(lib, s)
        assert f"{s}(" in header
    assert "SFH_DICTZIP = 3" in header and "#define SFH_DZ_MAX_CHUNKS 32762u" in header
    assert _capi.COMPRESS_CONTAINER["dictzip"] == DICTZIP and "dictzip" not in _capi.CONTAINER  # the decoders keep refusing 3
    assert C.sizeof(_capi.DzInfo) == 24
    for name in ("dictzip_index", "decompress_dictzip", "read_ranges"):
        assert name in starflate_amd.__all__ and callable(getattr(starflate_amd, name))
    for name in ("decompress_dictzip", "read_ranges"):
        assert callable(getattr(starflate_amd.Compressor, name))
    assert _capi.make_options(container="dictzip").container == DICTZIP


def test_header_and_bound_arithmetic():
    lib = _capi.lib()
    for n, nseg in ((0, 1), (1, 1), (32768, 1), (32769, 2), (3 * 32768 + 5, 4), (2 << 20, 64), (LIMIT, 32762)):
        assert lib.sfh_dz_header_bytes(n) == 22 + 2 * nseg
        for bb in (0, 32768):
            # the gzip bound at 32 KiB strips plus what the header has beyond gzip's ten bytes
            assert lib.sfh_compress_bound_container(n, bb, DICTZIP) == lib.sfh_compress_bound(n, 32768) + 12 + 2 * nseg
        for bb in (65536, 262144, 1000):  # what the call would refuse
            assert lib.sfh_compress_bound_container(n, bb, DICTZIP) == 0
        for kind in (0, 1, 2):
            for bb in (0, 32768, 262144, 1000):
                assert lib.sfh_compress_bound_container(n, bb, kind) == lib.sfh_compress_bound(n, bb)
        assert lib.sfh_compress_bound_container(n, 0, 4) == 0
    assert lib.sfh_dz_header_bytes(LIMIT + 1) == 0 and lib.sfh_compress_bound_container(LIMIT + 1, 0, DICTZIP) == 0
    assert lib.sfh_dz_header_bytes(LIMIT) == 22 + 2 * 32762 and lib.sfh_compress_bound_container(LIMIT, 0, DICTZIP) != 0
    assert lib.sfh_compress_bound_container(LIMIT + 1, 0, 2) == lib.sfh_compress_bound(LIMIT + 1, 0)
    # what the Python compress calls size their buffers by
    assert starflate_amd.Compressor._bound(32769, "dictzip", 0) == lib.sfh_compress_bound(32769, 0) + 16
    assert starflate_amd.Compressor._bound(32769, "gzip", 65536) == lib.sfh_compress_bound(32769, 0)
    with pytest.raises(ValueError, match="dictzip"):
        starflate_amd.Compressor._bound(32769, "dictzip", 65536)
    with pytest.raises(ValueError, match="dictzip"):
        starflate_amd.Compressor._bound(LIMIT + 1, "dictzip", 0)


def test_refusals_with_a_null_context():
    lib = _capi.lib()
    buf = np.zeros(256, np.uint8)
    idx = np.zeros(8, np.uint64)
    info = _capi.DzInfo()
    n64, st = C.c_uint64(0), C.c_uint32(0)
    p = buf.ctypes.data
    assert lib.sfh_dz_read_index_device(None, p, 64, C.byref(info), idx.ctypes.data, 8, None) == -1
    assert lib.sfh_decompress_dz_device(None, p, 64, p + 128, 64, C.byref(n64), C.byref(st), None) == -1
    assert lib.sfh_decompress_dz(None, p, 64, p + 128, 64, C.byref(n64), C.byref(st)) == -1
    off, ln, dsts, sts = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(1), (C.c_void_p * 1)(p + 128), (C.c_uint32 * 1)()
    assert lib.sfh_decompress_dz_ranges(None, p, 64, 1, off, ln, dsts, sts) == -1
    assert lib.sfh_decompress_dz_ranges(None, p, 64, 0, None, None, None, None) == -1
    # the compress calls with SFH_DICTZIP and no context
    opt = _capi.make_options(container="dictzip")
    out_n = C.c_size_t(0)
    assert lib.sfh_compress(None, p, 64, p + 128, 128, C.byref(out_n), C.byref(opt)) == -1
    assert lib.sfh_compress_device(None, p, 64, p + 128, 128, C.byref(out_n), C.byref(opt), None) == -1
    assert lib.sfh_compress_device_async(None, p, 64, p + 128, 128, p, C.byref(opt), None) == -1
    # the host reader: null pointers
    assert lib.sfh_dz_read_index(p, 64, None, idx.ctypes.data, 8) == -1
    assert lib.sfh_dz_read_index(None, 64, C.byref(info), idx.ctypes.data, 8) == -1
    assert lib.sfh_dz_read_index(p, 64, C.byref(info), None, 8) == -1


def _read(blob, cap=None):
    lib = _capi.lib()
    src = np.frombuffer(blob, np.uint8)
    cap = _capi.DZ_MAX_CHUNKS + 1 if cap is None else cap
    idx = np.full(cap + 1, 7, np.uint64)
    info = _capi.DzInfo(1, 2, 3, 4, 5)
    rc = lib.sfh_dz_read_index(src.ctypes.data if src.size else None, src.size, C.byref(info), idx.ctypes.data, cap)
    return rc, info, idx


def test_read_index_through_the_library():
    for kw in (DZ.VARIANTS["inside"], DZ.VARIANTS["all"]):
        for n in DZ.SIZES:
            data = DZ.text(n, seed=n + 5)
            blob, want = DZ.write(data, **kw)
            rc, info, idx = _read(blob)
            nseg = max(1, -(-n // 32768))
            assert rc == 0 and (info.total_n, info.nseg, info.header_bytes, info.status, info.reserved) == (n, nseg, want[0], 0, 0)
            assert [int(v) for v in idx[: nseg + 1]] == want and np.all(idx[nseg + 1:] == 7)
            rc, info, idx = _read(blob, cap=nseg)  # one entry short: SFH_E_DST_TOO_SMALL, nothing written
            assert rc == -2 and np.all(idx == 7) and info.total_n == 1 and info.reserved == 5
            # the Python spelling
            index, total_n = starflate_amd.dictzip_index(blob)
            assert total_n == n and index.dtype == np.uint64 and [int(v) for v in index] == want
    blob, want = DZ.write(b"", chcnt0=True)
    rc, info, idx = _read(blob)
    assert rc == 0 and (info.total_n, info.nseg, info.status) == (0, 1, 0) and [int(v) for v in idx[:2]] == want
    # not a dictzip file of 32 KiB chunks: SFH_E_NOT_INDEXABLE, nothing written -- neither the index nor the info
    blob = DZ.write(DZ.text(70000, seed=2), chlen=58315)[0]
    rc, info, idx = _read(blob)
    assert rc == -8 and np.all(idx == 7) and (info.total_n, info.nseg, info.header_bytes, info.status, info.reserved) == (1, 2, 3, 4, 5)
    with pytest.raises(starflate_amd.StarflateError) as e:
        starflate_amd.dictzip_index(blob)
    assert e.value.code == -8
    # a header that does not parse: SFH_OK, the status in the info, the other fields 0, the index untouched
    for bad, st in ((blob[:17], 5), (b"\x1e" + blob[1:], 1)):
        rc, info, idx = _read(bad)
        assert rc == 0 and (info.total_n, info.nseg, info.header_bytes, info.status, info.reserved) == (0, 0, 0, st, 0) and np.all(idx == 7)
        with pytest.raises(starflate_amd.StarflateError) as e:
            starflate_amd.dictzip_index(bad)
        assert e.value.code == st


def test_python_checks_before_a_device():
    blob, _ = DZ.write(DZ.text(40000, seed=1))
    with pytest.raises(ValueError, match="does not lie inside"):
        starflate_amd.read_ranges(blob, [39999], [2])
    with pytest.raises(ValueError, match="offsets but"):
        starflate_amd.read_ranges(blob, [0, 1], [2])
    with pytest.raises(starflate_amd.StarflateError):
        starflate_amd.read_ranges(blob[:20], [0], [1])
    with pytest.raises(KeyError):
        _capi.make_options(container="dictzip2")
    # the decoders' container argument keeps refusing "dictzip"
    with pytest.raises(ValueError, match="container"):
        starflate_amd.decompress_stream_batch([blob], container="dictzip")
