"""CPU-side checks of the ZIP entry points (sfh_zip_*, sfh_compress_zip*, sfh_decompress_zip*): exported, declared, listed and
bound in Python; sfh_zip_bound's arithmetic; the host walk through the library on Python-made archives and on the damage
catalogue; refusals that need no device."""
import ctypes as C
import io
import os
import zipfile

import numpy as np

import starflate_amd
import zip_files as Z
from starflate_amd import _capi, build

NEW = ("sfh_zip_read_index", "sfh_zip_read_index_device", "sfh_decompress_zip_device", "sfh_decompress_zip", "sfh_zip_bound",
       "sfh_compress_zip_device_async", "sfh_compress_zip_device", "sfh_compress_zip")


def test_zip_symbols_exported_declared_listed():
    build.build()
    lib = _capi.lib()
    with open(os.path.join(os.path.dirname(build.PKG_DIR), "include", "starflate_hip.h")) as f:
        header = f.read()
    for s in NEW:
        assert s in _capi.EXPORTS and hasattr(lib, s)
        assert f"{s}(" in header
    assert "typedef struct sfh_zip_info" in header and "typedef struct sfh_zip_entry" in header
    assert "#define SFH_ZIP_ENTRY_UNSUPPORTED 0xFFFFFFF9u" in header
    assert C.sizeof(_capi.ZipInfo) == 40 and C.sizeof(_capi.ZipEntry) == 64 == starflate_amd.ZIP_ENTRY_DTYPE.itemsize == Z.ENTRY_BYTES
    assert [n for n, _ in _capi.ZipEntry._fields_] == list(starflate_amd.ZIP_ENTRY_DTYPE.names) == list(Z.ENTRY_DTYPE.names)
    for name in ("compress_zip", "decompress_zip", "zip_index", "zip_bound"):
        assert name in starflate_amd.__all__ and callable(getattr(starflate_amd, name))
    for name in ("compress_zip", "compress_zip_tensors", "zip_index_tensor", "decompress_zip", "decompress_zip_tensors"):
        assert callable(getattr(starflate_amd.Compressor, name))
    assert "sf_zip.hip" in build.SOURCES and any(h.endswith("sf_zip_plan.h") for h in build.HEADERS)


def test_bound_arithmetic():
    lib = _capi.lib()
    for sizes, lens in (([], []), ([0], [1]), ([1, 32768, 32769, 3 * 32768 + 5], [1, 17, 255, 65535]), ([7] * 300, [5] * 300)):
        want = sum(30 + k + lib.sfh_compress_bound(n, 0) for n, k in zip(sizes, lens)) + sum(46 + k for k in lens) + 22 + 76
        assert starflate_amd.zip_bound(sizes, lens) == want == Z.zip_bound(sizes, lens)
    assert starflate_amd.zip_bound([], []) == 98
    assert lib.sfh_zip_bound(1, None, None) == 0


def test_bound_on_the_class_is_the_function():
    """Compressor.zip_bound (a static method: no context) on the smallest items and on a batch of them"""
    lib = _capi.lib()
    for sizes, lens in (([0], [1]), ([1], [1]), ([32769], [3]), ([0, 1, 32769], [1, 2, 3])):
        want = sum(30 + k + lib.sfh_compress_bound(n, 0) for n, k in zip(sizes, lens)) + sum(46 + k for k in lens) + 22 + 76
        assert starflate_amd.Compressor.zip_bound(sizes, lens) == want == starflate_amd.zip_bound(sizes, lens)


def test_host_walk_through_the_library():
    for name, blob in Z.foreign_archives().items():
        info, ents = starflate_amd.zip_index(blob)
        zf = zipfile.ZipFile(io.BytesIO(blob))
        assert info["status"] == 0 and info["entries"] == len(zf.infolist()), name
        assert starflate_amd.zip_names(blob, ents) == [zi.orig_filename for zi in zf.infolist()]
        st, winfo, went = Z.walk(blob)
        assert {k: info[k] for k in winfo} == winfo
        for k in ("data_off", "csize", "usize", "out_off", "crc32", "status"):
            assert [int(v) for v in ents[k]] == [w[k] for w in went], (name, k)
    for name, (blob, want_index, want_entries) in Z.damage_catalogue().items():
        info, ents = starflate_amd.zip_index(blob)
        assert info["status"] == want_index, name
        assert {i: int(s) for i, s in enumerate(ents["status"]) if s} == want_entries, name


def test_counts_come_with_dst_too_small():
    lib = _capi.lib()
    blob = Z.foreign_archives()["levels"]
    info = _capi.ZipInfo()
    ents = np.zeros(4, Z.ENTRY_DTYPE)
    assert lib.sfh_zip_read_index(blob, len(blob), C.byref(info), ents.ctypes.data, 3) == -2
    assert (info.entries, info.status) == (4, 0) and info.total_out > 0 and not ents.view(np.uint8).any()
    assert lib.sfh_zip_read_index(blob, len(blob), C.byref(info), ents.ctypes.data, 4) == 0 and ents["csize"].all()


def test_refusals_with_a_null_context_or_null_pointers():
    lib = _capi.lib()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    info = _capi.ZipInfo()
    ents = np.zeros(2, Z.ENTRY_DTYPE)
    st, out_n = (C.c_uint32 * 2)(), C.c_size_t(0)
    ptrs, sizes, caps = (C.c_void_p * 1)(p), (C.c_uint64 * 1)(64), (C.c_uint64 * 1)(64)
    names, lens = (C.c_char_p * 1)(b"a"), (C.c_uint32 * 1)(1)
    opt = _capi.make_options()
    assert lib.sfh_zip_read_index(p, 64, None, ents.ctypes.data, 2) == -1
    assert lib.sfh_zip_read_index(None, 64, C.byref(info), ents.ctypes.data, 2) == -1
    assert lib.sfh_zip_read_index(p, 64, C.byref(info), None, 2) == -1
    assert lib.sfh_zip_read_index(None, 0, C.byref(info), None, 0) == 0 and info.status == 5
    assert lib.sfh_zip_read_index_device(None, p, 64, C.byref(info), ents.ctypes.data, 2, None) == -1
    assert lib.sfh_decompress_zip_device(None, p, 64, ents.ctypes.data, 1, ptrs, caps, st, None) == -1
    assert lib.sfh_decompress_zip(None, p, 64, ents.ctypes.data, 1, ptrs, caps, st) == -1
    assert lib.sfh_compress_zip_device_async(None, 1, ptrs, sizes, names, lens, p + 1024, 3000, p, C.byref(opt), None) == -1
    assert lib.sfh_compress_zip_device(None, 1, ptrs, sizes, names, lens, p + 1024, 3000, C.byref(out_n), C.byref(opt), None) == -1
    assert lib.sfh_compress_zip(None, 1, ptrs, sizes, names, lens, p + 1024, 3000, C.byref(out_n), C.byref(opt)) == -1
    assert not buf.any()


def test_python_argument_checks_need_no_device():
    names, srcs = starflate_amd.compressor._zip_items({"a": b"x", "b": np.arange(3, dtype=np.uint8)})
    assert names == [b"a", b"b"] and [s.tobytes() for s in srcs] == [b"x", b"\0\1\2"]
    names, _ = starflate_amd.compressor._zip_items([("grüße", b""), (b"raw", b"")])
    assert names == ["grüße".encode("utf-8"), b"raw"]
