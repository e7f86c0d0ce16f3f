"""ctypes access to tests/cpp/stream_host.cpp (built once per session into a temporary directory): the block-start predicate
for the host, and the serial decoder of include/starflate/container.hpp.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix="sfs"), "libsfs.so")
        subprocess.check_call([CLANG, "-O2", "-std=c++23", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                               "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "stream_host.cpp"),
                               "-o", so])
        L = C.CDLL(so)
        L.sfs_scan.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
        L.sfs_scan.restype = C.c_uint64
        L.sfs_serial.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_int64)]
        L.sfs_serial.restype = C.c_uint32
        L.sfs_chain_round.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        L.sfs_chain_round.restype = C.c_uint32
        _LIB = L
    return _LIB


def _padded(data):
    buf = np.zeros(len(data) + 8, np.uint8)
    buf[: len(data)] = np.frombuffer(bytes(data), np.uint8)
    return buf


def scan(data, lo=0, hi=None):
    """bit offsets of data where the strict dynamic-header predicate holds"""
    buf = _padded(data)
    hi = 8 * len(data) if hi is None else hi
    cap = 1 << 16
    hits = np.zeros(cap, np.uint64)
    k = lib().sfs_scan(buf.ctypes.data, len(data), lo, hi, hits.ctypes.data, cap)
    assert k <= cap
    return [int(h) for h in hits[:k]]


CONTAINERS = {"raw": 0, "zlib": 1, "gzip": 2}


def serial(stream, container, cap):
    """container.hpp's decompress(stream, dst[cap], container) -> (status, bytes written: raw / gzip the body's, zlib None, dst)"""
    buf = _padded(stream)
    dst = np.zeros(max(cap, 1), np.uint8)
    w = C.c_int64(0)
    st = lib().sfs_serial(buf.ctypes.data if len(stream) else None, len(stream), CONTAINERS[container], dst.ctypes.data, cap,
                          C.byref(w))
    return st, (None if w.value < 0 else w.value), dst[:cap]


# sf::StreamChunk (starflate_amd/csrc/sf_stream_chain.h)
CHUNK = np.dtype([("start", "<u8"), ("limit", "<u8"), ("end", "<u8"), ("out", "<u8"), ("base", "<u8"), ("status", "<u4"),
                  ("final", "<u4")])
assert CHUNK.itemsize == 48


def chain_round(rec):
    """sf::stream_chain_round, the library's own, on a CHUNK array (updated in place) -> (redo list, confirmed chunks)"""
    redo = np.zeros(max(len(rec), 1), np.uint32)
    chain = C.c_uint32(0)
    k = lib().sfs_chain_round(rec.ctypes.data, len(rec), redo.ctypes.data, C.byref(chain))
    return [int(x) for x in redo[:k]], chain.value
