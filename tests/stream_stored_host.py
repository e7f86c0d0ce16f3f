"""ctypes access to tests/cpp/stream_stored_host.cpp (built once per session into a temporary directory): the stored-block
start predicate for the host, and its closed form in Python.  TEST INFRASTRUCTURE ONLY."""
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
        so = os.path.join(tempfile.mkdtemp(prefix="sfss"), "libsfss.so")
        subprocess.check_call([CLANG, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                               os.path.join(ROOT, "tests", "cpp", "stream_stored_host.cpp"), "-o", so])
        L = C.CDLL(so)
        L.sfss_scan.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
        L.sfss_scan.restype = C.c_uint64
        _LIB = L
    return _LIB


def scan(data, lo=0, hi=None, min_len=0, look=False):
    """bit offsets of the body `data` where the stored-block start predicate holds, every offset tried.  look: only the hits
    k_stream_find takes, those with a stored header behind the payload (stored_run_follows); min_len: only those with LEN >=
    min_len (for counting; the library has no such filter)"""
    data = bytes(data)
    buf = np.full(len(data) + 8, 0xA5, np.uint8)  # (nothing behind the body may matter)
    buf[: len(data)] = np.frombuffer(data, np.uint8)
    hi = 8 * len(data) if hi is None else hi
    cap = 1 << 16
    hits = np.zeros(cap, np.uint64)
    k = lib().sfss_scan(buf.ctypes.data, len(data), lo, hi, hits.ctypes.data, cap, min_len, int(look))
    assert k <= cap
    return [int(h) for h in hits[:k]]


def closed_form(data):
    """{8(B-1) + bit_length(body[B-1])} over the LEN bytes B with body[B-1] < 32, LEN ^ NLEN == 0xFFFF and B + 4 + LEN <= n"""
    a = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    n = a.size
    if n < 5:
        return []
    b = np.arange(1, n - 3)  # B + 4 <= n
    ln = a[b] | (a[b + 1] << 8)
    nl = a[b + 2] | (a[b + 3] << 8)
    ok = (a[b - 1] < 32) & ((ln ^ nl) == 0xFFFF) & (b + 4 + ln <= n)
    return [8 * (int(B) - 1) + int(a[B - 1]).bit_length() for B in b[ok]]


def stored_starts(blocks):
    """the non-final stored blocks of deflate_writer.inflate's block list -> [(start bit, LEN byte B)]"""
    return [(b["start"], (b["start"] + 3 + 7) // 8) for b in blocks if b["type"] == 0 and not b.get("final")]
