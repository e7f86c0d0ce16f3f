"""ctypes access to tests/cpp/members_host.cpp (built once per session into a temporary directory): the specification of
Container::GzipMembers (include/starflate/container.hpp), and sf_members.h's steps walked against it.  sanitizer_program()
builds the same file as a stand-alone program under AddressSanitizer and UBSan.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
SOURCE = os.path.join(ROOT, "tests", "cpp", "members_host.cpp")
COMMON = ["-std=c++23", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
_LIB = None
_DIR = None

# starflate::GzipMember
MEMBER = np.dtype([("src_end", "<u8"), ("out_end", "<u8"), ("crc32", "<u4"), ("isize", "<u4")])
assert MEMBER.itemsize == 24


def _dir():
    global _DIR
    if _DIR is None:
        _DIR = tempfile.mkdtemp(prefix="sfm")
    return _DIR


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_dir(), "libsfm.so")
        subprocess.check_call([CLANG, "-O2", "-shared", "-fPIC"] + COMMON + [SOURCE, "-o", so])
        L = C.CDLL(so)
        L.sfm_members.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64,
                                  C.POINTER(C.c_uint64)]
        L.sfm_members.restype = C.c_uint32
        L.sfm_agree.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
        L.sfm_agree.restype = C.c_int
        L.sfm_head_candidates.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
        L.sfm_head_candidates.restype = C.c_uint64
        _LIB = L
    return _LIB


def _buf(data):
    return np.frombuffer(bytes(data) or b"\0", np.uint8).copy()


def spec(blob, cap):
    """decompress_members(blob, dst[cap]) -> (status, output bytes on status 0 else None, MEMBER rows of the members that passed)"""
    src, dst = _buf(blob), np.zeros(max(cap, 1), np.uint8)
    produced, nrec = C.c_uint64(0), C.c_uint64(0)
    recs = np.zeros(4096, MEMBER)
    st = lib().sfm_members(src.ctypes.data, len(blob), dst.ctypes.data, cap, C.byref(produced), recs.ctypes.data, len(recs),
                           C.byref(nrec))
    assert nrec.value <= len(recs)
    return st, (dst[: produced.value].tobytes() if st == 0 else None), recs[: nrec.value]


def agree(blob, cap):
    """0, or the line of members_host.cpp at which sf_members.h's walk left the specification's"""
    src = _buf(blob)
    return lib().sfm_agree(src.ctypes.data, len(blob), cap)


def head_candidates(blob, lo=0, hi=None):
    src = _buf(blob)
    hits = np.zeros(1 << 12, np.uint64)
    k = lib().sfm_head_candidates(src.ctypes.data, len(blob), lo, len(blob) if hi is None else hi, hits.ctypes.data, len(hits))
    assert k <= len(hits)
    return [int(h) for h in hits[:k]]


def sanitizer_program():
    """members_host.cpp with its own main under -fsanitize=address,undefined -> the program's path"""
    exe = os.path.join(_dir(), "members_host_san")
    if not os.path.exists(exe):
        subprocess.check_call([CLANG, "-O1", "-g", "-DSFM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + COMMON +
                              [SOURCE, "-o", exe])
    return exe
