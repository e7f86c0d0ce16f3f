"""The dictzip table reader (starflate_amd/csrc/sf_dz_plan.h) compiled for the host with every warning an error and run on
files made by a Python dictzip writer (tests/dictzip_files.py): the index must be the writer's own offsets, every damaged
header must give the outcome include/starflate_hip.h states, and so must every truncation of a good file below its header
size.  The same cases run once more through a stand-alone program built with AddressSanitizer + UBSan, every case in a heap
allocation of exactly its size: a read past src_n is a report there."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import dictzip_files as DZ
from conftest import ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "dz_index_host.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
NOT_INDEXABLE, DST_TOO_SMALL = -8, -2
ERROR, SRC_TOO_SMALL = 1, 5


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    so = tmp_path_factory.mktemp("sfdz") / "libsfdz.so"
    subprocess.check_call([CLANG, "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", str(so)])
    L = C.CDLL(str(so))
    L.sfdz_read.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    L.sfdz_read.restype = None
    L.sfdz_header_bytes.argtypes = [C.c_uint64]
    L.sfdz_header_bytes.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def files():
    return DZ.good_files()


def read(L, blob, cap=32763):
    """-> (rc, status, nseg, header_bytes, total_n, index or None)"""
    src = np.frombuffer(blob, np.uint8)
    index = np.full(cap + 1, 0xDEADBEEF, np.uint64)  # one guard entry behind the capacity
    out = np.zeros(5, np.int64)
    L.sfdz_read(src.ctypes.data if src.size else None, src.size, index.ctypes.data, cap, out.ctypes.data)
    rc, st, nseg, hdr, total = (int(v) for v in out)
    assert index[cap] == 0xDEADBEEF
    if rc != 0 or st != 0:
        assert np.all(index == 0xDEADBEEF), "nothing is written unless the call and the header succeed"
        return rc, st, nseg, hdr, total, None
    assert np.all(index[nseg + 1:] == 0xDEADBEEF)
    return rc, st, nseg, hdr, total, [int(v) for v in index[: nseg + 1]]


def test_good_files_give_the_writers_offsets(reader, files):
    assert len(files) == 6 * 6 * 2 + 1
    for name, (data, blob, want) in files.items():
        rc, st, nseg, hdr, total, index = read(reader, blob)
        assert (rc, st) == (0, 0), name
        assert total == len(data) and nseg == max(1, -(-len(data) // 32768)), name
        assert index == want and hdr == want[0] and index[nseg] == len(blob) - 8, name
        assert zlib.decompress(blob, wbits=31) == data, name  # (the writer writes gzip)
        # every segment of the index inflates alone to its 32 KiB: the dictzip contract, with the reader's last entry
        for k in range(nseg):
            got = zlib.decompressobj(-15).decompress(blob[index[k]: index[k + 1]])
            assert got == data[k * 32768: (k + 1) * 32768], (name, k)
        # index_cap one short of nseg + 1: refused, nothing written
        assert read(reader, blob, cap=nseg)[:2] == (DST_TOO_SMALL, 0), name
        assert read(reader, blob, cap=nseg + 1)[5] == want, name


def test_header_bytes_arithmetic(reader):
    for n, nseg in ((0, 1), (1, 1), (32768, 1), (32769, 2), (3 * 32768 + 5, 4), (32762 * 32768, 32762)):
        assert reader.sfdz_header_bytes(n) == 22 + 2 * nseg
    assert reader.sfdz_header_bytes(32762 * 32768 + 1) == 0


def patched(blob, at, new):
    return blob[:at] + new + blob[at + len(new):]


def damaged():
    """(name, file, expected (rc, status)) for every outcome the header states"""
    data = DZ.text(32769 + 100, seed=9)
    good, index = DZ.write(data)  # gzip 10 | XLEN | 'R' 'A' LEN | VER CHLEN CHCNT | 2 sizes
    assert index[0] == 26 and good[12:14] == b"RA"
    out = [
        ("no FEXTRA", gzip.compress(data, mtime=0), (NOT_INDEXABLE, 0)),
        ("no RA subfield", patched(good, 12, b"RB"), (NOT_INDEXABLE, 0)),
        ("VER 2", patched(good, 16, struct.pack("<H", 2)), (NOT_INDEXABLE, 0)),
        ("CHLEN 58315", DZ.write(data, chlen=58315)[0], (NOT_INDEXABLE, 0)),
        ("CHLEN 16384", DZ.write(data, chlen=16384)[0], (NOT_INDEXABLE, 0)),
        ("empty", b"", (0, SRC_TOO_SMALL)),
        ("17 bytes", good[:17], (0, SRC_TOO_SMALL)),
        ("file name without its end", DZ.write(b"ab", fname=b"name")[0][:27] + DZ.write(b"ab", fname=b"name")[0][-8:], (0, SRC_TOO_SMALL)),
        ("bad magic", patched(good, 0, b"\x1e"), (0, ERROR)),
        ("bad CM", patched(good, 2, b"\x07"), (0, ERROR)),
        ("reserved flag", patched(good, 3, b"\x24"), (0, ERROR)),
        ("LEN short of its sizes", patched(good, 20, struct.pack("<H", 3)), (0, ERROR)),  # CHCNT 3, LEN 6 + 2 * 2
        ("LEN below 6", DZ.write(data, before=None)[0][:14] + struct.pack("<H", 4) + good[16:], (0, ERROR)),
        ("a subfield overrunning XLEN", patched(good, 14, struct.pack("<H", 6 + 2 * 2 + 2)), (0, ERROR)),
        ("XLEN overrunning the file", patched(good, 10, struct.pack("<H", 0xFFFF)), (0, ERROR)),
        ("CHCNT against ISIZE", good[:-4] + struct.pack("<I", len(data) + 32768), (0, ERROR)),
        ("CHCNT 0 with ISIZE 1", DZ.write(b"", chcnt0=True)[0][:-4] + struct.pack("<I", 1), (0, ERROR)),
        ("sizes past the trailer", patched(good, 22, struct.pack("<H", 0xFFFF)), (0, ERROR)),
        ("body cut short", good[:index[0] + 10] + good[-8:], (0, ERROR)),
    ]
    return out


def test_damaged_headers(reader):
    for name, blob, want in damaged():
        got = read(reader, blob)
        assert got[:2] == want, name
        assert got[2:] == (0, 0, 0, None), name


def truncations():
    """(file cut to L bytes, expected status) for every L below the header size of a plain file and of one with everything"""
    out = []
    for kw in (dict(), DZ.VARIANTS["all"]):
        for n in (1, 32769):
            blob, index = DZ.write(DZ.text(n, seed=3), **kw)
            xend = 12 + struct.unpack("<H", blob[10:12])[0]  # the extra field's end; the header's: index[0]
            for L in range(index[0]):
                # below a gzip member's 18 bytes: SrcTooSmall; the extra field not in front of the trailer: Error (XLEN
                # overruns); the file name or comment not in front of it: SrcTooSmall
                out.append((blob[:L], SRC_TOO_SMALL if L < 18 else ERROR if L - 8 < xend else SRC_TOO_SMALL))
    return out


def test_truncated_headers(reader):
    cuts = truncations()
    assert len(cuts) > 150
    for blob, want in cuts:
        assert read(reader, blob) == (0, want, 0, 0, 0, None), len(blob)


def test_same_cases_under_asan_ubsan(reader, files, tmp_path):
    """the stand-alone program, every case in an allocation of exactly its size"""
    blobs = [f for _, f, _ in files.values()] + [b for _, b, _ in damaged()] + [b for b, _ in truncations()]
    cases = tmp_path / "cases.bin"
    with open(cases, "wb") as f:
        for b in blobs:
            f.write(struct.pack("<Q", len(b)) + b)
    exe = tmp_path / "dz_index_host"
    subprocess.check_call([CLANG, "-O1", "-g"] + WARN + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", str(exe)])
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == f"{len(blobs)} cases"
    for b, line in zip(blobs, lines):
        rc, st, nseg, hdr, total, index = read(reader, b)
        assert [int(v) for v in line.split()] == [rc, st, nseg, hdr, total, sum(index) if index else 0]
