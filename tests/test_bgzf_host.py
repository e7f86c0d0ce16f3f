"""The BGZF member parser (starflate_amd/csrc/sf_bgzf_plan.h) compiled for the host with every warning an error and run on
files made with Python's zlib (tests/bgzf_files.py): the index must be what a pure-Python walker finds, every good file must
be a gzip file of its data, every damaged file must give the status include/starflate_hip.h states.  The same cases run
once more through a stand-alone program built with AddressSanitizer + UBSan, every case in a heap allocation of exactly its
size: a read past src_n is a report there."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bgzf_files as BZ
from conftest import ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "bgzf_index_host.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
DST_TOO_SMALL = -2
GUARD = 0xDEADBEEF


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    so = tmp_path_factory.mktemp("sfbgzf") / "libsfbgzf.so"
    subprocess.check_call([CLANG, "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", str(so)])
    L = C.CDLL(str(so))
    L.sfbgzf_read.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.sfbgzf_read.restype = None
    L.sfbgzf_bound.argtypes = [C.c_uint64]
    L.sfbgzf_bound.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def files():
    return BZ.good_files()


def read(L, blob, cap=4096):
    """-> (rc, status, members, max_isize, has_eof, total_n, member_off or None, out_off or None)"""
    src = np.frombuffer(blob, np.uint8)
    moff = np.full(cap + 1, GUARD, np.uint64)  # one guard entry behind the capacity
    ooff = np.full(cap + 1, GUARD, np.uint64)
    out = np.zeros(6, np.int64)
    L.sfbgzf_read(src.ctypes.data if src.size else None, src.size, moff.ctypes.data, ooff.ctypes.data, cap, out.ctypes.data)
    rc, st, m, widest, eof, total = (int(v) for v in out)
    assert moff[cap] == GUARD and ooff[cap] == GUARD
    if rc != 0 or st != 0:
        assert np.all(moff == GUARD) and np.all(ooff == GUARD), "nothing is written unless the call and the file succeed"
        return rc, st, m, widest, eof, total, None, None
    assert np.all(moff[m + 1:] == GUARD) and np.all(ooff[m + 1:] == GUARD)
    return rc, st, m, widest, eof, total, [int(v) for v in moff[: m + 1]], [int(v) for v in ooff[: m + 1]]


def test_good_files_give_the_walkers_index(reader, files):
    assert len(files) >= 9
    for name, (data, blob, want_m, want_o, want_eof) in files.items():
        assert gzip.decompress(blob) == data, name
        wm, wo, widest, eof = BZ.walk(blob)
        assert (wm, wo, eof) == (want_m, want_o, want_eof), name  # the walker against the writer
        rc, st, m, got_widest, got_eof, total, moff, ooff = read(reader, blob)
        assert (rc, st) == (0, 0), name
        assert (m, got_widest, got_eof, total) == (len(wm) - 1, widest, int(eof), len(data)), name
        assert moff == wm and ooff == wo and moff[m] == len(blob) and ooff[m] == len(data), name
        # cap one short of members + 1: refused, nothing written (the info carries the count)
        short = read(reader, blob, cap=m)
        assert short[:3] == (DST_TOO_SMALL, 0, m) and short[6] is None, name
        assert read(reader, blob, cap=m + 1)[6] == wm, name


def test_members_of_65280_bytes_and_fake_headers(reader, files):
    assert read(reader, files["65280-byte members"][1])[2:4] == (4, 65280)
    for name in BZ.fake_header_files():
        blob = files[name][1]
        assert read(reader, blob)[2] == 3, name  # two members and the EOF member: the fake head is nobody's successor
        assert blob.count(BZ.EOF[:16]) == 4, name


def test_empty_file(reader):
    assert read(reader, b"") == (0, 0, 0, 0, 0, 0, [0], [0])
    assert read(reader, b"", cap=0)[:3] == (DST_TOO_SMALL, 0, 0)
    assert read(reader, BZ.EOF)[2:6] == (1, 0, 1, 0)


def test_damaged_files(reader):
    cases = BZ.damaged()
    assert len(cases) >= 12
    for name, blob, want in cases:
        with pytest.raises(BZ.WalkError) as e:
            BZ.walk(blob)
        assert e.value.status == want, name  # the walker agrees with what the case is meant to be
        assert read(reader, blob) == (0, want, 0, 0, 0, 0, None, None), name


def test_every_truncation_of_a_good_file(reader, files):
    """a file cut anywhere ends in a status (5 unless the cut falls on a member's end), never in a read past its bytes"""
    data, blob, moff, _, _ = files["subfield before BC"]
    for cut in list(range(0, 60)) + list(range(len(blob) - 60, len(blob))) + moff:
        part = blob[:cut]
        try:
            wm, wo, widest, eof = BZ.walk(part)
            want = (0, 0, len(wm) - 1, widest, int(eof), wo[-1], wm, wo)
        except BZ.WalkError as e:
            want = (0, e.status, 0, 0, 0, 0, None, None)
        assert read(reader, part) == want, cut


def test_bound(reader):
    per = 32768 + 4096 + 640 + 26
    for n, members in ((0, 1), (1, 1), (32768, 1), (32769, 2), (3 * 32768 + 5, 4)):
        assert reader.sfbgzf_bound(n) == members * per + 28


def test_same_cases_under_asan_ubsan(reader, files, tmp_path):
    """the stand-alone program, every case in an allocation of exactly its size"""
    blobs = [f[1] for f in files.values()] + [b for _, b, _ in BZ.damaged()] + [b"", BZ.EOF]
    blob = files["sizes eof=True"][1]
    blobs += [blob[:cut] for cut in range(0, len(blob), 7)]
    cases = tmp_path / "cases.bin"
    with open(cases, "wb") as f:
        for b in blobs:
            f.write(struct.pack("<Q", len(b)) + b)
    exe = tmp_path / "bgzf_index_host"
    subprocess.check_call([CLANG, "-O1", "-g"] + WARN + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", str(exe)])
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == f"{len(blobs)} cases"
    for b, line in zip(blobs, lines):
        rc, st, m, widest, eof, total, moff, ooff = read(reader, b, cap=8192)
        assert [int(v) for v in line.split()] == [rc, st, m, widest, eof, total, sum(moff) + sum(ooff) if moff else 0]
