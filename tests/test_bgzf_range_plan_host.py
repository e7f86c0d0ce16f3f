"""The BGZF random-access planner (starflate_amd/csrc/sf_bgzf_range_plan.h: ranges -> the members of their decode spans, write
windows, launch batches) compiled for the host with every warning an error and checked against a brute-force model that
walks the members one by one.  The same enumeration runs once more in a stand-alone program built with AddressSanitizer +
UBSan, every index in a heap allocation of exactly its size: a read past members + 1 entries is a report there."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "bgzf_range_plan_host.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
LISTS = [[0, 1, 100, 32768, 31, 0], [65280, 65280, 7, 65536, 0, 0, 5], [0, 0, 0, 0], [777], [65536], [0], []]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = tmp_path_factory.mktemp("sfbr") / "libsfbr.so"
    subprocess.check_call([CLANG, "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", str(so)])
    L = C.CDLL(str(so))
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.sfbr_digest.argtypes = [vp, u32]
    L.sfbr_digest.restype = u64
    L.sfbr_span.argtypes = [vp, u32, u64, u64, vp]
    L.sfbr_row.argtypes = [vp, u32, u32, u64, u64, vp]
    L.sfbr_batches.argtypes = [u64, u32, C.c_int, vp, u64]
    L.sfbr_piece.argtypes = [vp, u32, u32, u64, vp]
    for f in (L.sfbr_span, L.sfbr_row, L.sfbr_batches, L.sfbr_piece):
        f.restype = None
    return L


def offsets_of(out_off):
    total = out_off[-1]
    return sorted({o + d for o in out_off for d in (-1, 0, 1) if 0 <= o + d <= total})


def model_span(sizes, off, ln):
    """member by member: the members that hold a byte of the range, and the empty ones between them"""
    if ln == 0:
        return 0, 0
    at, holds = 0, []
    for i, n in enumerate(sizes):
        if at < off + ln and at + n > off:
            holds.append(i)
        at += n
    return holds[0], holds[-1] - holds[0] + 1


@pytest.mark.parametrize("sizes", LISTS, ids=[str(s) for s in LISTS])
def test_span_row_and_batches_against_the_model(planner, sizes):
    m = len(sizes)
    out_off = np.concatenate([[0], np.cumsum(sizes, dtype=np.uint64)]).astype(np.uint64)
    oo = [int(v) for v in out_off]
    total = oo[-1]
    span, row = np.zeros(3, np.uint64), np.zeros(5, np.uint64)
    for off in offsets_of(oo):
        for ln in sorted({0, 1, 3, 4, 5, total - off}):
            if ln > total - off:
                continue
            planner.sfbr_span(out_off.ctypes.data, m, off, ln, span.ctypes.data)
            first, rows, inside = (int(v) for v in span)
            want_first, want_rows = model_span(sizes, off, ln)
            assert inside == 1 and rows == want_rows and (rows == 0 or first == want_first), (off, ln)
            if rows:
                # the issue's two rules, literally
                assert first == min(i for i in range(m) if oo[i + 1] > off)
                assert first + rows - 1 == min(j for j in range(m) if oo[j + 1] >= off + ln)
            covered, dst_at = [], 0
            for k in range(rows):
                planner.sfbr_row(out_off.ctypes.data, first, k, off, ln, row.ctypes.data)
                member, out_n, lo, hi, dst_off = (int(v) for v in row)
                assert member == first + k and out_n == sizes[member] and lo <= hi <= out_n
                if sizes[member] == 0:
                    assert lo == hi  # an empty member inside the span: a row that writes nothing
                if lo < hi:
                    assert dst_off == dst_at  # contiguous in the destination
                    covered.append((oo[member] + lo, oo[member] + hi))
                    dst_at += hi - lo
            if rows:
                # the first and the last row hold bytes of the range, and the windows' union is exactly the range
                assert covered[0][0] == off and covered[-1][1] == off + ln and dst_at == ln
                assert all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
            for bc in (1, 2, 3):
                for wide in (0, 1):
                    out = np.zeros(2 + rows + 1, np.uint64)
                    planner.sfbr_batches(rows, bc, wide, out.ctypes.data, rows + 1)
                    per = max(1, bc // 2) if wide else bc
                    assert int(out[0]) == per and int(out[1]) == -(-rows // per)
                    got = [int(v) for v in out[2: 2 + int(out[1])]]
                    assert sum(got) == rows and all(0 < g <= per for g in got) and all(g == per for g in got[:-1])
    # behind the output: no rows, and said so
    planner.sfbr_span(out_off.ctypes.data, m, total, 1, span.ctypes.data)
    assert (int(span[1]), int(span[2])) == (0, 0)
    planner.sfbr_span(out_off.ctypes.data, m, total + 1, 0, span.ctypes.data)
    assert (int(span[1]), int(span[2])) == (0, 0)
    planner.sfbr_span(out_off.ctypes.data, m, (1 << 64) - 1, 2, span.ctypes.data)
    assert (int(span[1]), int(span[2])) == (0, 0)


def test_upload_piece(planner):
    moff = np.array([0, 100, 1000, 1030, 5000], np.uint64)
    out = np.zeros(2, np.uint64)
    for first, rows, src_n, want in ((0, 1, 5000, (0, 112)), (1, 2, 5000, (96, 1040 - 96)), (2, 2, 5000, (992, 5000 - 992)),
                                     (1, 0, 5000, (0, 0)), (2, 2, 1010, (992, 18)), (3, 1, 1000, (992, 8))):
        planner.sfbr_piece(moff.ctypes.data, first, rows, src_n, out.ctypes.data)
        lo, n = int(out[0]), int(out[1])
        assert (lo, n) == want and lo % 16 == 0 and lo + n <= src_n


def test_same_enumeration_under_asan_ubsan(planner, tmp_path):
    cases = tmp_path / "cases.bin"
    with open(cases, "wb") as f:
        for sizes in LISTS:
            f.write(struct.pack(f"<Q{len(sizes)}Q", len(sizes), *sizes))
    exe = tmp_path / "bgzf_range_plan_host"
    subprocess.check_call([CLANG, "-O1", "-g"] + WARN + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", str(exe)])
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == f"{len(LISTS)} lists"
    for sizes, line in zip(LISTS, lines):
        arr = np.array(sizes, np.uint64)
        assert int(line) == planner.sfbr_digest(arr.ctypes.data if arr.size else None, len(sizes)), sizes
