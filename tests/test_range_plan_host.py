"""The random-access planner (starflate_amd/csrc/sf_range_plan.h: ranges -> decode spans, write windows, strips, launch
batches) compiled for the host with every warning an error and checked against a brute-force model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from range_cases import edge_ranges, random_ranges

SEG = 32768
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = tmp_path_factory.mktemp("sfr") / "libsfr.so"
    subprocess.check_call([CLANG, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "range_plan_host.cpp"), "-o", str(so)])
    L = C.CDLL(str(so))
    u64p = C.POINTER(C.c_uint64)
    L.sfr_plan.argtypes = [C.c_uint64, C.c_uint32, C.c_size_t, u64p, u64p, C.c_uint32, u64p]
    L.sfr_plan.restype = C.c_int
    L.sfr_read.argtypes = [C.c_void_p] * 4
    L.sfr_read.restype = None
    return L


def plan(L, total_n, block_bytes, ranges, cap):
    k = len(ranges)
    offs = (C.c_uint64 * max(k, 1))(*[r[0] for r in ranges])
    lens = (C.c_uint64 * max(k, 1))(*[r[1] for r in ranges])
    counts = (C.c_uint64 * 5)()
    rc = L.sfr_plan(total_n, block_bytes, k, offs, lens, cap, counts)
    if rc:
        return rc, None
    rows = np.zeros((counts[0], 7), np.uint64)
    spans = np.zeros((counts[1], 3), np.uint64)
    strips = np.zeros((counts[2], 2), np.uint64)
    batches = np.zeros((counts[3], 4), np.uint64)
    L.sfr_read(rows.ctypes.data, spans.ctypes.data, strips.ctypes.data, batches.ctypes.data)
    return 0, dict(rows=rows.astype(np.int64), spans=spans.astype(np.int64), strips=strips.astype(np.int64),
                   batches=batches.astype(np.int64), widest=int(counts[4]))


def check(P, total_n, block_bytes, ranges, cap):
    """the brute-force model: every property, range by range and row by row"""
    sps = (block_bytes or SEG) // SEG
    rows, spans, strips, batches = P["rows"], P["spans"], P["strips"], P["batches"]
    assert len(spans) == len(ranges)
    at = 0
    for r, (off, ln) in enumerate(ranges):
        first, row0, nrows = (int(v) for v in spans[r])
        assert row0 == at  # the spans' rows follow each other
        if ln == 0:
            assert nrows == 0
            continue
        # the decode span starts on a strip start and ends with the range's last segment
        want_first = off // SEG // sps * sps
        want_last = (off + ln - 1) // SEG
        assert first == want_first and first % sps == 0
        assert nrows == want_last - want_first + 1
        covered = []  # the bytes of the output the windows cover, in row order
        dst_at = 0
        for k in range(nrows):
            seg, dst_off, rng_, out_n, hist, lo, hi = (int(v) for v in rows[row0 + k])
            assert seg == first + k and rng_ == r
            assert out_n == min(SEG, total_n - seg * SEG) and out_n > 0
            assert hist == (seg % sps) * SEG
            assert lo <= hi <= out_n
            if lo < hi:
                assert dst_off == dst_at  # contiguous in the destination
                covered.append((seg * SEG + lo, seg * SEG + hi))
                dst_at += hi - lo
        assert rows[row0 + nrows - 1][0] == want_last
        # the union of the windows is exactly the range
        assert covered and covered[0][0] == off and covered[-1][1] == off + ln and dst_at == ln
        for a, b in zip(covered, covered[1:]):
            assert a[1] == b[0]
        at += nrows
    assert at == len(rows)
    # launch batches: consecutive, of whole strips, under the cap except for a single strip that alone is larger
    r_at = s_at = 0
    widest = 0
    for row0, nrows, strip0, nstrips in (tuple(int(v) for v in b) for b in batches):
        assert row0 == r_at and strip0 == s_at and nrows > 0 and nstrips > 0
        in_batch = 0
        for s0, sn in (tuple(int(v) for v in s) for s in strips[strip0: strip0 + nstrips]):
            assert s0 == in_batch and 0 < sn <= sps
            srows = rows[row0 + s0: row0 + s0 + sn]
            # one range, one strip of the stream, in order, the first row with as much history as its place in the strip says
            assert len(set(int(v) for v in srows[:, 2])) == 1
            assert len(set(int(v) // sps for v in srows[:, 0])) == 1
            assert [int(v) for v in srows[:, 0]] == list(range(int(srows[0][0]), int(srows[0][0]) + sn))
            assert int(srows[0][0]) % sps == 0 and int(srows[0][4]) == 0
            in_batch += sn
        assert in_batch == nrows
        assert nrows <= cap or nstrips == 1
        widest = max(widest, nrows)
        r_at += nrows
        s_at += nstrips
    assert r_at == len(rows) and s_at == len(strips) and widest == P["widest"]


CASES = [(0, 0), (1, 0), (32767, 32768), (32768, 0), (32769, 65536), (100000, 32768), (100000, 65536), (262144, 262144),
         (262144 * 3 + 12345, 262144), (1 << 20, 1 << 20), ((1 << 21) + 7, 1 << 20), (655360 + 5, 131072)]


@pytest.mark.parametrize("total_n, block_bytes", CASES)
def test_plan_edges_and_random(planner, total_n, block_bytes):
    rng = np.random.default_rng(total_n + block_bytes)
    ranges = edge_ranges(total_n, block_bytes) + random_ranges(rng, total_n, 200)
    sps = (block_bytes or SEG) // SEG
    for cap in (1 << 15, 1, 2, sps, sps + 1, 7, 64):  # caps smaller than one decode span among them
        rc, P = plan(planner, total_n, block_bytes, ranges, cap)
        assert rc == 0
        check(P, total_n, block_bytes, ranges, cap)
    # the ranges one by one: a span of its own is what a call with that range alone plans
    for r in ranges[:: max(1, len(ranges) // 60)]:
        rc, P = plan(planner, total_n, block_bytes, [r], 1 << 15)
        assert rc == 0
        check(P, total_n, block_bytes, [r], 1 << 15)


def test_plan_random_geometry(planner):
    rng = np.random.default_rng(20260)
    for _ in range(150):
        block_bytes = int(rng.choice([0, 32768, 65536, 98304, 262144, 1 << 20]))
        total_n = int(rng.integers(0, 6 * (block_bytes or SEG) + 3))
        if rng.integers(0, 3) == 0:
            total_n = total_n // SEG * SEG
        ranges = random_ranges(rng, total_n, int(rng.integers(0, 40)), max_len=2 * (block_bytes or SEG) + 100)
        if total_n:
            ranges += edge_ranges(total_n, block_bytes)[:: 7]
        cap = int(rng.integers(1, 80))
        rc, P = plan(planner, total_n, block_bytes, ranges, cap)
        assert rc == 0
        check(P, total_n, block_bytes, ranges, cap)


def test_plan_refusals(planner):
    assert plan(planner, 1000, 1000, [(0, 1)], 8)[0] == -1       # block_bytes not a multiple of 32768
    assert plan(planner, 1000, 0, [(999, 2)], 8)[0] == -1        # behind total_n
    assert plan(planner, 1000, 0, [(1001, 0)], 8)[0] == -1
    assert plan(planner, 1000, 0, [((1 << 64) - 1, 2)], 8)[0] == -1  # overflowing
    assert plan(planner, 1000, 0, [(0, 1)], 0)[0] == -1          # no cap
    # decode spans of more than 2^31 - 1 segments: refused before anything is allocated
    big = 1 << 44
    assert plan(planner, big, 0, [(0, big)] * 17, 1 << 15)[0] == -2
