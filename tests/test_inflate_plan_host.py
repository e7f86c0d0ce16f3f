"""The indexed decoder's cut into launch batches (starflate_amd/csrc/sf_inflate_plan.h: items -> segments, strips, launch
batches) compiled for the host with every warning an error and checked against a brute-force model.  It decides the geometry
of every indexed decode, a single stream's included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SEG = 32768
CLANG = "/opt/rocm/llvm/bin/clang++"
CAPS = (1, 2, 3, 4, 8, 32768)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = tmp_path_factory.mktemp("sfi") / "libsfi.so"
    subprocess.check_call([CLANG, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "inflate_plan_host.cpp"), "-o", str(so)])
    L = C.CDLL(str(so))
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.sfi_plan.argtypes = [C.c_size_t, u64p, u32p, C.c_uint32, u64p]
    L.sfi_plan.restype = None
    L.sfi_read.argtypes = [u64p, u32p] + [C.c_void_p] * 3
    L.sfi_read.restype = C.c_uint64
    return L


def nseg_of(n):
    return max(1, -(-n // SEG))


def plan(L, items, cap):
    k = len(items)
    dst_n = (C.c_uint64 * max(k, 1))(*[it[0] for it in items])
    bbs = (C.c_uint32 * max(k, 1))(*[it[1] for it in items])
    counts = (C.c_uint64 * 4)()
    L.sfi_plan(k, dst_n, bbs, cap, counts)
    rows = np.zeros((counts[0], 4), np.uint64)
    strips = np.zeros((counts[1], 2), np.uint64)
    batches = np.zeros((counts[2], 6), np.uint64)
    assert L.sfi_read(dst_n, bbs, rows.ctypes.data, strips.ctypes.data, batches.ctypes.data) == counts[0]
    return dict(rows=rows.astype(np.int64), strips=strips.astype(np.int64), batches=batches.astype(np.int64), widest=int(counts[3]))


def check(P, items, cap):
    rows, strips, batches = P["rows"], P["strips"], P["batches"]
    # every segment exactly once, in item order, with its size and history
    want = [(i, k) for i, (n, _) in enumerate(items) for k in range(nseg_of(n))]
    assert [(int(r[0]), int(r[1])) for r in rows] == want
    for i, k, out_n, hist in (tuple(int(v) for v in r) for r in rows):
        n, bb = items[i]
        sps = (bb or SEG) // SEG
        assert out_n == max(0, min(SEG, n - k * SEG)) and hist == (k % sps) * SEG
    assert len(strips) == sum(-(-nseg_of(n) // ((bb or SEG) // SEG)) for n, bb in items)
    # batches: consecutive in both tables, named by their first segment; strips: one item, one batch, whole strips of the item
    r_at = s_at = widest = 0
    for row0, nseg, strip0, nstrips, item0, k0 in (tuple(int(v) for v in b) for b in batches):
        assert (row0, strip0) == (r_at, s_at) and nseg > 0 and nstrips > 0
        assert (int(rows[row0][0]), int(rows[row0][1])) == (item0, k0)
        in_batch = 0
        for s0, sn in (tuple(int(v) for v in s) for s in strips[strip0: strip0 + nstrips]):
            assert s0 == in_batch and sn > 0
            srows = rows[row0 + s0: row0 + s0 + sn]
            assert len(srows) == sn  # (the strip ends inside its batch)
            i, first = int(srows[0][0]), int(srows[0][1])
            sps = (items[i][1] or SEG) // SEG
            assert first % sps == 0 and int(srows[0][3]) == 0
            assert [(int(r[0]), int(r[1])) for r in srows] == [(i, first + j) for j in range(sn)]
            assert sn == min(sps, nseg_of(items[i][0]) - first)  # a whole strip of the item: the cut does not change the strips
            in_batch += sn
        assert in_batch == nseg
        assert nseg <= cap or nstrips == 1
        widest = max(widest, nseg)
        r_at += nseg
        s_at += nstrips
    assert r_at == len(rows) and s_at == len(strips) and widest == P["widest"]


SIZES = (0, 1, SEG - 1, SEG, SEG + 1, 3 * SEG, 4 * SEG, 7 * SEG - 5, 8 * SEG, 9 * SEG + 777, 23 * SEG + 777, 70 * SEG + 1)
BLOCKS = (0, SEG, 2 * SEG, 3 * SEG, 4 * SEG, 8 * SEG, 16 * SEG)


@pytest.mark.parametrize("cap", CAPS)
def test_single_item_batches_are_the_strip_aligned_cut(planner, cap):
    """One item: batch = max(sps, cap / sps * sps) segments, starting at 0, batch, 2 * batch, ... -- the cut of the single call
    before it became a batch of one."""
    for n in SIZES:
        for bb in BLOCKS:
            P = plan(planner, [(n, bb)], cap)
            check(P, [(n, bb)], cap)
            sps = (bb or SEG) // SEG
            batch = max(sps, cap // sps * sps)
            nseg = nseg_of(n)
            want = [(g0, min(batch, nseg - g0)) for g0 in range(0, nseg, batch)]
            assert [(int(b[0]), int(b[1])) for b in P["batches"]] == want, (n, bb)
            assert P["widest"] == min(nseg, batch)


@pytest.mark.parametrize("cap", CAPS)
def test_item_lists(planner, cap):
    rng = np.random.default_rng(cap)
    lists = [[], [(0, 0)] * 5, [(n, 4 * SEG) for n in SIZES], [(n, bb) for n in SIZES[:8] for bb in BLOCKS],
             [(4096, 0)] * 100, [(70000, 262144), (200000, 262144), (100000, 262144), (50000, 262144), (300000, 32768), (1000, 262144)]]
    for _ in range(40):
        lists.append([(int(rng.choice(SIZES)) if rng.integers(0, 2) else int(rng.integers(0, 40 * SEG)), int(rng.choice(BLOCKS)))
                      for _ in range(int(rng.integers(1, 12)))])
    for items in lists:
        check(plan(planner, items, cap), items, cap)


def test_small_items_share_batches_and_large_ones_stand_alone(planner):
    # three segments fit a batch of four together with one more; the item of nine is cut at its strips, into batches of its own
    P = plan(planner, [(3 * SEG, 0), (SEG, 0), (2 * SEG, 0), (9 * SEG, 2 * SEG), (SEG, 0)], 4)
    assert [(int(b[0]), int(b[1])) for b in P["batches"]] == [(0, 4), (4, 2), (6, 4), (10, 4), (14, 1), (15, 1)]
    # a strip larger than the cap is a batch of its own
    P = plan(planner, [(SEG, 0), (5 * SEG, 4 * SEG), (SEG, 0)], 2)
    assert [(int(b[1]), int(b[3])) for b in P["batches"]] == [(1, 1), (4, 1), (1, 1), (1, 1)]
