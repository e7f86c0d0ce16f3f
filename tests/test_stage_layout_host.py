"""Where the batched host-buffer entry points put their items, compiled for the host with every warning an error: the packed
layout (starflate_amd/csrc/sf_stage_plan.h: pack_layout, the one place the 16-byte rounding is written) and the piece of the
stream that sfh_decompress_ranges uploads for a decode span (sf_range_plan.h: source_piece).  Both are checked against the
arithmetic the entry points used when each wrote it out by hand, restated here.  Carve (sf_stage_plan.h) is how the C-ABI lays
several arrays out in one scratch buffer: every piece starts at a multiple of 16, and the totals the library reports
(sfh_last_stream_stats, sfh_last_decode_scratch_bytes) are what the chained al16 sums gave before it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("sfl") / "libsfl.so"
    subprocess.check_call([CLANG, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "stage_layout_host.cpp"), "-o", str(so)])
    L = C.CDLL(str(so))
    L.sfl_pack_layout.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    L.sfl_pack_layout.restype = None
    L.sfl_source_piece.argtypes = [C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.sfl_source_piece.restype = None
    L.sfl_carve.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.sfl_carve.restype = C.c_uint64
    L.sfl_carve_at.argtypes = [C.c_uint64]
    L.sfl_carve_at.restype = C.c_uint64
    L.sfl_stream_scratch.argtypes = [C.c_uint64, C.c_void_p]
    L.sfl_stream_scratch.restype = None
    return L


def pack_layout(L, lens):
    slot = np.asarray(list(lens) or [0], np.uint64)
    off = np.full(len(lens) + 2, 0xDEAD, np.uint64)  # (+1: a guard word behind off[count])
    L.sfl_pack_layout(slot.ctypes.data, len(lens), off.ctypes.data)
    assert off[len(lens) + 1] == 0xDEAD
    return [int(v) for v in off[: len(lens) + 1]]


LAYOUTS = {
    "no items": [],
    "one item": [100],
    "one empty item": [0],
    "an empty item at the front": [0, 5, 40],
    "an empty item in the middle": [5, 0, 40],
    "an empty item at the end": [5, 40, 0],
    "empty items everywhere": [0, 0, 7, 0, 0, 33, 0, 0],
    "lengths around the alignment": [1, 15, 16, 17, 32769],
    "lengths around the alignment, reversed": [32769, 17, 16, 15, 1],
    "each length alone": None,  # (below)
    "compress bounds": [165, 33000, 100400],  # slots that are no aligned sizes: sfh_compress_batch's are a bound apart
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layout_is_the_entry_points_arithmetic(lib, name):
    cases = [[n] for n in (1, 15, 16, 17, 32769)] if LAYOUTS[name] is None else [LAYOUTS[name]]
    for lens in cases:
        off = pack_layout(lib, lens)
        # what every entry point wrote out: in_off[i + 1] = (in_off[i] + n[i] + 15) / 16 * 16
        want = [0]
        for n in lens:
            want.append((want[-1] + n + 15) // 16 * 16)
        assert off == want
        assert len(off) == len(lens) + 1 and off[0] == 0
        assert all(o % 16 == 0 for o in off)
        for i, n in enumerate(lens):  # ascending, and item i's bytes end before item i + 1's begin
            assert off[i] <= off[i] + n <= off[i + 1]
            assert off[i + 1] - (off[i] + n) < 16  # no more than the alignment is left between two items


def test_random_layouts(lib):
    rng = np.random.default_rng(7)
    for _ in range(200):
        lens = [int(rng.choice([0, 1, 15, 16, 17, 32769, int(rng.integers(0, 1 << 20))])) for _ in range(int(rng.integers(0, 20)))]
        off = pack_layout(lib, lens)
        at = 0
        for i, n in enumerate(lens):
            assert off[i] == at and at % 16 == 0
            at = (at + n + 15) // 16 * 16
        assert off[len(lens)] == at


def source_piece(L, first_seg, nrows, index, src_n):
    ix = np.asarray(index, np.uint64)
    out = np.zeros(2, np.uint64)
    L.sfl_source_piece(first_seg, nrows, ix.ctypes.data, src_n, out.ctypes.data)
    return int(out[0]), int(out[1])


# name: (index, src_n, [(first_seg, nrows), ...])
PIECES = {
    "an intact index": ([0, 1000, 2017, 3333, 4096, 5001], 5001, [(0, 5), (0, 1), (1, 3), (4, 1), (2, 2)]),
    "an intact index behind a header": ([10, 1000, 2017, 3333], 3341, [(0, 3), (1, 2), (2, 1)]),
    "entries that are not monotone": ([0, 3000, 1000, 2000, 500, 4000], 4000, [(0, 5), (1, 2), (1, 3), (2, 3)]),
    "an entry above src_n": ([0, 1000, 1 << 40, 3000, 5000], 3500, [(0, 4), (1, 1), (1, 2), (2, 2), (3, 1)]),
    "every entry above src_n": ([9000, 9500, 10000], 100, [(0, 2), (1, 1)]),
    "src_n no multiple of 16": ([0, 50, 99], 99, [(0, 2), (1, 1)]),
    "nrows == 0": ([0, 1000, 2000], 2000, [(0, 0), (1, 0), (2, 0)]),
    "an empty stream": ([0, 0], 0, [(0, 1), (0, 0)]),
}


@pytest.mark.parametrize("name", list(PIECES))
def test_source_piece(lib, name):
    index, src_n, spans = PIECES[name]
    for first, nrows in spans:
        lo, n = source_piece(lib, first, nrows, index, src_n)
        # inside the stream, from a 16-byte multiple on
        assert lo % 16 == 0 and 0 <= lo <= lo + n <= src_n
        # every entry of the span that lies inside the stream is covered (one at src_n is the end of the piece)
        entries = index[first: first + nrows + 1] if nrows else []
        for e in entries:
            if e <= src_n:
                assert lo <= e <= lo + n
        # ... and it is what sfh_decompress_ranges computed by hand
        w_lo = w_hi = 0
        if nrows:
            w_lo, w_hi = min(entries), max(entries)
        w_lo = min(w_lo, src_n) // 16 * 16
        w_hi = min(src_n, (min(w_hi, src_n) + 15) // 16 * 16)
        assert (lo, n) == (w_lo, w_hi - w_lo)
        if nrows == 0:
            assert (lo, n) == (0, 0)


def al16(b):
    return (b + 15) // 16 * 16


def carve(L, pieces):
    esize = np.asarray([e for e, _ in pieces] or [1], np.uint32)
    count = np.asarray([c for _, c in pieces] or [0], np.uint64)
    off = np.full(len(pieces) + 1, 0xDEAD, np.uint64)  # (+1: a guard word)
    total = L.sfl_carve(esize.ctypes.data, count.ctypes.data, len(pieces), off.ctypes.data)
    assert off[len(pieces)] == 0xDEAD and total != 2**64 - 1
    return [int(v) for v in off[: len(pieces)]], int(total)


# (element size, count) per piece: every element size the shim has a type for, counts 0 and 1 among them
CARVES = {
    "nothing": [],
    "one byte": [(1, 1)],
    "one empty piece": [(8, 0)],
    "every size once": [(1, 1), (2, 1), (4, 1), (8, 1), (12, 1), (72, 1)],
    "every size, odd counts": [(72, 3), (1, 17), (12, 5), (2, 9), (8, 3), (4, 1000), (1, 0), (4, 7)],
    "empty pieces everywhere": [(4, 0), (1, 5), (8, 0), (8, 0), (12, 1), (2, 0)],
    "aligned already": [(8, 2), (4, 4), (1, 16), (72, 2), (12, 4)],
    "bytes around the alignment": [(1, 15), (1, 16), (1, 17), (1, 32769), (2, 1)],
}


@pytest.mark.parametrize("name", list(CARVES))
def test_carve_pieces_are_aligned_disjoint_and_in_order(lib, name):
    pieces = CARVES[name]
    off, total = carve(lib, pieces)
    at = 0  # what chaining al16 by hand gives: o_next = al16(o + bytes of the piece)
    for (esize, count), o in zip(pieces, off):
        assert o % 16 == 0
        assert o == at  # in order, and behind the piece before it: disjoint
        at = al16(o + esize * count)
    assert total == at and total % 16 == 0
    if pieces:
        assert total >= off[-1] + pieces[-1][0] * pieces[-1][1]  # bytes() covers the last piece
    else:
        assert total == 0


def test_carve_random(lib):
    rng = np.random.default_rng(11)
    for _ in range(200):
        pieces = [(int(rng.choice([1, 2, 4, 8, 12, 72])), int(rng.choice([0, 1, int(rng.integers(0, 5000))]))) for _ in range(int(rng.integers(0, 12)))]
        off, total = carve(lib, pieces)
        at = 0
        for (esize, count), o in zip(pieces, off):
            assert o == at and o % 16 == 0
            at = al16(o + esize * count)
        assert total == at


def test_carve_at_is_base_plus_offset(lib):
    for o in (0, 16, 48):
        assert lib.sfl_carve_at(o) == o


@pytest.mark.parametrize("nc", [1, 2, 1000])
def test_stream_scratch_total_is_the_chained_sum(lib, nc):
    """cand | recs | list of the stream driver: the total it reports (sfh_last_stream_stats count 5, less the plane and windows)
    is what al16(8 nc) + al16(sizeof(StreamChunk) nc) + al16(4 nc) was when the driver chained the offsets by hand."""
    out = np.zeros(5, np.uint64)
    lib.sfl_stream_scratch(nc, out.ctypes.data)
    o_cand, o_rec, o_list, total, rec = (int(v) for v in out)
    assert rec == 48  # sf_stream_chain.h
    assert (o_cand, o_rec, o_list) == (0, al16(8 * nc), al16(8 * nc) + al16(rec * nc))
    assert total == al16(8 * nc) + al16(rec * nc) + al16(4 * nc)
