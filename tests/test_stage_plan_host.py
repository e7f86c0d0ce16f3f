"""The staging loops of the batched host-buffer entry points (starflate_amd/csrc/sf_stage_plan.h: a packed layout moved through
one pinned buffer, piece by piece) compiled for the host with every warning an error and run with a tiny piece size, so that
items straddle piece boundaries -- in the library a piece is 64 MiB, and no other test pushes more than one piece through.
Packing up and unpacking down are checked byte by byte against a plain model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def stager(tmp_path_factory):
    so = tmp_path_factory.mktemp("sfg") / "libsfg.so"
    subprocess.check_call([CLANG, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "stage_plan_host.cpp"), "-o", str(so)])
    L = C.CDLL(str(so))
    v, u = C.c_void_p, C.c_uint64
    L.sfg_pack_up.argtypes = [u, u, v, v, v, v, u, v, v, u]
    L.sfg_pack_up.restype = u
    L.sfg_unpack_down.argtypes = [u, u, v, v, v, u, v, v, v, u]
    L.sfg_unpack_down.restype = u
    L.sfg_failing_transfer.argtypes = [u, v, u, u, C.POINTER(u)]
    L.sfg_failing_transfer.restype = C.c_int
    return L


def layout(lens, align):
    """packed offsets as the entry points lay items out: each item `align` bytes aligned -> (off[count], total)"""
    off, at = [], 0
    for n in lens:
        off.append(at)
        at = (at + n + align - 1) // align * align
    return off, at


def u64(a):
    return np.asarray(list(a) or [0], np.uint64)


def pieces(total, piece):
    return [(p0, min(piece, total - p0)) for p0 in range(0, total, piece)]


def roundtrip(L, piece, lens, align, skip=()):
    """up then down through pieces of `piece` bytes; skip: the items unpacked with length 0 (failed items)"""
    rng = np.random.default_rng(len(lens) * 1000 + piece)
    count = len(lens)
    off, total = layout(lens, align)
    item_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    items = rng.integers(1, 255, int(item_off[-1]) + 1, dtype=np.uint8)
    dev = np.full(total + 1, 0xAA, np.uint8)  # (+1: a guard byte behind the layout)
    cap = total // piece + 2
    copied = np.zeros(2 * cap, np.uint64)
    ln, of = u64(lens), u64(off)
    k = L.sfg_pack_up(piece, count, items.ctypes.data, item_off.ctypes.data, ln.ctypes.data, of.ctypes.data, total,
                      dev.ctypes.data, copied.ctypes.data, cap)
    # up: every piece of the layout goes up once, in order, and every item's bytes lie at its packed offset
    assert [tuple(int(x) for x in copied[2 * j: 2 * j + 2]) for j in range(k)] == pieces(total, piece)
    assert dev[total] == 0xAA
    for i in range(count):
        a = int(item_off[i])
        assert dev[off[i]: off[i] + lens[i]].tobytes() == items[a: a + lens[i]].tobytes(), i
    # down: the reference, byte by byte
    got = [0 if i in skip else lens[i] for i in range(count)]
    want = np.full(len(items), 0x55, np.uint8)
    touched = set()
    for i in range(count):
        for b in range(got[i]):
            want[int(item_off[i]) + b] = dev[off[i] + b]
            touched.add((off[i] + b) // piece)
    out = np.full(len(items), 0x55, np.uint8)
    gn = u64(got)
    k = L.sfg_unpack_down(piece, count, dev.ctypes.data, gn.ctypes.data, of.ctypes.data, total, out.ctypes.data,
                          item_off.ctypes.data, copied.ctypes.data, cap)
    assert out.tobytes() == want.tobytes()
    # only the pieces that hold a byte of an item that is not skipped come down, each once, in order
    assert [int(copied[2 * j]) for j in range(k)] == [p0 for p0, _ in pieces(total, piece) if p0 // piece in touched]
    for j in range(k):
        assert int(copied[2 * j + 1]) == min(piece, total - int(copied[2 * j]))
    if not skip:
        assert out[:-1].tobytes() == items[:-1].tobytes()


CASES = {
    "one item inside one piece": (64, [40], 16),
    "an item straddling one boundary": (64, [40, 40], 16),            # the second item: [48, 88)
    "an item straddling several boundaries": (32, [10, 150, 7], 16),  # the middle item: [16, 166), pieces 0..5
    "an item ending exactly on a boundary": (64, [64, 30], 16),
    "an item ending on a boundary after a gap": (64, [20, 32, 5], 16),  # the second item: [32, 64)
    "items of exactly one piece": (48, [48, 48, 48], 16),
    "empty items": (32, [0, 20, 0, 0, 50, 0], 16),
    "only empty items": (32, [0, 0, 0], 16),
    "an empty item on a boundary": (32, [32, 0, 32], 16),
    "many small items per piece": (64, [3, 1, 0, 7, 16, 2, 9, 30, 1, 1], 16),
    "unaligned layout": (16, [5, 17, 0, 33, 16, 1], 1),
    "a piece of one byte": (1, [3, 0, 2], 1),
}


@pytest.mark.parametrize("name", list(CASES))
def test_pack_and_unpack_match_the_model(stager, name):
    piece, lens, align = CASES[name]
    roundtrip(stager, piece, lens, align)


@pytest.mark.parametrize("name", list(CASES))
def test_skipped_items_are_left_alone(stager, name):
    """failed items (length 0 on the way down): nothing is written to them, and a piece that holds only their bytes is not
    fetched"""
    piece, lens, align = CASES[name]
    for skip in ({0}, {len(lens) - 1}, set(range(0, len(lens), 2)), set(range(len(lens)))):
        roundtrip(stager, piece, lens, align, skip)


@pytest.mark.parametrize("seed", range(30))
def test_random_layouts(stager, seed):
    rng = np.random.default_rng(seed)
    piece = int(rng.choice([1, 7, 16, 32, 100]))
    lens = [int(rng.choice([0, 1, piece, 2 * piece, int(rng.integers(0, 4 * piece + 1))])) for _ in range(int(rng.integers(1, 25)))]
    skip = {i for i in range(len(lens)) if rng.random() < 0.3}
    roundtrip(stager, piece, lens, int(rng.choice([1, 16])), skip)


def test_a_failing_transfer_stops_the_loop(stager):
    item = np.arange(100, dtype=np.uint8)
    n = C.c_uint64(0)
    assert stager.sfg_failing_transfer(16, item.ctypes.data, 100, 3, C.byref(n)) == -7
    assert n.value == 3
    assert stager.sfg_failing_transfer(16, item.ctypes.data, 100, 99, C.byref(n)) == 0
    assert n.value == 7
