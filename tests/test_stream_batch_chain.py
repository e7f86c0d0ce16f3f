"""The per-item chain round (sf_stream_chain.h) that the batched stream decoder runs over each item's slice of one record
array: on random record sets, concatenated items give exactly the records and redo lists of the one-stream round run on each
item alone (tests/cpp/stream_batch_chain.cpp, compiled for the host as stream_host.py builds its own)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import stream_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix="sfb"), "libsfb.so")
        subprocess.check_call([H.CLANG, "-O2", "-std=c++23", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                               os.path.join(ROOT, "tests", "cpp", "stream_batch_chain.cpp"), "-o", so])
        L = C.CDLL(so)
        L.sfb_chain_round_slice.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        L.sfb_chain_round_slice.restype = C.c_uint32
        L.sfb_chain_round_vector.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        L.sfb_chain_round_vector.restype = C.c_uint32
        _LIB = L
    return _LIB


def _records(rng, m):
    """a random set of decoded records: starts ascending, limits the next start, ends near them, some failed, some final"""
    rec = np.zeros(m, H.CHUNK)
    starts = np.sort(rng.choice(np.arange(1, 40 * m + 2), m - 1, replace=False)) if m > 1 else np.zeros(0, np.int64)
    rec["start"] = np.concatenate([[0], starts])
    rec["limit"][:-1] = rec["start"][1:]
    rec["limit"][-1] = (1 << 64) - 1
    for i in range(m):
        lim = int(rec["limit"][i]) if i + 1 < m else int(rec["start"][i]) + 50
        r = rng.random()
        rec["end"][i] = lim if r < 0.6 else lim + int(rng.integers(1, 30)) if r < 0.85 else max(int(rec["start"][i]), lim - int(rng.integers(1, 5)))
        rec["out"][i] = int(rng.integers(0, 5000))
        rec["status"][i] = 0 if rng.random() < 0.9 else int(rng.integers(1, 8))
        rec["final"][i] = 1 if rng.random() < 0.05 or i + 1 == m else 0
    return rec


@pytest.mark.parametrize("seed", range(40))
def test_slices_match_items_alone(seed):
    rng = np.random.default_rng(seed)
    items = [_records(rng, int(rng.integers(1, 60))) for _ in range(int(rng.integers(1, 12)))]
    alone = []
    for rec in items:
        r = rec.copy()
        redo = np.zeros(len(r), np.uint32)
        chain = C.c_uint32(0)
        k = lib().sfb_chain_round_vector(r.ctypes.data, len(r), redo.ctypes.data, C.byref(chain))
        alone.append((r, [int(x) for x in redo[:k]], chain.value))
    cat = np.concatenate(items)
    redo = np.zeros(len(cat), np.uint32)
    r0 = 0
    for rec, (want, want_redo, want_chain) in zip(items, alone):
        chain = C.c_uint32(0)
        k = lib().sfb_chain_round_slice(cat.ctypes.data, r0, len(rec), redo.ctypes.data, C.byref(chain))
        assert [int(x) - r0 for x in redo[:k]] == want_redo
        assert chain.value == want_chain
        assert cat[r0: r0 + len(rec)].tobytes() == want.tobytes()
        r0 += len(rec)


def test_vector_overload_is_the_library_round():
    """the shim's one-stream round is stream_host.chain_round's (tests/cpp/stream_host.cpp), record for record"""
    rng = np.random.default_rng(99)
    for _ in range(20):
        rec = _records(rng, int(rng.integers(1, 80)))
        a, b = rec.copy(), rec.copy()
        want = H.chain_round(a)
        redo = np.zeros(len(b), np.uint32)
        chain = C.c_uint32(0)
        k = lib().sfb_chain_round_vector(b.ctypes.data, len(b), redo.ctypes.data, C.byref(chain))
        assert ([int(x) for x in redo[:k]], chain.value) == want
        assert a.tobytes() == b.tobytes()
