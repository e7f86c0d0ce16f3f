"""decode_segment (starflate_amd/csrc/sf_inflate_core.h) on segments above 32 KiB of output -- the indexed decoder's wide rows --
compiled for the host (tests/cpp/inflate_core_wide_host.cpp, every warning an error): bodies of 32769, 65280 and 65536
bytes in every block shape, and hand-made ones with the matches a 32 KiB segment never sees (tests/bgzf_wide_cases.py),
against zlib's output.  The same cases run once more through the stand-alone program built with AddressSanitizer + UBSan,
body, tokens and output each in a heap allocation of its own size.  And the wide-row arithmetic of sf_bgzf_plan.h."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_files as BZ
import bgzf_wide_cases as K
from conftest import ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "inflate_core_wide_host.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
INVALID_DISTANCE = 7


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    so = tmp_path_factory.mktemp("sfiw") / "libsfiw.so"
    subprocess.check_call([CLANG, "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", str(so)])
    L = C.CDLL(str(so))
    L.sfiw_decode.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    L.sfiw_decode.restype = C.c_uint32
    L.sfiw_wide_batch.argtypes = [C.c_uint32]
    L.sfiw_wide_batch.restype = C.c_uint32
    L.sfiw_checksum_rows.argtypes = [C.c_uint64, C.c_int]
    L.sfiw_checksum_rows.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def cases():
    """[(name, body, out_n, status wanted, bytes wanted or None)]"""
    out = []
    for n in (32769, K.WIDE, 65536):
        txt = BZ.text(n, seed=n % 7)
        out.append((f"text {n}", K.zlib_body(txt), n, 0, txt))
        out.append((f"nibbles {n}", K.zlib_body(K.nibbles(n, n)), n, 0, K.nibbles(n, n)))
    for name, (payload, body) in K.shape_cases().items():
        out.append((name, body, len(payload), 0, payload))
    for name, (payload, body) in K.far_cases().items():
        out.append((name, body, len(payload), 0, payload))
    body, claims = K.invalid_distance()
    out.append(("distance 101 at position 100", body, claims, INVALID_DISTANCE, None))
    for name, body, n, st, want in out:
        assert st or zlib.decompress(body, -15) == want, name
    return out


def test_wide_segments_against_zlib(core, cases):
    assert len(cases) >= 17
    for name, body, n, want_st, want in cases:
        src = np.frombuffer(body, np.uint8)
        out = np.full(n + 16, 0xA5, np.uint8)
        st = core.sfiw_decode(src.ctypes.data, src.size, n, out.ctypes.data)
        assert st == want_st, name
        if st == 0:
            assert out[:n].tobytes() == want, name
        assert np.all(out[n:] == 0xA5), name


def test_a_segment_promised_one_byte_more_or_less(core, cases):
    """the row's size is the member's ISIZE: a body that holds more is DstTooSmall (4), one that holds less SrcTooSmall (5)"""
    name, body, n, _, _ = cases[2]
    assert n == K.WIDE
    src = np.frombuffer(body, np.uint8)
    out = np.zeros(n + 16, np.uint8)
    assert core.sfiw_decode(src.ctypes.data, src.size, n - 1, out.ctypes.data) == 4
    assert core.sfiw_decode(src.ctypes.data, src.size, n + 1, out.ctypes.data) == 5


def test_wide_row_arithmetic(core):
    """a wide member's tokens take twice a narrow one's scratch: half as many members per launch batch, one at least; two
    checksum rows per member"""
    for per, want in ((32768, 16384), (4, 2), (5, 2), (2, 1), (1, 1)):
        assert core.sfiw_wide_batch(per) == want
        assert want * 65536 <= max(per, 2) * 32768  # the token scratch keeps its bound
    for m in (0, 1, 9, 2**31 - 1):
        assert core.sfiw_checksum_rows(m, 0) == m and core.sfiw_checksum_rows(m, 1) == 2 * m


def test_same_cases_under_asan_ubsan(cases, tmp_path):
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for _, body, n, st, want in cases:
            f.write(struct.pack("<QII", len(body), n, st) + body + (want if st == 0 else b""))
    exe = tmp_path / "inflate_core_wide_host"
    subprocess.check_call([CLANG, "-O1", "-g"] + WARN + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", str(exe)])
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == f"{len(cases)} cases"
    for (name, _, _, st, _), line in zip(cases, lines):
        assert line == f"{st} {int(st == 0)}", name
