"""One status per malformation class on the indexed decoder's core (starflate_amd/csrc/sf_inflate_core.h, compiled for the
host): every class of tests/malformed_cases.py in every placement, and one stream cut at every byte, must get the status
the rule of malformed_cases.py states -- the serial decoder's (container.hpp compiled for the host, the judge) on the
segment's own bytes -- whatever lies behind the segment's last byte.  The oracle's restatement of the reference decoder
(sfo_decompress) must agree with the judge on all of them.  (The GPU kernels: tests/test_gpu_malformed.py.)"""
import ctypes as C
import os
import subprocess
import zlib
from collections import Counter

import numpy as np
import pytest

import malformed_cases as M
import oracle_lib as O
import stream_host as S
from conftest import ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
ROW = 65536


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    so = tmp_path_factory.mktemp("sfm") / "libsfi.so"
    subprocess.check_call([CLANG, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "inflate_core_host.cpp"), "-o", str(so)])
    L = C.CDLL(str(so))
    L.sfi_decode_segment_ex.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.sfi_decode_segment_ex.restype = C.c_uint32
    L.sfi_decode_segment_sub.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.sfi_decode_segment_sub.restype = C.c_uint32
    L.sfi_expand_tokens.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.sfi_expand_tokens.restype = C.c_longlong
    return L


@pytest.fixture(scope="module")
def cases():
    return M.class_cases()


@pytest.fixture(scope="module")
def judged(cases):
    """the rule's answer for every case, computed once: name -> (status, judge's status, bytes written, output)"""
    return {c.name: M.rule(S.serial, c.segment(), c.out_n, c.boundary) for c in cases}


def decode(L, buf, lo, hi, out_n, hist=0, exact=0):
    """the core on bytes [lo, hi) of buf (every byte of buf is readable, none behind it is) -> (status, bytes or None)"""
    n = len(buf)
    mem = np.zeros(n + 3 if n else 4, np.uint8)  # the reader loads whole dwords; src_n bounds them
    mem[:n] = buf
    tok = np.zeros(ROW + 4, np.uint32)
    ntok, raw, raw_off = C.c_uint32(), C.c_uint32(), C.c_uint64()
    st = L.sfi_decode_segment_ex(mem.ctypes.data, n, lo, hi, out_n, hist, exact, tok.ctypes.data, C.byref(ntok), C.byref(raw),
                                 C.byref(raw_off))
    if st:
        return st, None
    if raw.value:
        return 0, mem[raw_off.value: raw_off.value + out_n].copy()
    if hist:
        return 0, None
    out = np.zeros(max(out_n, 1), np.uint8)
    assert L.sfi_expand_tokens(tok.ctypes.data, ntok.value, out.ctypes.data, out_n) == out_n
    return 0, out[:out_n]


def trailers(c):
    """the case's stream as it is, and its segment in front of other bytes: -> [(label, buffer, lo, hi)]"""
    rng = np.random.default_rng(7)
    seg = c.segment()
    out = [("own", c.stream, c.lo, c.hi)]
    gs, glo, ghi = M.gap_variant(c)
    out.append(("gap", gs, glo, ghi))
    for label, tail in (("zeros", np.zeros(80, np.uint8)), ("ones", np.full(80, 255, np.uint8)),
                        ("noise", rng.integers(0, 256, 80, dtype=np.uint8)), ("nothing", np.zeros(0, np.uint8))):
        out.append((label, np.concatenate([seg, tail]), 0, len(seg)))
    return out


def test_generator_covers_every_exit(cases, judged):
    """no class is missing, each hits the exit it was built for, the judge's statuses include each of 1 to 7, and zlib
    refuses what the judge refuses"""
    names = {c.cls for c in cases}
    assert {n for n, _, _ in M.CLASSES} <= names and {"two_errors", "two_segments", "empty", "boundary"} <= names
    for n, _, _ in M.CLASSES:
        assert {c.place for c in cases if c.cls == n} == {"a", "b", "c", "e"}, n
    seen = Counter()
    for c in cases:
        want, s, w, dst = judged[c.name]
        assert want == c.hint, (c.name, want, s, w)
        seen[s] += 1
        if c.boundary or not len(c.segment()):
            continue
        d = zlib.decompressobj(-15)
        try:
            d.decompress(c.segment().tobytes(), max(c.out_n, 1))
            z_ok = d.eof
        except zlib.error:
            z_ok = False
        if s != 0:
            assert not z_ok, c.name  # (incomplete codes included: zlib refuses their headers, M.ZLIB_KNOWN)
        elif want != 0:
            assert z_ok and w < c.out_n, c.name  # a good stream: only the index promised more
        else:
            assert c.cls in M.ACCEPTED and not z_ok, c.name  # the reference's HLIT / HDIST acceptances
            assert bytes(dst[:w]) == c.head, c.name
    assert set(range(1, 8)) <= set(seen), seen


def test_every_class_and_placement(core, cases, judged):
    bad = []
    for c in cases:
        want, s, w, dst = judged[c.name]
        got = {}
        for label, buf, lo, hi in trailers(c):
            st, out = decode(core, buf, lo, hi, c.out_n)
            got[label] = st
            if st == 0 and want == 0:
                assert np.array_equal(out, dst[:w]), (c.name, label)
        if set(got.values()) != {want}:
            bad.append((c.name, want, got))
    assert not bad, bad


def test_good_neighbours_decode(core, cases):
    for c in cases:
        for seg, want in c.good.items():
            st, out = decode(core, c.stream, c.idx[seg], c.idx[seg + 1], len(want))
            assert st == 0 and out.tobytes() == want, (c.name, seg)


def test_oracle_agrees_with_the_judge(cases, judged):
    s, out, cuts = M.sweep_cuts()
    for c in cases:
        if len(c.segment()):
            assert O.decompress(c.segment(), c.out_n)[:2] == judged[c.name][1:3], c.name
    for k in cuts:
        assert O.decompress(s[:k], len(out))[:2] == S.serial(s[:k], "raw", len(out))[:2], k


def test_truncation_sweep(core):
    """one stream of a dynamic, a fixed and a stored block cut at every byte, each cut in front of five trailers"""
    s, out, cuts = M.sweep_cuts()
    assert len(s) <= 300 and len(cuts) == len(s) - 1
    seen, bad = Counter(), []
    for k in cuts:
        want = M.rule(S.serial, s[:k], len(out))[0]
        seen[want] += 1
        got = {t: decode(core, M.with_trailer(s, k, t), 0, k, len(out))[0] for t in M.TRAILERS}
        if set(got.values()) != {want}:
            bad.append((k, want, got))
    assert {1, 6, 7} <= set(seen), seen
    assert not bad, (len(bad), bad[:20])
    st, got = decode(core, s, 0, len(s), len(out))
    assert st == 0 and got.tobytes() == out


def test_strips_reach_their_history(core):
    for name, strip, lo, hist, out_n, hint in M.strip_cases():
        s, w, _ = S.serial(strip, "raw", hist + out_n)
        assert s == hint, name
        assert decode(core, strip, lo, len(strip), out_n, hist=hist)[0] == s, name
        assert O.decompress(strip, hist + out_n)[0] == s, name


def test_exact_end_rule(core, cases, judged):
    """decode_segment<true> (a recovered index: the segment is not the stream's last): a segment whose blocks end on its last
    bit is fine, a final block stays Error, and a damaged segment gets the rule's status all the same"""
    by = {c.name: c for c in cases}
    c = by["boundary_full"]
    assert decode(core, c.stream, c.lo, c.hi, c.out_n, exact=1)[0] == 0
    g = by["btype3/e"]  # its last segment is good and ends with a final block
    assert decode(core, g.stream, g.idx[2], g.idx[3], len(g.good[2]))[0] == 0
    assert decode(core, g.stream, g.idx[2], g.idx[3], len(g.good[2]), exact=1)[0] == M.ERROR
    for c in cases:
        want = judged[c.name][0]
        if c.place == "a" and want != 0 and len(c.segment()):
            assert decode(core, c.stream, c.lo, c.hi, c.out_n, exact=1)[0] == want, c.name


def _sub(L, seg, out_n, sub):
    mem = np.zeros(len(seg) + 3, np.uint8)
    mem[: len(seg)] = seg
    tok = np.zeros(M.SEG + 4, np.uint32)
    ntok, raw, raw_off = C.c_uint32(), C.c_uint32(), C.c_uint64()
    sub = np.ascontiguousarray(sub, np.uint32)
    st = L.sfi_decode_segment_sub(mem.ctypes.data, len(seg), 0, len(seg), out_n, sub.ctypes.data, tok.ctypes.data, C.byref(ntok),
                                  C.byref(raw), C.byref(raw_off))
    return st, tok, ntok.value


def test_sub_indexed_path(core, cases, judged):
    """through the region lanes: the two in-place classes and every header class get the rule's status, not merely an error"""
    seg, sub, out, patched = M.sub_fixed_segment()
    st, tok, ntok = _sub(core, seg, M.SEG, sub)
    assert st == 0
    got = np.zeros(M.SEG, np.uint8)
    assert core.sfi_expand_tokens(tok.ctypes.data, ntok, got.ctypes.data, M.SEG) == M.SEG and got.tobytes() == out
    for name, (bad, hint) in patched.items():
        want = M.rule(S.serial, bad, M.SEG)[0]
        assert want == hint, name
        assert _sub(core, bad, M.SEG, sub)[0] == want, name
    wrong = sub.copy()
    wrong[7, 0] += 1  # a good stream under a wrong sub-index stays Error
    assert _sub(core, seg, M.SEG, wrong)[0] == M.ERROR
    for c in cases:
        if c.cls in M.HEADER_CLASSES and c.place == "a" and c.hint != 0:
            assert _sub(core, c.segment(), c.out_n, np.zeros((32, 2), np.uint32))[0] == judged[c.name][0], c.name
