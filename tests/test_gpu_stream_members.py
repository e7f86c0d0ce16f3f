"""Files of gzip members decoded on the GPU (container="gzip_members", SFH_GZIP_MEMBERS; DESIGN.md 3a "Files of members").
Every result is compared with the host specification (include/starflate/container.hpp, decompress_members, through
tests/members_host.py) and, where the status is 0, with gzip.decompress.  Two contexts: nominal chunks of 512 bytes, where
chunk starts fall into every part of a member, and the default."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest
import torch

import bgzf_files as B
import deflate_writer as W
import members_cases as MC
import members_host as MH
import stream_cases as SC
import starflate_amd
from starflate_amd import Compressor, _capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = "gzip_members"
INVALID_ARG = -1
# sf::StreamMember, the SFH_DBG_STREAM_MEMBERS record
RECORD = np.dtype([("src_end", "<u8"), ("out_end", "<u8"), ("crc32", "<u4"), ("isize", "<u4"), ("item", "<u4"), ("status", "<u4")])
assert RECORD.itemsize == 32


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def _ctx(mp, **env):
    for k, v in env.items():
        mp.setenv(k, v)
    c = Compressor(0)
    for k in env:
        mp.delenv(k)
    return c


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(monkeypatch_module):
    c = _ctx(monkeypatch_module, SFH_STREAM_CHUNK="512")
    yield c
    c.close()


def check(c, blob, cap=None):
    """one file through the size query (cap None) and the decode against the specification -> (status, stats of the decode)"""
    want_st, want, _ = MH.spec(blob, 8 * MC.BIG if cap is None else cap)
    out, st = c.decompress_stream(blob, cap, KIND)
    s = c.last_stream_stats()
    assert st == want_st, (st, want_st, s)
    if st == 0:
        assert out == want
        assert out == gzip.decompress(blob)
    else:
        assert out == b""
    return st, s


def aligned_second(first, second, S=512):
    """first, zero bytes, second: the second member's head on a nominal chunk boundary of the body (bytes from the first header's
    end, 10), so that its body start is the first thing the finder meets in that chunk's range"""
    m1 = MC.member(first)
    pad = -(len(m1) - 10) % S
    return m1 + bytes(pad) + MC.member(second)


def far_match_member(n=70000):
    """a raw stream: 32768 random literals, then copies at distance 32768 up to n bytes"""
    rng = np.random.default_rng(32768)
    b = SC.Builder()
    for _ in range(8):
        b.dynamic([int(x) for x in rng.integers(0, 256, 4096)])
    left = n - 32768
    toks = [W.match(258, 32768)] * (left // 258) + ([W.match(left % 258, 32768)] if left % 258 >= 3 else [])
    b.dynamic(toks, final=True)
    return b.bw.bytes().tobytes(), bytes(b.out)


def lookalike_files():
    inner = MC.join(MC.pieces(3000, 1000, 8))  # a complete gzip file of three members
    deflate = MC.raw(MC.text(20000, 9), level=6)  # a run of DEFLATE data
    out = {}
    for name, payload in (("gzip_file_in_stored", inner * 8), ("deflate_in_stored", deflate)):
        b = SC.Builder()
        b.stored(payload[: len(payload) // 2])
        b.stored(payload[len(payload) // 2:], final=True)
        out[name] = MC.join([MC.text(2000, 1)]) + MC.member(payload, body=b.bw.bytes().tobytes()) + MC.join([MC.text(2000, 2)])
    return out


def chunk_files():
    t = MC.text(300000, 7)
    far_raw, far_data = far_match_member()
    return {
        "three_of_1500": MC.join(MC.pieces(13500, 4500, 1)),
        "forty_of_100": MC.join(MC.pieces(40 * 160, 160, 2)),
        "empties_2000": MC.member(b"") * 2000,
        "big_then_five": MC.join([t[:204800]] + MC.pieces(5000, 1000, 3)),
        "second_on_a_candidate": aligned_second(t[:5000], t[5000:15000]),
        "stored_second": MC.join([t[:4000]]) + MC.member(t[4000:9000], body=MC.stored_first(t[4000:9000], 2500)) + MC.join([t[9000:12000]]),
        "fixed_second": MC.join([t[:4000]]) + MC.member(t[4000:6000], body=MC.fixed_first(t[4000:6000])) + MC.join([t[6000:9000]]),
        "far_match_in_second": MC.join([t[:40000]]) + MC.member(far_data, body=far_raw),
    }


CHUNK_FILES = chunk_files()
GOOD = MC.good()
BAD = MC.bad()
LOOK = lookalike_files()
# the window rule: member 2 opens with a match of distance 5 behind `fill` literals of its own; member 1 is 200 or 20000 bytes
REACH = {"in_the_closing_chunk": MC.member(MC.text(200, 5)) + MC.member(b"", body=MC.reach_back()),
         "chunks_later": MC.member(MC.text(200, 5)) + MC.member(b"", body=MC.reach_back(fill=20000, dist=5))}


@pytest.mark.parametrize("name", sorted(CHUNK_FILES))
def test_members_against_chunks(small, name):
    blob = CHUNK_FILES[name]
    st, s = check(small, blob)
    assert st == 0
    st, s = check(small, blob, len(gzip.decompress(blob)))
    assert st == 0
    # zlib writes members of this size as one block each, so the only true chunk starts are the members' body starts
    if name == "second_on_a_candidate":
        assert (s["candidates"], s["confirmed"]) == (2, 2), s  # the file's first bit and member 2's body
    if name == "three_of_1500":
        assert s["confirmed"] == 3, s
    if name == "big_then_five":
        assert s["confirmed"] > 5, s


@pytest.mark.parametrize("name", sorted(GOOD))
def test_host_cases_on_both_contexts(comp, small, name):
    for c in (comp, small):
        assert check(c, GOOD[name])[0] == 0


@pytest.mark.parametrize("name", sorted(REACH))
def test_a_match_may_not_leave_its_member(comp, small, name):
    """reach_back(fill): the offending match lies `fill` bytes into member 2, so with 20000 it is chunks behind the member's start"""
    for c in (comp, small):
        st, _ = check(c, REACH[name], MC.BIG)
        assert st == SC.INVALID_DISTANCE


def test_what_users_have_joined_batch_items(comp, small):
    parts = [MC.text(100 << 10, 10 + i) for i in range(5)]
    blob = b"".join(comp.compress_batch(parts, container="gzip"))
    assert gzip.decompress(blob) == b"".join(parts)
    for c in (comp, small):
        assert check(c, blob)[0] == 0


@pytest.mark.parametrize("name", ["sizes eof=True", "no EOF member", "stored members", "65280-byte members"])
def test_what_users_have_bgzf(comp, small, name):
    data, blob = B.good_files()[name][:2]
    for c in (comp, small):
        assert check(c, blob)[0] == 0
        assert c.decompress_stream(blob, None, KIND) == c.decompress_bgzf(blob) == (data, 0)


def test_what_users_have_five_mib_of_64k_members(comp):
    data = MC.text(5 << 20, 12)
    blob = MC.join([data[i: i + 65536] for i in range(0, len(data), 65536)])
    st, s = check(comp, blob)
    assert st == 0 and s["confirmed"] >= 80, s


def test_a_single_member_is_the_gzip_case(comp, small):
    blob = MC.join([MC.text(50000, 13)])
    for c in (comp, small):
        for cap in (None, 50000, 49999, 60000):
            assert c.decompress_stream(blob, cap, KIND) == c.decompress_stream(blob, cap, "gzip")


@pytest.mark.parametrize("name", sorted(LOOK))
def test_lookalikes(comp, small, name):
    for c in (comp, small):
        st, s = check(c, LOOK[name])
        assert st == 0
        assert s["repair_rounds"] <= 2, s  # (one follow lane mends a run of false candidates: tests/test_gpu_stream.py)


@pytest.mark.parametrize("name", sorted(BAD))
def test_statuses(comp, small, name):
    blob, cap, want = BAD[name]
    for c in (comp, small):
        st, _ = check(c, blob, cap)
        assert st == want


def test_trailers_are_checked_behind_the_bodies(comp, small):
    """the documented difference: a wrong CRC in member 1 and a type-3 block in member 3 -- the host stops at the CRC (1), the
    device reports the body (2)"""
    t = MC.text(6000, 14)
    blob = MC.member(t[:2000], crc=1) + MC.member(t[2000:4000]) + MC.member(b"", body=bytes([0x07]) + bytes(8))
    assert MH.spec(blob, MC.BIG)[0] == SC.ERROR
    for c in (comp, small):
        assert c.decompress_stream(blob, MC.BIG, KIND) == (b"", SC.INVALID_BLOCK_HEADER)


def test_size_query(comp, small):
    t = MC.text(6000, 15)
    wrong_crc = MC.member(t[:3000]) + MC.member(t[3000:], crc=7)
    short = MC.join([t[:3000], t[3000:]])[:-2]
    n, st = C.c_uint64(0), C.c_uint32(9)
    for c in (comp, small):
        for blob, want in ((wrong_crc, (0, 6000)), (short, (SC.SRC_TOO_SMALL, None))):
            src = np.frombuffer(blob, np.uint8)
            assert c._lib.sfh_inflate_stream(c._h, src.ctypes.data, src.size, 4, None, 0, C.byref(n), C.byref(st)) == 0
            assert st.value == want[0] and (want[1] is None or n.value == want[1])
        assert c.decompress_stream(wrong_crc, None, KIND) == (b"", SC.ERROR)


def batch_items():
    t = MC.text(250000, 16)  # (alone nearly a launch batch of SFH_BATCH_CHUNKS=8: 256 KiB of output)
    return [(CHUNK_FILES["three_of_1500"], MC.BIG), BAD["wrong_crc_2_of_3"][:2], (MC.member(b"") * 30, 0),
            (MC.join([t[:125000], t[125000:]]), 250000), BAD["reach_into_member_1"][:2], (GOOD["zeros"], 9000 + 16)]


def test_batch(comp, small, monkeypatch_module):
    items = batch_items()
    blobs, caps = [b for b, _ in items], [c for _, c in items]
    split = _ctx(monkeypatch_module, SFH_BATCH_CHUNKS="8", SFH_STREAM_CHUNK="512")
    try:
        for c in (comp, small, split):
            singles = [c.decompress_stream(b, cap, KIND) for b, cap in items]
            assert [st for _, st in singles] == [MH.spec(b, cap)[0] for b, cap in items]
            assert sum(1 for _, st in singles if st) == 2
            outs, sts = c.decompress_stream_batch(blobs, caps, KIND)
            assert list(zip(outs, sts)) == singles
            assert c.decompress_stream_batch(blobs, None, KIND) == (outs, sts)
            # device tensors: each destination inside a guarded buffer
            srcs = [torch.from_numpy(np.frombuffer(b + bytes(-len(b) % 4), np.uint8).copy()).cuda()[: len(b)] for b in blobs]
            room = [min(cap, 300000) for cap in caps]
            guards = [torch.full((64 + r + 64,), 0xA5, dtype=torch.uint8, device="cuda") for r in room]
            touts, tsts = c.decompress_stream_batch_tensors(srcs, room, KIND, outs=[g[64: 64 + max(r, 1)] for g, r in zip(guards, room)])
            assert tsts == sts
            for g, r, o, out, st in zip(guards, room, touts, outs, sts):
                h = g.cpu().numpy()
                assert (h[:64] == 0xA5).all() and (h[64 + max(r, 1):] == 0xA5).all()
                if st == 0:
                    assert o.cpu().numpy().tobytes() == out
    finally:
        split.close()
    assert starflate_amd.decompress_stream_batch(blobs, caps, KIND) == (outs, sts)


def read_table(c, cap=4096):
    buf = np.zeros(8 + cap * 32, np.uint8)
    rc = c._lib.sfh_debug_read(c._h, _capi.DBG_STREAM_MEMBERS, buf.ctypes.data, buf.size)
    if rc:
        return rc, None
    n = int(buf[:8].view("<u8")[0])
    return 0, buf[8: 8 + min(n, cap) * 32].view(RECORD)


def test_member_table(comp, small):
    t = MC.text(9000, 17)
    blobs = [GOOD["three"], MC.member(t[:100]) + MC.member(t[100:200], isize=5) + MC.member(b""), BAD["type3_in_member_3"][0],
             GOOD["zeros"]]
    for c in (comp, small):
        outs, sts = c.decompress_stream_batch(blobs, [MC.BIG] * 4, KIND)
        assert sts == [0, SC.ERROR, SC.INVALID_BLOCK_HEADER, 0]
        rc, rows = read_table(c)
        assert rc == 0
        want = []
        for i in (0, 1, 3):  # (item 2's body did not decode: no records)
            src = out = 0
            blob = blobs[i]
            for k, r in enumerate(MH.spec(blob if i != 1 else MC.member(t[:100]) + MC.member(t[100:200]) + MC.member(b""), MC.BIG)[2]):
                want.append((int(r["src_end"]), int(r["out_end"]), int(r["crc32"]), 5 if (i, k) == (1, 1) else int(r["isize"]), i,
                             int((i, k) == (1, 1))))
        assert [tuple(int(x) for x in r) for r in rows] == want
        # as many whole records as fit, and never fewer than the count's 8 bytes
        rc, two = read_table(c, cap=2)
        assert rc == 0 and len(two) == 2 and [tuple(int(x) for x in r) for r in two] == want[:2]
        tiny = np.zeros(7, np.uint8)
        assert c._lib.sfh_debug_read(c._h, _capi.DBG_STREAM_MEMBERS, tiny.ctypes.data, 7) == INVALID_ARG
        assert c.decompress_stream(GOOD["one"], None, "gzip")[1] == 0
        assert read_table(c)[0] == INVALID_ARG


def test_refusals_on_a_context(comp):
    blob = np.frombuffer(GOOD["one"], np.uint8)
    dst = np.zeros(4096, np.uint8)
    n, st, sz = C.c_uint64(0), C.c_uint32(0), C.c_size_t(0)
    lib, h = comp._lib, comp._h
    sp, dp = (C.c_void_p * 1)(blob.ctypes.data), (C.c_void_p * 1)(dst.ctypes.data)
    sn, dn = (C.c_uint64 * 1)(blob.size), (C.c_uint64 * 1)(3000)
    st1 = np.zeros(1, np.uint32)
    assert lib.sfh_decompress_batch(h, 1, sp, sn, None, None, dp, dn, None, 4, st1.ctypes.data) == INVALID_ARG
    assert lib.sfh_decompress_any(h, blob.ctypes.data, blob.size, 4, dst.ctypes.data, 3000, 3000, C.byref(n), C.byref(st)) == INVALID_ARG
    o = _capi.make_options()
    o.container = 4
    assert lib.sfh_compress(h, dst.ctypes.data, 4096, dst.ctypes.data, 4096, C.byref(sz), C.byref(o)) == INVALID_ARG
    assert lib.sfh_compress_bound_container(1000, 0, 4) == 0
    assert lib.sfh_inflate_stream(h, blob.ctypes.data, blob.size, 9, dst.ctypes.data, 4096, C.byref(n), C.byref(st)) == INVALID_ARG
    st2 = (C.c_uint32 * 1)()
    n2 = (C.c_uint64 * 1)()
    assert lib.sfh_inflate_stream_batch(h, 1, sp, sn, 9, dp, dn, n2, st2) == INVALID_ARG
    with pytest.raises(ValueError):
        comp.decompress_stream(GOOD["one"], None, "dictzip")


def test_cpp_host_api(tmp_path):
    """tests/cpp/stream_members.cpp: compressor::decompress_stream(..., Container::GzipMembers) round trip"""
    from starflate_amd import build

    lib = build.build()
    exe = tmp_path / "stream_members"
    libdir = os.path.dirname(lib)
    flags = ["-std=c++23", "-fno-exceptions", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror", "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["/opt/rocm/llvm/bin/clang++", "-O2"] + flags + [os.path.join(ROOT, "tests", "cpp", "stream_members.cpp"),
                                                                          "-L" + libdir, "-lstarflate_hip", "-Wl,-rpath," + libdir,
                                                                          "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
