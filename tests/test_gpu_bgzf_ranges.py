"""BGZF random access on the device (sfh_decompress_bgzf_ranges_device, sfh_decompress_bgzf_ranges): byte ranges of a BGZF
file decoded for the members that hold them.  The files are made with Python's zlib (tests/bgzf_files.py), the expected
bytes are slices of the payload; the calls and range sets are in tests/bgzf_range_cases.py.  Every device call runs with its
destinations packed into one guarded buffer: a byte written outside a destination fails the call's helper."""
import ctypes as C
import gzip
import hashlib
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import bgzf_files as BZ
import bgzf_range_cases as R
import bgzf_wide_cases as K
import deflate_writer as W
import starflate_amd as sa
from conftest import ROOT
from starflate_amd import Compressor, _capi

pytestmark = pytest.mark.gpu

INVALID_ARG, NOT_INDEXABLE = -1, -8
WIDE = 65280


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def narrow():
    return R.narrow_case()


@pytest.fixture(scope="module")
def wide():
    return R.wide_case()


def child(case, **env):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]), **env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bgzf_range_cases.py"), case], env=env, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    scratch, digest = out.stdout.split()[-2:]
    return int(scratch), digest


# ---- 1. narrow rows ----
def test_narrow_rows(comp, narrow):
    data, blob, ranges = narrow
    assert len(ranges) > 100 and (0, len(data)) in ranges and (len(data), 0) in ranges
    rc, outs, st, pos = R.run_device(comp, blob, ranges)
    assert rc == 0
    R.check_exact(data, ranges, outs, st)
    assert len({p % 4 for p in pos}) == 4  # every destination alignment
    assert comp.last_decode_scratch_bytes() <= len(ranges) * 3 * 32768 * 4


# ---- 2. wide rows, coded members; the lane-serial token kernel ----
def test_wide_rows(comp, wide):
    data, blob, ranges = wide
    assert BZ.walk(blob)[2] == 65536
    rc, outs, st, pos = R.run_device(comp, blob, ranges)
    assert rc == 0
    R.check_exact(data, ranges, outs, st)
    assert len({p % 4 for p in pos}) == 4
    # the same ranges with SFH_INFLATE_SERIAL=1, in a fresh process: the same bytes
    _, digest = child("wide", SFH_INFLATE_SERIAL="1")
    assert digest == hashlib.sha256(b"".join(outs)).hexdigest()


# ---- 3. wide stored members ----
def test_wide_stored_members(comp):
    """Members of 65280 random bytes in one stored block each (level 0), and one member of two stored blocks.  (A member of
    65535 + 1 stored bytes does not exist: with its two block headers and the wrapper it would take 65572 bytes, and BSIZE
    holds 65536.  The largest member of two stored blocks holds 65500 bytes: here 65499 + 1.)"""
    rnd = np.random.default_rng(41).integers(0, 256, 2 * WIDE + 65500, dtype=np.uint8).tobytes()
    blob, moff, ooff = BZ.write(rnd[: 2 * WIDE], [WIDE, WIDE], level=0, eof=False)
    assert blob[moff[0] + 18: moff[0] + 23] == b"\x00" + struct.pack("<HH", WIDE, WIDE ^ 0xFFFF)  # LEN = 65280
    bw = W.BitWriter()
    W.write_stored(bw, rnd[2 * WIDE: 2 * WIDE + 65499])
    W.write_stored(bw, rnd[2 * WIDE + 65499:], final=True)
    two = K.hand_member(bw.bytes().tobytes(), rnd[2 * WIDE:])
    assert len(two) == 65536
    blob += two + BZ.EOF
    assert gzip.decompress(blob) == rnd
    ooff = [0, WIDE, 2 * WIDE]
    ranges = []
    for b in ooff:
        ranges += [(b + 5, 1000), (b + 100, 32000),              # inside the first 32 KiB
                   (b + 40000, 20000), (b + 32768 + 513, 7),      # inside the last 32 KiB
                   (b + 30000, 5000), (b + 32767, 2), (b + 1, 65000),  # across the middle
                   (b + 65279, 1)]
    ranges += [(ooff[2] + 65498, 2), (ooff[2] + 65499, 1), (ooff[1] - 2, 5), (0, len(rnd))]
    rc, outs, st, _ = R.run_device(comp, blob, ranges)
    assert rc == 0
    R.check_exact(rnd, ranges, outs, st)
    info = comp.debug(_capi.DBG_SEGINFO, 1)
    assert int(info[0, 2]) & 1, "a member of one stored block takes the raw copy"


# ---- 4. far matches inside a wide member ----
def test_far_matches_inside_a_wide_member(comp):
    """the second half repeats the first 32 KiB at distance 32768 (zlib's own matches stop at 32506: the body is written by
    hand); the ranges lie in the second half only, and the member must still be resolved from its start"""
    t = K._lits(32768, 11) + [W.match(258, 32768)] * 126 + [W.match(4, 32768)]
    payload = W.expand(t)
    assert len(payload) == WIDE and payload[32768:] == payload[: WIDE - 32768]
    tail = BZ.text(100, seed=43)
    blob = K.hand_member(K.body_of_tokens(t), payload) + BZ.member(tail) + BZ.EOF
    assert gzip.decompress(blob) == payload + tail
    ranges = [(32768, 1), (32768 + 5, 4096), (40000, WIDE - 40000), (WIDE - 3, 3), (WIDE - 1, 2), (33000, 258 * 3 + 1)]
    rc, outs, st, _ = R.run_device(comp, blob, ranges)
    assert rc == 0
    R.check_exact(payload + tail, ranges, outs, st)


# ---- 5. damage ----
@pytest.fixture(scope="module")
def three():
    data = BZ.text(3 * WIDE, seed=21)
    blob, moff, ooff = BZ.write(data, [WIDE] * 3)
    return data, blob, moff, ooff


def _inflate_rejects(member):
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(member[18: -8]) + d.flush()
    except zlib.error:
        return True
    return len(out) != WIDE or not d.eof


def _whole_file_status(comp, blob, total):
    out, n, st = comp.decompress_bgzf_wide_tensor(R.cuda(blob), total)
    return st


def test_damage(comp, three):
    data, blob, moff, ooff = three
    index = R.device_index(comp, blob)  # (of the undamaged file)
    body1 = moff[2] - 8 - (moff[1] + 18)
    at = next(a for a in range(moff[1] + 18 + body1 - body1 // 8, moff[2] - 8)
              if _inflate_rejects(BZ.patched(blob, a, bytes([blob[a] ^ 0x55]))[moff[1]: moff[2]]))
    bad = BZ.patched(blob, at, bytes([blob[at] ^ 0x55]))
    want = _whole_file_status(comp, bad, len(data))
    assert want != 0
    # ranges inside members 0 and 2; ranges whose span holds member 1: one at its start (its window misses the damage), one
    # over its end, one from member 0 into it
    ranges = [(100, 4096), (ooff[2] + 40000, 4096), (ooff[1] + 3, 100), (ooff[2] - 50, 100), (ooff[1] - 10, 20), (ooff[2], 5)]
    hit = [False, False, True, True, True, False]
    for name, blob_k, status_k in (("a body byte", bad, want),
                                   ("ISIZE = out_n - 1", BZ.patched(blob, moff[2] - 4, struct.pack("<I", WIDE - 1)), BZ.ERROR),
                                   ("bad CM", BZ.patched(blob, moff[1] + 2, b"\x07"), BZ.ERROR)):
        # (the damaged file's own walk: the ISIZE case would shift its index, the CM case fails it -- the undamaged file's holds)
        rc, outs, st, _ = R.run_device(comp, blob_k, ranges, index=index)
        assert rc == 0, name
        for (off, ln), got, s, h in zip(ranges, outs, st, hit):
            if h:
                assert s == status_k, (name, off, ln, s)
            else:
                assert s == 0 and got == data[off: off + ln], (name, off, ln, s)
        # the host call, index given: a failed range's destination is left untouched
        got, hst = comp.read_bgzf_ranges(blob_k, [r[0] for r in ranges], [r[1] for r in ranges],
                                         index=(index[0].cpu().numpy(), index[1].cpu().numpy(), index[2]))
        assert [int(s) for s in hst] == st, name
        assert [g is None for g in got] == hit and all(g == data[o: o + n] for g, (o, n), h in zip(got, ranges, hit) if not h), name


def test_host_call_leaves_a_failed_ranges_destination_untouched(comp, three):
    data, blob, moff, ooff = three
    bad = BZ.patched(blob, moff[1] + 2, b"\x07")
    m_off, o_off, info = sa.bgzf_index(blob)
    binfo = R.info_struct(info)
    dsts = [np.full(300, R.GUARD, np.uint8) for _ in range(2)]
    dp = (C.c_void_p * 2)(*[d.ctypes.data for d in dsts])
    st = np.full(2, 9, np.uint32)
    src = np.frombuffer(bad, np.uint8)
    rc = _capi.lib().sfh_decompress_bgzf_ranges(comp._h, src.ctypes.data, src.size, m_off.ctypes.data, o_off.ctypes.data, C.byref(binfo), 2,
                                                (C.c_uint64 * 2)(ooff[1] + 5, 7), (C.c_uint64 * 2)(200, 200), dp, st.ctypes.data)
    assert rc == 0 and [int(s) for s in st] == [BZ.ERROR, 0]
    assert np.all(dsts[0] == R.GUARD)
    assert dsts[1][:200].tobytes() == data[7: 207] and np.all(dsts[1][200:] == R.GUARD)


# ---- 6. a lying index ----
def test_lying_index(comp, narrow):
    data, blob, _ = narrow
    big = BZ.good_files()["65280-byte members"]
    index = R.device_index(comp, big[1])  # larger members, a larger file: most of its offsets lie behind this file's end
    total = index[2]["total_n"]
    ranges = [(0, 100), (65279, 3), (70000, 4096), (total - 5, 5), (0, total), (10, 0), (total, 0)]
    rc, outs, st, _ = R.run_device(comp, blob, ranges, index=index)
    assert rc == 0
    assert all((s != 0) == (ln != 0) for (_, ln), s in zip(ranges, st)), st
    # the narrow file's own index with wide members' info, and the other way round: statuses or bytes, never a stray write
    own = R.device_index(comp, blob)
    rc, outs, st, _ = R.run_device(comp, blob, [(0, 100), (200, 30000)], index=own, max_isize=65536)
    assert rc == 0 and st == [0, 0] and outs[0] == data[:100]  # (wide rows hold narrow members)
    own_big = R.device_index(comp, big[1])
    rc, outs, st, _ = R.run_device(comp, big[1], [(0, 100), (65279, 3)], index=own_big, max_isize=32768)
    assert rc == 0 and st == [BZ.ERROR, BZ.ERROR]  # a member above the row width: Error, no row the kernels would overrun


# ---- 7. launch batches ----
def test_launch_batches(comp):
    data, blob, ranges = R.batches_case()
    rc, outs, st, _ = R.run_device(comp, blob, ranges)
    assert rc == 0
    R.check_exact(data, ranges, outs, st)
    # SFH_BATCH_CHUNKS=2 in a fresh process: a wide launch batch holds ONE row, so the five-member span crosses four batch
    # boundaries; the token scratch is one batch's
    scratch, digest = child("batches", SFH_BATCH_CHUNKS="2")
    assert digest == hashlib.sha256(b"".join(outs)).hexdigest()
    assert scratch == 1 * 65536 * 4
    scratch, digest = child("narrow", SFH_BATCH_CHUNKS="2")
    assert scratch == 2 * 32768 * 4


# ---- 8. the host twin ----
@pytest.mark.parametrize("case", ["narrow", "wide"])
def test_host_twin(comp, narrow, wide, case):
    """The bytes that go up are the spans' pieces, not the file: the staging exposes no counter or size to observe that
    through, so this is not asserted here (the piece arithmetic is held against its model in test_bgzf_range_plan_host.py)."""
    data, blob, ranges = narrow if case == "narrow" else wide
    offs, lens = [r[0] for r in ranges], [r[1] for r in ranges]
    for index in (None, sa.bgzf_index(blob)):
        got, st = comp.read_bgzf_ranges(blob, offs, lens, index=index)
        assert not st.any()
        assert got == [data[o: o + n] for o, n in ranges]
    got, st = sa.read_bgzf_ranges(blob, offs[:5], lens[:5])
    assert got == [data[o: o + n] for o, n in ranges[:5]]


def test_host_twin_on_a_file_that_does_not_parse(comp):
    name, blob, want = BZ.damaged()[0]
    got, st = comp.read_bgzf_ranges(blob, [0, 5], [10, 0])
    assert got == [None, None] and [int(s) for s in st] == [want, want]


# ---- 9. refusals and edges ----
def _raw(comp, src, n, moff, ooff, binfo, k, offs, lens, dsts, status, stream=None):
    return _capi.lib().sfh_decompress_bgzf_ranges_device(
        comp._h, src, n, moff, ooff, C.byref(binfo) if binfo is not None else None, k,
        (C.c_uint64 * len(offs))(*offs) if offs is not None else None, (C.c_uint64 * len(lens))(*lens) if lens is not None else None,
        (C.c_void_p * len(dsts))(*dsts) if dsts is not None else None, status, stream)


def test_refusals(comp, narrow):
    data, blob, _ = narrow
    src = R.cuda(blob)
    moff, ooff, info = R.device_index(comp, blob)
    binfo = R.info_struct(info)
    out = torch.full((4096,), R.GUARD, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    good = dict(src=src.data_ptr(), n=len(blob), moff=moff.data_ptr(), ooff=ooff.data_ptr(), binfo=binfo, k=2, offs=[0, 50], lens=[10, 10],
                dsts=[out.data_ptr(), out.data_ptr() + 10], status=status.data_ptr())
    assert _raw(comp, **good) == 0
    torch.cuda.synchronize()
    assert out[:20].cpu().numpy().tobytes() == data[:10] + data[50:60] and status[:2].tolist() == [0, 0]
    total = len(data)
    for name, change in [("null file", dict(src=None)), ("null member_off", dict(moff=None)), ("null out_off", dict(ooff=None)),
                         ("null info", dict(binfo=None)), ("null offsets", dict(offs=None)), ("null lengths", dict(lens=None)),
                         ("null dsts", dict(dsts=None)), ("null status", dict(status=None)),
                         ("a null destination", dict(dsts=[out.data_ptr(), None])),
                         ("misaligned file", dict(src=src.data_ptr() + 1)), ("misaligned member_off", dict(moff=moff.data_ptr() + 4)),
                         ("misaligned out_off", dict(ooff=ooff.data_ptr() + 4)), ("misaligned status", dict(status=status.data_ptr() + 2)),
                         ("behind total_n", dict(offs=[0, total - 5])), ("offset behind total_n", dict(offs=[0, total + 1], lens=[10, 0])),
                         ("overflowing", dict(offs=[0, (1 << 64) - 1], lens=[10, 2])),
                         ("overlapping destinations", dict(dsts=[out.data_ptr(), out.data_ptr() + 9]))]:
        out.fill_(R.GUARD)
        status.fill_(77)
        torch.cuda.synchronize()
        assert _raw(comp, **dict(good, **change)) == INVALID_ARG, name
        torch.cuda.synchronize()
        assert bool((out == R.GUARD).all()) and status.tolist() == [77] * 4, name
    assert _capi.lib().sfh_decompress_bgzf_ranges_device(None, None, 0, None, None, None, 0, None, None, None, None, None) == INVALID_ARG  # no context
    # not BGZF; no ranges; an index that failed
    assert _raw(comp, **dict(good, binfo=R.info_struct(info, max_isize=65537))) == NOT_INDEXABLE
    assert _raw(comp, **dict(good, k=0)) == 0
    assert _raw(comp, None, 0, None, None, None, 0, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((out == R.GUARD).all()) and status.tolist() == [77] * 4
    assert _raw(comp, **dict(good, binfo=R.info_struct(info, status=5))) == 0
    torch.cuda.synchronize()
    assert status[:2].tolist() == [5, 5] and bool((out == R.GUARD).all())
    # the host call's own refusals
    h = np.frombuffer(blob, np.uint8)
    hm, ho, hinfo = sa.bgzf_index(blob)
    L = _capi.lib()
    dst = np.zeros(64, np.uint8)
    hst = np.zeros(2, np.uint32)
    args = lambda m, o, i, offs=(0,), lens=(10,), d=dst.ctypes.data, s=hst.ctypes.data: (  # noqa: E731
        comp._h, h.ctypes.data, h.size, m, o, i, 1, (C.c_uint64 * 1)(*offs), (C.c_uint64 * 1)(*lens), (C.c_void_p * 1)(d), s)
    hb = R.info_struct(hinfo)
    assert L.sfh_decompress_bgzf_ranges(*args(hm.ctypes.data, ho.ctypes.data, C.byref(hb))) == 0 and dst[:10].tobytes() == data[:10]
    assert L.sfh_decompress_bgzf_ranges(*args(hm.ctypes.data, None, C.byref(hb))) == INVALID_ARG  # all three or none
    assert L.sfh_decompress_bgzf_ranges(*args(None, None, None, offs=(total,), lens=(1,))) == INVALID_ARG
    assert L.sfh_decompress_bgzf_ranges(*args(None, None, None, s=None)) == INVALID_ARG
    assert L.sfh_decompress_bgzf_ranges(*args(None, None, None, d=None)) == INVALID_ARG
    assert L.sfh_decompress_bgzf_ranges(*args(hm.ctypes.data, ho.ctypes.data, C.byref(R.info_struct(hinfo, max_isize=65537)))) == NOT_INDEXABLE
    assert L.sfh_decompress_bgzf_ranges(*args(hm.ctypes.data, ho.ctypes.data, C.byref(R.info_struct(hinfo, status=5)))) == 0 and hst[0] == 5


def test_more_rows_than_a_call_holds(comp):
    """65537 members of one byte and 32769 ranges over all of them: 2^31 + 98305 rows.  Refused once the planner's row total
    is known; no decoder kernel runs, no destination is touched."""
    one = BZ.member(b"a")
    m = 65537
    blob = one * m + BZ.EOF
    src = R.cuda(blob)
    moff, ooff, info = comp.bgzf_index_tensor(src)
    assert info["members"] == m + 1 and info["total_n"] == m
    k = 32769
    out = torch.full((k * m,), R.GUARD, dtype=torch.uint8, device="cuda")
    status = torch.full((k,), 77, dtype=torch.int32, device="cuda")
    rc = _raw(comp, src.data_ptr(), len(blob), moff.data_ptr(), ooff.data_ptr(), R.info_struct(info), k, [0] * k, [m] * k,
              [out.data_ptr() + r * m for r in range(k)], status.data_ptr())
    torch.cuda.synchronize()
    assert rc == INVALID_ARG and "2^31" in comp.last_error()
    assert bool((out == R.GUARD).all()) and bool((status == 77).all())
    # one range fewer rows than that: 3 ranges run
    rc, outs, st, _ = R.run_device(comp, blob, [(0, m), (5, 1), (m - 1, 1)], index=(moff, ooff, info))
    assert rc == 0 and st == [0, 0, 0] and outs == [b"a" * m, b"a", b"a"]


def test_callers_stream_and_context_reuse(comp, narrow, wide):
    stream = torch.cuda.Stream()
    for _ in range(2):
        for data, blob, ranges in (narrow, wide):
            rc, outs, st, _ = R.run_device(comp, blob, ranges[::7], stream=stream.cuda_stream)
            assert rc == 0
            R.check_exact(data, ranges[::7], outs, st)
            # a whole-file decode between two range calls on the one context
            out, n, s = comp.decompress_bgzf_wide_tensor(R.cuda(blob), len(data))
            assert s == 0 and out[:n].cpu().numpy().tobytes() == data
    assert comp._lib.sfh_index_entries(comp._h) == 0  # afterwards the context holds no index


# ---- 10. the Python surface; virtual offsets ----
def test_python_surface_and_virtual_offsets(comp, wide):
    data, blob, ranges = wide
    moff, ooff, info = sa.bgzf_index(blob)
    # a file from the library's own writer, and bgzip's member size
    own = BZ.text(200000, seed=51)
    for payload, file_k in ((own, comp.compress_bgzf(own)), (data, blob)):
        rng = np.random.default_rng(52)
        offs = [int(v) for v in rng.integers(0, len(payload) - 5000, 12)]
        lens = [int(v) for v in rng.integers(1, 5000, 12)]
        got, st = comp.read_bgzf_ranges(file_k, offs, lens)
        assert not st.any() and got == [payload[o: o + n] for o, n in zip(offs, lens)]
        src = R.cuda(file_k)
        d_moff, d_ooff, d_info = comp.bgzf_index_tensor(src)
        outs, dst = comp.read_bgzf_ranges_tensor(src, d_moff, d_ooff, d_info, offs, lens)
        assert dst.tolist() == [0] * 12
        assert [o[:n].cpu().numpy().tobytes() for o, n in zip(outs, lens)] == got
        # packed views as destinations
        pack = torch.zeros(sum(lens), dtype=torch.uint8, device="cuda")
        at = np.concatenate([[0], np.cumsum(lens)])
        views = [pack[int(a): int(a) + n] for a, n in zip(at, lens)]
        comp.read_bgzf_ranges_tensor(src, d_moff, d_ooff, d_info, offs, lens, outs=views)
        assert pack.cpu().numpy().tobytes() == b"".join(got)
    # virtual offsets taken from the index fetch the same bytes as the offsets they translate to
    vs = [int(m) << 16 | u for m, a, b in zip(moff, ooff, ooff[1:]) for u in (0, min(7, int(b - a) - 1)) if b > a]
    offs = [int(o) for o in sa.bgzf_voffsets_to_offsets(moff, ooff, vs)]
    assert offs == [int(a) + u for a, b in zip(ooff, ooff[1:]) for u in (0, min(7, int(b - a) - 1)) if b > a]
    lens = [min(300, len(data) - o) for o in offs]
    got, st = comp.read_bgzf_ranges(blob, offs, lens, index=(moff, ooff, info))
    assert not st.any() and got == [data[o: o + n] for o, n in zip(offs, lens)]
    assert [int(v) for v in sa.bgzf_offsets_to_voffsets(moff, ooff, offs)] == vs
