"""Batched decompression (sfh_decompress_batch / sfh_decompress_batch_device_async) and the batch index
(sfh_batch_index_size / sfh_copy_batch_index): compress_batch's items come back exact from their batch index, a raw item's
bytes and status are the single decoder's on it alone, a wrapped item's status is include/starflate/container.hpp's, items
stay isolated from one another, and pages from zlib decode without an index."""
import ctypes as C
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from conftest import ROOT
from starflate_amd import Compressor, synth
from single_decode_cases import context_under, damaged_batch, first_entry_batch, parent_record

pytestmark = pytest.mark.gpu

CHUNK = 32768
OK, ERROR, INVALID_BLOCK_HEADER, DST_TOO_SMALL, SRC_TOO_SMALL, INVALID_DISTANCE = 0, 1, 2, 4, 5, 7
SIZES = (0, 1, 100, 32767, 32768, 32769, 64 << 10, (1 << 20) + 7, 3 << 20)


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


def _content(kind, n, seed):
    if kind == "text":
        return synth.gen_text(n, seed=seed)
    if kind == "random":
        return synth.gen_random(n, seed=seed)
    return np.repeat(np.random.default_rng(seed).integers(0, 256, n // 97 + 1, dtype=np.uint8), 97)[:n].copy()  # runs


def _items(sizes, seed=0):
    kinds = ("text", "random", "runs")
    return [_content(kinds[(i + seed) % 3], n, seed * 100 + i) for i, n in enumerate(sizes)]


def _nseg(n):
    return max(1, -(-n // CHUNK))


def _dev(arrays):
    return [torch.from_numpy(np.array(a, dtype=np.uint8)).cuda() if len(a) else torch.empty(0, dtype=torch.uint8, device="cuda")
            for a in arrays]


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
def test_round_trip_host_and_device(comp, container):
    items = _items(SIZES, seed=1)
    streams = comp.compress_batch(items, container=container)
    idx, sub, bb = comp.last_batch_index()
    assert len(bb) == len(items)
    assert idx.size == sum(_nseg(n) + 1 for n in SIZES) and sub.size == sum(_nseg(n) for n in SIZES) * 64
    sizes = [a.size for a in items]
    for use_sub in (False, True):
        outs, st = comp.decompress_batch(streams, sizes, index=idx, subindex=sub if use_sub else None, block_bytes=bb,
                                         container=container)
        assert st == [0] * len(items)
        for o, a in zip(outs, items):
            assert o == a.tobytes()
        touts, tst = comp.decompress_batch_tensors(_dev([np.frombuffer(s, np.uint8) for s in streams]), sizes,
                                                   index=torch.from_numpy(idx.astype(np.int64)).cuda(),
                                                   subindex=torch.from_numpy(sub.view(np.int32)).cuda() if use_sub else None,
                                                   block_bytes=bb, container=container)
        torch.cuda.synchronize()
        assert tst.cpu().tolist() == [0] * len(items)
        for o, a in zip(touts, items):
            assert o[: a.size].cpu().numpy().tobytes() == a.tobytes()


@pytest.mark.parametrize("effort, block_bytes", [("fast", 0), ("fastest", 0), ("thorough", 262144), ("max", 0), ("best", 0),
                                                 ("ultra", 262144), ("extreme", 0), ("chain4", 0), ("recent", 0),
                                                 ("recent_all", 32768), ("default", 262144)])
def test_round_trip_efforts_and_strips(comp, effort, block_bytes):
    sizes = (5, 40000, 300000, (1 << 20) + 3)
    items = _items(sizes, seed=2)
    streams = comp.compress_batch(items, effort=effort, block_bytes=block_bytes)
    idx, sub, bb = comp.last_batch_index()
    for use_sub in (False, True):
        outs, st = comp.decompress_batch(streams, sizes, index=idx, subindex=sub if use_sub else None, block_bytes=bb)
        assert st == [0] * len(items)
        assert outs == [a.tobytes() for a in items]


def _single(comp, stream, ix, sb, n, bb):
    """sfh_decompress_device on one item alone -> (bytes, status)"""
    out, st = comp.decompress_tensor(_dev([np.frombuffer(stream, np.uint8)])[0], torch.from_numpy(ix.astype(np.int64)).cuda(), n,
                                     out=torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda"),
                                     subindex=None if sb is None else torch.from_numpy(sb.view(np.int32)).cuda(), block_bytes=bb)
    torch.cuda.synchronize()
    return out[:n].cpu().numpy().tobytes(), st


def test_raw_items_equal_the_single_call_damaged_ones_included(comp):
    """(The single call is a batch of one item: beside it stand the statuses the implicit-geometry single call of the commit
    before that gave for these items, tests/golden/single_decode_parent.json.)"""
    sizes, items, streams, idx, sub, bb, per = damaged_batch(comp)
    recorded = parent_record()["batch_want_st"]["damaged"]
    for use_sub in (False, True):
        s_arg = sub if use_sub else None
        touts, tst = comp.decompress_batch_tensors(_dev([np.frombuffer(s, np.uint8) for s in streams]), sizes,
                                                   index=torch.from_numpy(idx.astype(np.int64)).cuda(),
                                                   subindex=None if s_arg is None else torch.from_numpy(s_arg.view(np.int32)).cuda(),
                                                   block_bytes=bb,
                                                   outs=[torch.zeros(n, dtype=torch.uint8, device="cuda") for n in sizes])
        torch.cuda.synchronize()
        st = tst.cpu().tolist()
        for i, n in enumerate(sizes):
            want_b, want_st = _single(comp, streams[i], per[i][0], per[i][1] if use_sub else None, n, int(bb[i]))
            assert st[i] == want_st, (i, use_sub)
            assert touts[i][:n].cpu().numpy().tobytes() == want_b, (i, use_sub)
        assert st == recorded[str(use_sub).lower()], use_sub
        assert st[0] == 0 and st[5] == 0 and st[2] != 0 and (st[3] != 0) == use_sub
        assert st[1] != 0 or touts[1].cpu().numpy().tobytes() != items[1].tobytes()  # (a flipped byte may still decode)
        assert st[4] == INVALID_DISTANCE


def test_raw_items_with_a_first_entry_past_0(comp):
    """A wrapped stream decoded as a raw body through its index (entry 0 = the header's end), and a damaged entry 0: a raw
    item's status is the single call's, which does not look at where entry 0 lies.  (Beside the single call, a batch of one
    item, stand the statuses recorded from the commit before it became one.)"""
    sizes, items, streams, idx, sub, bb, per = first_entry_batch(comp)
    recorded = parent_record()["batch_want_st"]["first_entry"]
    for use_sub in (False, True):
        outs, st = comp.decompress_batch(streams, sizes, index=idx, subindex=sub if use_sub else None, block_bytes=bb)
        for i, n in enumerate(sizes):
            want_b, want_st = _single(comp, streams[i], per[i][0], per[i][1] if use_sub else None, n, int(bb[i]))
            assert st[i] == want_st, (i, use_sub)
            if want_st == 0:
                assert outs[i] == want_b
        assert st == recorded[str(use_sub).lower()], use_sub
        assert st[0] == 0 and st[1] == 0 and outs[0] == items[0].tobytes()


def test_isolation_and_canaries(comp):
    sizes = (40000, 1000, 90000, 32768, 5000)
    items = _items(sizes, seed=4)
    streams = [bytearray(s) for s in comp.compress_batch(items, container="zlib")]
    idx, _, bb = comp.last_batch_index()
    streams[1][len(streams[1]) // 2] ^= 0xFF
    streams[3][-1] ^= 1
    gap = 4096
    offs, at = [], gap
    for n in sizes:
        offs.append(at)
        at = (at + n + gap + 15) // 16 * 16
    big = torch.full((at + gap,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = [big[o: o + n] for o, n in zip(offs, sizes)]
    _, tst = comp.decompress_batch_tensors(_dev([np.frombuffer(bytes(s), np.uint8) for s in streams]), sizes,
                                           index=torch.from_numpy(idx.astype(np.int64)).cuda(), block_bytes=bb,
                                           container="zlib", outs=outs)
    torch.cuda.synchronize()
    st = tst.cpu().tolist()
    assert st[0] == st[2] == st[4] == 0 and st[1] != 0 and st[3] == ERROR
    host = big.cpu().numpy()
    for i in (0, 2, 4):
        assert host[offs[i]: offs[i] + sizes[i]].tobytes() == items[i].tobytes()
    mask = np.ones(host.size, bool)
    for o, n in zip(offs, sizes):
        mask[o: o + n] = False
    assert (host[mask] == 0xA5).all()


def _gzip(raw_body, data, flags=0, extra=b"", name=b"", comment=b"", fix=None):
    hdr = bytearray([0x1F, 0x8B, 8, flags, 0, 0, 0, 0, 0, 3])
    if flags & 4:
        hdr += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        hdr += name + b"\0"
    if flags & 16:
        hdr += comment + b"\0"
    if flags & 2:
        hdr += struct.pack("<H", zlib.crc32(bytes(hdr)) & 0xFFFF)
    return bytes(hdr) + raw_body + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def _raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def test_container_failures(comp):
    text = synth.gen_text(20000, seed=5).tobytes()
    z = zlib.compress(text, 6)
    g = _gzip(_raw_deflate(text), text)
    cases = []  # (container, stream, dst_n, expected status: container.hpp's)
    cases.append(("zlib", z, len(text), OK))
    cases.append(("zlib", bytes([z[0] ^ 0x01]) + z[1:], len(text), ERROR))                # header: CM / FCHECK
    cases.append(("zlib", z[:-1] + bytes([z[-1] ^ 0x10]), len(text), ERROR))              # Adler-32
    cases.append(("zlib", z[:5], len(text), SRC_TOO_SMALL))                               # shorter than its wrapper
    cases.append(("gzip", g, len(text), OK))
    cases.append(("gzip", bytes([0x1E]) + g[1:], len(text), ERROR))                        # magic
    cases.append(("gzip", g[:-8] + bytes([g[-8] ^ 4]) + g[-7:], len(text), ERROR))        # CRC-32
    cases.append(("gzip", g[:-4] + struct.pack("<I", len(text) + 1), len(text), DST_TOO_SMALL))  # ISIZE + 1
    cases.append(("gzip", g[:-4] + struct.pack("<I", len(text) - 1), len(text), DST_TOO_SMALL))  # ISIZE - 1
    cases.append(("gzip", g[:17], len(text), SRC_TOO_SMALL))
    # a stored body damaged together with its checksum: the checksum of the damaged bytes is what fails
    zs = bytearray(zlib.compress(text, 0))
    zs[100] ^= 0x20
    cases.append(("zlib", bytes(zs), len(text), ERROR))
    zs2 = bytearray(zs)
    zs2[-4:] = struct.pack(">I", zlib.adler32(zlib.decompressobj(-15).decompress(bytes(zs[2:-4]))))
    cases.append(("zlib", bytes(zs2), len(text), OK))  # (the body is a stored block: the damage is data, the checksum agrees)
    # a body that fails -- BTYPE 3 in its first block header -- reports the body's status, with or without a damaged checksum
    for container, stream in (("zlib", z), ("gzip", g)):
        h = 2 if container == "zlib" else 10
        t = 4 if container == "zlib" else 8
        bad = bytearray(stream)
        bad[h] |= 0x06
        cases.append((container, bytes(bad), len(text), INVALID_BLOCK_HEADER))
        bad[len(bad) - t] ^= 0x40
        cases.append((container, bytes(bad), len(text), INVALID_BLOCK_HEADER))
    # gzip with ISIZE below the output size decodes into the first ISIZE bytes, as container.hpp does: a body of exactly ISIZE
    # bytes is a success
    short = text[:15000]
    cases.append(("gzip", _gzip(_raw_deflate(short), short), len(text), OK))
    for container in ("zlib", "gzip"):
        sel = [c for c in cases if c[0] == container]
        outs, st = comp.decompress_batch([c[1] for c in sel], [c[2] for c in sel], container=container)
        assert st == [c[3] for c in sel], container
        assert outs[0] == text


def test_foreign_pages_without_an_index(comp):
    rng = np.random.default_rng(6)
    pages, sizes = [], []
    text = synth.gen_text(1 << 20, seed=6).tobytes()
    for k, n in enumerate([0, 1, 7, 100, 4096, 10000, 32767, 32768] * 3):
        data = text[k * 3000: k * 3000 + n] if k % 3 else bytes(rng.integers(0, 256, n, dtype=np.uint8))
        level = (0, 1, 6, 9)[k % 4]
        strategy = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)[(k // 4) % 4]
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 1 if k % 5 == 0 else 8, strategy)  # memLevel 1: many blocks
        pages.append(c.compress(data) + c.flush())
        sizes.append(len(data))
    outs, st = comp.decompress_batch(pages, sizes, container="zlib")
    assert st == [0] * len(pages)
    assert outs == [zlib.decompress(p) for p in pages]
    data = text[:20000]
    gz = [_gzip(_raw_deflate(data), data, flags=f, extra=b"xy" * 9, name=b"page.txt", comment=b"a comment")
          for f in (0, 2, 4, 8, 16, 30)]
    outs, st = comp.decompress_batch(gz, [len(data)] * len(gz), container="gzip")
    assert st == [0] * len(gz) and outs == [data] * len(gz)
    raw = [_raw_deflate(text[i * 4096: i * 4096 + 4096], 6) for i in range(8)]
    outs, st = comp.decompress_batch(raw, [4096] * 8)
    assert st == [0] * 8 and outs == [text[i * 4096: i * 4096 + 4096] for i in range(8)]


def test_ten_thousand_pages(comp):
    text = synth.gen_text(4096 * 10000, seed=7).tobytes()
    pages = [zlib.compress(text[i * 4096: (i + 1) * 4096], 6) for i in range(10000)]
    outs, st = comp.decompress_batch(pages, [4096] * 10000, container="zlib")
    assert st == [0] * 10000
    assert b"".join(outs) == text


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from starflate_amd import Compressor, synth
c = Compressor(0)
sizes = (3, 70000, 200000, (1 << 20) + 5, 40000, 600000)
items = [synth.gen_text(n, seed=i) for i, n in enumerate(sizes)]
res = []
for bb in (0, 262144):
    for container in ("raw", "gzip"):
        streams = c.compress_batch(items, block_bytes=bb, container=container)
        idx, sub, bbs = c.last_batch_index()
        res.append(idx.tobytes() + sub.tobytes() + bbs.tobytes())
        for s in (None, sub):
            outs, st = c.decompress_batch(streams, sizes, index=idx, subindex=s, block_bytes=bbs, container=container)
            assert st == [0] * len(sizes), st
            assert outs == [a.tobytes() for a in items]
            res.append(b"".join(outs))
import hashlib
print(hashlib.sha256(b"".join(res)).hexdigest())
"""


def test_launch_batches_match_the_default():
    def run(env):
        e = dict(os.environ)
        e.pop("SFH_BATCH_CHUNKS", None)
        e.update(env)
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=600, env=e)
        assert p.returncode == 0, p.stderr[-2000:]
        return p.stdout.strip()
    assert run({"SFH_BATCH_CHUNKS": "4"}) == run({})


def test_an_item_is_cut_where_its_strips_do_not_divide_the_cap():
    """Strips of three segments under a cap of eight: an item is cut at max(sps, cap / sps * sps) = 6 segments, the single
    call's rule (sf_inflate_plan.h), so the item of seven, which would fit the cap whole, is a batch of six and a batch of one,
    and no batch of this call is wider than six (the token scratch says so).  Around it: an item in front, which shares no
    batch with it, a short last strip, and items that do not fit the batch open before them."""
    bb = 3 * CHUNK
    sizes = (1000, 7 * CHUNK - 5, 2 * CHUNK + 1, 6 * CHUNK, 4 * CHUNK)
    items = [synth.gen_text(n, seed=70 + i) for i, n in enumerate(sizes)]
    c = context_under(SFH_BATCH_CHUNKS="8")
    try:
        streams = c.compress_batch(items, block_bytes=bb)
        idx, sub, bbs = c.last_batch_index()
        assert bbs.tolist() == [bb] * len(sizes)
        for s in (None, sub):
            outs, st = c.decompress_batch(streams, sizes, index=idx, subindex=s, block_bytes=bbs)
            assert st == [0] * len(sizes)
            assert outs == [a.tobytes() for a in items]
            assert c.last_decode_scratch_bytes() == 6 * CHUNK * 4
    finally:
        c.close()


def test_async_ordering_and_index_state(comp):
    sizes = (1000, 50000, 400000)
    items = _items(sizes, seed=8)
    s = torch.cuda.Stream()
    streams = comp.compress_batch(items)
    idx, sub, bb = comp.last_batch_index()
    dstreams = _dev([np.frombuffer(x, np.uint8) for x in streams])
    didx = torch.from_numpy(idx.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        results = [comp.decompress_batch_tensors(dstreams, sizes, index=didx, block_bytes=bb, stream=s.cuda_stream) for _ in range(3)]
    s.synchronize()
    for outs, st in results:
        assert st.cpu().tolist() == [0] * 3
        assert [o[:n].cpu().numpy().tobytes() for o, n in zip(outs, sizes)] == [a.tobytes() for a in items]
    # the index-state rules: a batch decompress leaves no index of either kind; a batch compress has a batch index only;
    # a single compress has a single index only
    lib = comp._lib
    items_n, entries = C.c_size_t(0), C.c_size_t(0)
    assert lib.sfh_batch_index_size(comp._h, C.byref(items_n), C.byref(entries)) == -1
    assert lib.sfh_index_entries(comp._h) == 0
    one = comp.compress(items[1].tobytes())
    assert lib.sfh_batch_index_size(comp._h, C.byref(items_n), C.byref(entries)) == -1
    ix1, bb1 = comp.last_index(), comp.last_block_bytes()
    comp.compress_batch(items)
    assert lib.sfh_index_entries(comp._h) == 0
    assert lib.sfh_batch_index_size(comp._h, C.byref(items_n), C.byref(entries)) == 0
    assert (items_n.value, entries.value) == (3, sum(_nseg(n) + 1 for n in sizes))
    out, st = comp.decompress(one, ix1, sizes[1], block_bytes=bb1)
    assert st == 0 and out == items[1].tobytes()
    assert lib.sfh_batch_index_size(comp._h, C.byref(items_n), C.byref(entries)) == -1


def test_refusals_write_nothing(comp):
    lib = comp._lib
    data = synth.gen_text(50000, seed=9).tobytes()
    z = zlib.compress(data)
    src = _dev([np.frombuffer(z, np.uint8)])[0]
    dst = torch.full((1 << 17,), 7, dtype=torch.uint8, device="cuda")
    st = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    k = 2
    vp = C.c_void_p
    n = (C.c_uint64 * k)(len(z), len(z))

    def call(dsts, dst_n, index=None, sub=None, status=st.data_ptr()):
        return lib.sfh_decompress_batch_device_async(comp._h, k, (vp * k)(src.data_ptr(), src.data_ptr()), n, index, sub,
                                                     (vp * k)(*dsts), (C.c_uint64 * k)(*dst_n), None, 1, vp(status), None)

    base = dst.data_ptr()
    assert call([base, base + 16384], [20000, 20000]) == -1                      # overlap
    assert call([base + 8, base + 65536], [100, 100]) == -1                      # dst alignment
    assert call([base, base + 65536], [100, 100], status=st.data_ptr() + 2) == -1  # status alignment
    assert call([base, base + 65536], [50000, 100]) == -1                        # no index, an item above 32 KiB
    sub = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert call([base, base + 65536], [100, 100], sub=sub.data_ptr()) == -1      # a sub-index without an index
    ix = torch.tensor([2, len(z) - 4, 2, len(z) - 4, 0], dtype=torch.int64, device="cuda")
    assert call([base, base + 65536], [100, 100], index=ix.data_ptr() + 4) == -1  # index alignment
    assert lib.sfh_decompress_batch_device_async(comp._h, k, (vp * k)(src.data_ptr() + 2, src.data_ptr()), n, None, None,
                                                 (vp * k)(base, base + 65536), (C.c_uint64 * k)(100, 100), None, 1,
                                                 vp(st.data_ptr()), None) == -1  # src alignment
    # with a context: null arrays, an unknown container (also with count == 0)
    assert lib.sfh_decompress_batch_device_async(comp._h, k, None, None, None, None, None, None, None, 1, None, None) == -1
    assert lib.sfh_decompress_batch(comp._h, k, None, None, None, None, None, None, None, 1, None) == -1
    assert lib.sfh_decompress_batch_device_async(comp._h, 0, None, None, None, None, None, None, None, 3, None, None) == -1
    assert lib.sfh_decompress_batch(comp._h, 0, None, None, None, None, None, None, None, 3, None) == -1
    assert lib.sfh_decompress_batch_device_async(comp._h, k, (vp * k)(src.data_ptr(), src.data_ptr()), n, None, None,
                                                 (vp * k)(base, base + 65536), (C.c_uint64 * k)(100, 100), None, 3,
                                                 vp(st.data_ptr()), None) == -1
    torch.cuda.synchronize()
    assert (dst == 7).all() and (st == -1).all()
    assert lib.sfh_decompress_batch_device_async(comp._h, 0, None, None, None, None, None, None, None, 1, None, None) == 0
    # a destination of no bytes, even inside another item's range, overlaps nothing
    assert call([base, base + 16], [100, 0]) == 0
    torch.cuda.synchronize()
    assert (st[:2] != -1).all()


def test_cpp_decompress_batch(tmp_path):
    from conftest import GOLDEN
    from starflate_amd import build

    lib = build.build()
    exe = tmp_path / "decompress_batch"
    libdir = os.path.dirname(lib)
    clang = "/opt/rocm/llvm/bin/clang++"
    flags = ["-std=c++23", "-fno-exceptions", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror", "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call([clang, "-O2"] + flags + [os.path.join(ROOT, "tests", "cpp", "decompress_batch.cpp"), "-L" + libdir,
                                                   "-lstarflate_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = subprocess.run([str(exe), GOLDEN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
