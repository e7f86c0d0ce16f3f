"""Many block-flushed streams decoded in one call with no side information (sfh_recover_index_batch*,
sfh_decompress_any_batch*).  The expected values are never the batch's own: the bytes are the inputs, every
item's status and size are sfh_decompress_any_device's on that item alone, and the recovered index is the Python walk rule's
(unindexed_walk.recover_index) on that item."""
import ctypes as C
import gzip
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import starflate_amd
import unindexed_walk as W
from starflate_amd import Compressor, _capi, synth

pytestmark = pytest.mark.gpu

SEG = 32768
OK, ERROR, DST_TOO_SMALL = 0, 1, 4
NOT_INDEXABLE = starflate_amd.ITEM_NOT_INDEXABLE
TRAILER = _capi.SIZE_FROM_TRAILER
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
KIND = {"raw": 0, "zlib": 1, "gzip": 2}
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


def _data(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "text":
        return synth.gen_text(n, seed=seed)
    if kind == "noise":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    d = synth.gen_text(n, seed=seed)  # noise-head chunks: every 32 KiB chunk starts with 8 KiB of noise, then text
    for c0 in range(0, n, SEG):
        m = min(8192, n - c0)
        d[c0:c0 + m] = rng.integers(0, 256, m, dtype=np.uint8)
    return d


def nseg_of(n):
    return max(1, -(-n // SEG))


def single(comp, stream, want, container, cap=None):
    """sfh_decompress_any_device on one item alone -> (status, or NOT_INDEXABLE for SFH_E_NOT_INDEXABLE; its destination of
    cap bytes, which were FILL before)"""
    size = want if want != TRAILER else (int.from_bytes(stream[-4:], "little") if len(stream) >= 18 else 0)
    cap = size if cap is None else cap
    if size > cap:  # the single device call knows no capacity: the issue's rule for the batch is DstTooSmall, nothing written
        return DST_TOO_SMALL, bytes([FILL]) * cap
    src = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda() if stream else torch.zeros(4, dtype=torch.uint8, device="cuda")
    dst = torch.full((max(cap, 1) + 16,), FILL, dtype=torch.uint8, device="cuda")
    st = C.c_uint32(0)
    s = torch.cuda.current_stream().cuda_stream
    rc = comp._lib.sfh_decompress_any_device(comp._h, src.data_ptr(), len(stream), KIND[container], dst.data_ptr(), want, C.byref(st),
                                             C.c_void_p(s))
    torch.cuda.synchronize()
    assert rc in (0, -8), comp.last_error()
    return (NOT_INDEXABLE if rc else st.value), dst[:cap].cpu().numpy().tobytes()


def batch(comp, streams, wants, container, caps=None, gran=16, c=None):
    """sfh_decompress_any_batch_device over sources packed into one buffer at `gran` bytes and destinations of caps[i] bytes
    in one buffer, each between guards -> (statuses, sizes, destinations); asserts the guards"""
    c = c or comp
    k = len(streams)
    sizes = [w if w != TRAILER else (int.from_bytes(s[-4:], "little") if len(s) >= 18 else 0) for s, w in zip(streams, wants)]
    caps = list(sizes) if caps is None else caps
    s_off, at = [], 0
    for s in streams:
        s_off.append(at)
        at = (at + len(s) + gran - 1) // gran * gran
    src = np.zeros(at + 16, np.uint8)
    for o, s in zip(s_off, streams):
        src[o:o + len(s)] = np.frombuffer(s, np.uint8)
    d_off, at = [], GUARD
    for m in caps:
        d_off.append(at)
        at = (at + m + 15) // 16 * 16 + GUARD
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((at,), FILL, dtype=torch.uint8, device="cuda")
    sp = (C.c_void_p * k)(*[d_src.data_ptr() + o for o in s_off])
    dp = (C.c_void_p * k)(*[d_dst.data_ptr() + o for o in d_off])
    out_n = (C.c_uint64 * k)()
    st = (C.c_uint32 * k)()
    rc = c._lib.sfh_decompress_any_batch_device(c._h, k, sp, (C.c_uint64 * k)(*[len(s) for s in streams]), KIND[container], dp,
                                                (C.c_uint64 * k)(*caps), (C.c_uint64 * k)(*wants), out_n, st,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, c.last_error()
    h = d_dst.cpu().numpy()
    keep = np.ones(at, bool)
    for o, m in zip(d_off, caps):
        keep[o:o + m] = False
    assert (h[keep] == FILL).all(), "a byte outside every destination was written"
    return list(st), list(out_n), [h[o:o + m].tobytes() for o, m in zip(d_off, caps)]


def agree(comp, streams, wants, container, datas=None, caps=None, gran=16, c=None):
    """the batch against the single call, item by item; datas[i] (where given): the input the item must decode to"""
    st, out_n, dst = batch(comp, streams, wants, container, caps, gran, c)
    rows, rows1 = (c or comp).last_recover_stats()["rows"], 0
    nodes, nodes1 = (c or comp).last_recover_stats()["nodes"], 0
    for i, (s, w) in enumerate(zip(streams, wants)):
        s1, d1 = single(comp, s, w, container, None if caps is None else caps[i])
        rows1 += comp.last_recover_stats()["rows"] if s1 not in (NOT_INDEXABLE, DST_TOO_SMALL) else 0
        nodes1 += comp.last_recover_stats()["nodes"] if s1 != DST_TOO_SMALL else 0
        assert st[i] == s1, (i, st[i], s1)
        if s1 == OK:
            assert dst[i] == d1, i
        elif d1 == bytes([FILL]) * len(d1):
            assert dst[i] == d1, f"item {i}: a failed item's destination was written where the single call leaves it alone"
        if datas is not None and datas[i] is not None:
            assert st[i] == OK and dst[i][:out_n[i]] == datas[i] and out_n[i] == len(datas[i]), i
    if container == "raw":  # (a raw stream has no wrapper to fail: every single call got as far as its own count)
        assert rows == rows1, "rows of dependent segments: the batch against the single calls"
        assert nodes == nodes1, "nodes of the walk: the batch against the single calls"
    return st, out_n, dst


def recovered(comp, streams, sizes, container):
    ts = [torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda() if s else torch.zeros(0, dtype=torch.uint8, device="cuda")
          for s in streams]
    ix, st = comp.recover_index_batch(ts, sizes, container)
    ix = ix.cpu().numpy().astype(np.uint64)
    out, at = [], 0
    for n in sizes:
        out.append(ix[at:at + nseg_of(n) + 1].tolist())
        at += nseg_of(n) + 1
    assert at == ix.size
    return out, st


def walk(stream, n, container):
    try:
        return W.recover_index(stream, n, container)
    except W.NotIndexable:
        return None


# ---- 1. mixed sizes and contents, every container ----
MIXED_SIZES = (0, 1, 32767, 32768, 32769, 65537, 200 << 10, (1 << 20) + 7)
MIXED_KINDS = ("text", "noise", "zeros", "noisehead")


@pytest.fixture(scope="module")
def mixed(comp):
    datas = [_data(kind, n, 7 * j + 1) for j, n in enumerate(MIXED_SIZES) for kind in MIXED_KINDS]
    return datas, {cont: comp.compress_batch(datas, container=cont) for cont in KIND}


@pytest.mark.parametrize("container, trailer", [("raw", False), ("zlib", False), ("gzip", False), ("gzip", True)])
def test_mixed_batch(comp, mixed, container, trailer):
    datas, streams = mixed
    streams = streams[container]
    sizes = [d.size for d in datas]
    agree(comp, streams, [TRAILER] * len(sizes) if trailer else sizes, container, [d.tobytes() for d in datas])
    if not trailer:
        ix, st = recovered(comp, streams, sizes, container)
        assert st == [OK] * len(sizes)
        for i, s in enumerate(streams):
            assert ix[i] == W.recover_index(s, sizes[i], container), i


def test_host_buffer_calls(comp, mixed):
    datas, streams = mixed
    outs, st = comp.decompress_any_batch(streams["zlib"], [d.size for d in datas], "zlib")
    assert st == [OK] * len(datas) and outs == [d.tobytes() for d in datas]
    outs, st = comp.decompress_any_batch(streams["gzip"], None, "gzip")
    assert st == [OK] * len(datas) and outs == [d.tobytes() for d in datas]
    # sfh_recover_index_batch on host buffers: the same flat index
    sub = streams["raw"][16:]
    sizes = [d.size for d in datas][16:]
    k = len(sub)
    bufs = [np.frombuffer(s, np.uint8) for s in sub]
    entries = sum(nseg_of(n) + 1 for n in sizes)
    ix = np.full(entries, 77, np.uint64)
    st = (C.c_uint32 * k)()
    rc = comp._lib.sfh_recover_index_batch(comp._h, k, (C.c_void_p * k)(*[b.ctypes.data for b in bufs]),
                                           (C.c_uint64 * k)(*[b.size for b in bufs]), 0, (C.c_uint64 * k)(*sizes), ix.ctypes.data, st)
    assert rc == 0 and list(st) == [OK] * k
    assert ix.tolist() == [v for s, n in zip(sub, sizes) for v in W.recover_index(s, n, "raw")]


# ---- 2. sources back to back at 4-byte granularity ----
def _stream_of_length_0_mod_4(comp, **kw):
    for seed in range(64):
        d = _data("text", 2 * SEG + 1000 + seed, seed)
        s = comp.compress(d, **kw)
        if len(s) % 4 == 0:
            return d, s
    raise AssertionError("no stream of a length that is a multiple of 4")


def _stream_with_a_marker_at_2_mod_4(comp):
    for seed in range(64):
        d = _data("text", 4 * SEG + 100 + seed, 200 + seed)
        s = comp.compress(d)
        for p in range(len(s) - 4):
            if s[p:p + 4] == b"\x00\x00\xff\xff" and (p + 2) % 4 == 0:
                return d, s, s[:p + 2]
    raise AssertionError("no flush marker at an offset of 2 modulo 4")


def test_packed_sources(comp):
    items = []  # (stream, size, data or None)
    # a final_stream=0 item ends in 00 00 FF FF, directly in front of the next item
    d, s = _stream_of_length_0_mod_4(comp, final_stream=False)
    assert s.endswith(b"\x00\x00\xff\xff")
    items.append((s, d.size, None))  # (its last segment has no final block: whatever the single call says)
    d2 = _data("text", 3 * SEG + 5, 90)
    items.append((comp.compress(d2), d2.size, d2.tobytes()))
    # an item cut so that it ends in 00 00, directly in front of one that begins FF FF
    d3, s3, front = _stream_with_a_marker_at_2_mod_4(comp)
    assert front.endswith(b"\x00\x00") and len(front) % 4 == 0 and s3[len(front):len(front) + 2] == b"\xff\xff"
    items.append((front, d3.size, None))
    items.append((s3[len(front):], d3.size, None))
    items.append((comp.compress(d2, strategy="fixed"), d2.size, d2.tobytes()))
    # stored payloads whose fake markers and fake stored headers straddle the scan's 8 KiB waves
    rng = np.random.default_rng(5)
    for off in range(8186, 8193):  # the pattern's first byte in the stream: markers end at 8190..8196, headers start at 8186..8192
        for pat in (b"\x00\x00\xff\xff", b"\x00\x00\x80\xff\x7f", b"\x01\x00\x80\xff\x7f"):
            d = rng.integers(1, 255, 3 * SEG + 40, dtype=np.uint8)
            d[off - 5:off - 5 + len(pat)] = np.frombuffer(pat, np.uint8)  # (the stream's first stored header takes 5 bytes)
            s = comp.compress(d, strategy="stored")
            assert s[off:off + len(pat)] == pat
            items.append((s, d.size, d.tobytes()))
    streams, sizes, datas = [i[0] for i in items], [i[1] for i in items], [i[2] for i in items]
    assert len(streams[0]) % 4 == 0 and len(streams[2]) % 4 == 0  # (the item behind each begins on its last byte's heels)
    agree(comp, streams, sizes, "raw", datas, gran=4)
    ix, rst = recovered(comp, streams, sizes, "raw")
    for i, s in enumerate(streams):
        want = walk(s, sizes[i], "raw")
        assert (rst[i] == OK) == (want is not None), i
        if want is not None:
            assert ix[i] == want, i


# ---- 3. adversarial stored payloads beside clean items ----
def test_adversarial_items_beside_clean_ones(comp):
    rng = np.random.default_rng(11)
    bad = rng.integers(0, 256, 8 * SEG + 77, dtype=np.uint8)
    for off in range(123, bad.size - 8, 300):
        bad[off:off + 4] = (0, 0, 0xFF, 0xFF)
    for off in range(250, bad.size - 8, 700):
        bad[off:off + 5] = (rng.integers(0, 2), 0, 0x80, 0xFF, 0x7F)
    clean = [_data("text", 3 * SEG + 9, 1), _data("zeros", 2 * SEG, 2), _data("noisehead", 5 * SEG - 1, 3)]
    datas = [clean[0], bad, clean[1], bad, clean[2]]
    streams = [comp.compress(clean[0]), comp.compress(bad, strategy="stored"), comp.compress(clean[1]), comp.compress(bad),
               comp.compress(clean[2])]
    sizes = [d.size for d in datas]
    agree(comp, streams, sizes, "raw", [d.tobytes() for d in datas], gran=4)
    ix, st = recovered(comp, streams, sizes, "raw")
    assert st == [OK] * 5
    assert comp.last_recover_stats()["nodes"] > 2 * 8 * 100
    for i, s in enumerate(streams):
        assert ix[i] == W.recover_index(s, sizes[i], "raw"), i


# ---- 4. isolation ----
def test_isolation_zlib(comp):
    good = [_data(k, n, j) for j, (k, n) in enumerate([("text", 3 * SEG + 1), ("noise", 2 * SEG + 7), ("zeros", 70000), ("text", 100)])]
    gs = comp.compress_batch(good, container="zlib")
    d = _data("text", 4 * SEG + 5, 20).tobytes()
    unflushed = zlib.compress(d, 6)
    damaged = bytearray(gs[0])
    damaged[len(damaged) // 2] ^= 0x10
    bad_adler = gs[1][:-1] + bytes([gs[1][-1] ^ 0x40])
    sync_only = W.zlib_flushed(d, 6, zlib.Z_SYNC_FLUSH, 15, True)
    streams = [gs[0], unflushed, gs[1], bytes(damaged), gs[2], bad_adler, sync_only, gs[3]]
    sizes = [good[0].size, len(d), good[1].size, good[0].size, good[2].size, good[1].size, len(d), good[3].size]
    datas = [good[0].tobytes(), None, good[1].tobytes(), None, good[2].tobytes(), None, d, good[3].tobytes()]
    st, _, _ = agree(comp, streams, sizes, "zlib", datas)
    assert st[1] == NOT_INDEXABLE and st[3] != OK and st[5] == ERROR


def test_isolation_gzip_sizes_from_the_trailer(comp):
    good = [_data(k, n, j) for j, (k, n) in enumerate([("text", 3 * SEG + 1), ("noisehead", 2 * SEG + 7), ("text", 0)])]
    gs = comp.compress_batch(good, container="gzip")
    d = _data("text", 4 * SEG + 5, 21).tobytes()
    unflushed = gzip.compress(d, 6)
    damaged = bytearray(gs[0])
    damaged[len(damaged) // 3] ^= 0x01
    not_gzip = b"\x1f\x8c" + gs[1][2:]
    streams = [gs[0], gs[1], unflushed, gs[1], bytes(damaged), gs[2], not_gzip, gs[0]]
    caps = [good[0].size, good[1].size - 1, len(d), good[1].size + 100, good[0].size, 0, good[1].size, good[0].size + 16]
    datas = [good[0].tobytes(), None, None, good[1].tobytes(), None, b"", None, good[0].tobytes()]
    st, out_n, _ = agree(comp, streams, [TRAILER] * len(streams), "gzip", datas, caps=caps)
    assert st[1] == DST_TOO_SMALL and st[2] == NOT_INDEXABLE and st[4] != OK and st[6] == ERROR
    # explicit sizes: one above its capacity is that item's DstTooSmall
    sizes = [good[0].size, good[1].size, len(d), good[1].size, good[0].size, 0, good[1].size, good[0].size]
    caps = [good[0].size, good[1].size - 1, len(d), good[1].size, good[0].size, 0, good[1].size, good[0].size]
    st, _, dst = batch(comp, streams, sizes, "gzip", caps=caps)
    assert st[1] == DST_TOO_SMALL and dst[1] == bytes([FILL]) * caps[1]
    assert [st[i] for i in (0, 3, 5, 7)] == [OK] * 4 and dst[3] == good[1].tobytes()


# ---- 5. small launch batches ----
def test_small_launch_batches(comp):
    segs = [1, 3, 4, 2, 2, 5, 1, 3, 2, 9, 1]
    datas = [_data(("text", "noisehead", "zeros")[j % 3], n * SEG - (j % 2) * 100, j) for j, n in enumerate(segs)]
    streams = comp.compress_batch(datas, container="zlib")
    sizes = [d.size for d in datas]
    want = batch(comp, streams, sizes, "zlib")
    assert want[0] == [OK] * len(segs) and want[2] == [d.tobytes() for d in datas]
    assert comp.last_decode_scratch_bytes() == sum(segs) * SEG * 4
    old = os.environ.get("SFH_BATCH_CHUNKS")
    os.environ["SFH_BATCH_CHUNKS"] = "4"
    try:
        small = Compressor(0)
    finally:
        if old is None:
            del os.environ["SFH_BATCH_CHUNKS"]
        else:
            os.environ["SFH_BATCH_CHUNKS"] = old
    try:
        small.set_profiling(True)
        got = batch(comp, streams, sizes, "zlib", c=small)
        assert got == want
        assert small.last_decode_scratch_bytes() == 9 * SEG * 4  # the widest batch (the item above the cap, alone), not the call
        assert small.last_recover_stats()["rows"] == comp.last_recover_stats()["rows"]
        assert all(v > 0 for v in small.inflate_ms().values())  # (summed over the launch batches)
    finally:
        small.close()


# ---- 6. the Python surface ----
def test_module_level_fallback():
    datas = [_data("text", n, n).tobytes() for n in (5, 40000, 3 * SEG + 1, 100000)]
    flushed = starflate_amd.compress_batch(datas, container="gzip")
    plain = [gzip.compress(d, 6) for d in datas]
    streams = [flushed[0], plain[1], flushed[2], plain[3], plain[0], flushed[1], plain[2], flushed[3]]
    want = [datas[0], datas[1], datas[2], datas[3], datas[0], datas[1], datas[2], datas[3]]
    outs, st = starflate_amd.decompress_any_batch(streams, container="gzip", fallback=True)
    assert st == [OK] * 8 and outs == want
    outs, st = starflate_amd.decompress_any_batch(streams, [len(d) for d in want], "gzip", fallback=False)
    # (gzip.compress of 5 bytes is one segment: any one-segment stream is indexable)
    assert st == [OK, NOT_INDEXABLE, OK, NOT_INDEXABLE, OK, OK, NOT_INDEXABLE, OK]
    assert outs == [w if s == OK else b"" for w, s in zip(want, st)]


def test_tensor_surface(comp, mixed):
    datas, streams = mixed
    ts = [torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda() for s in streams["gzip"]]
    outs, st = comp.decompress_any_batch_tensors(ts, [d.size for d in datas], "gzip")
    assert st == [OK] * len(datas)
    assert all(o.cpu().numpy().tobytes() == d.tobytes() for o, d in zip(outs, datas))
    bufs = [torch.empty(max(d.size, 1), dtype=torch.uint8, device="cuda") for d in datas]
    outs, st = comp.decompress_any_batch_tensors(ts, None, "gzip", outs=bufs)
    assert st == [OK] * len(datas)
    assert all(o.cpu().numpy().tobytes() == d.tobytes() for o, d in zip(outs, datas))
    assert comp._lib.sfh_index_entries(comp._h) == 0  # afterwards the context has no index of either kind
    items, entries = C.c_size_t(0), C.c_size_t(0)
    assert comp._lib.sfh_batch_index_size(comp._h, C.byref(items), C.byref(entries)) != 0


# ---- 8. the golden fixtures as items of a batch ----
def test_golden_as_batch_items(comp):
    with open(os.path.join(GOLDEN, "starfleet.html"), "rb") as f:
        data = f.read()
    names = ["starfleet.html.dynamic.flushed", "starfleet.html.fixed.flushed"]
    streams = []
    for name in names:
        with open(os.path.join(GOLDEN, name), "rb") as f:
            streams.append(f.read())
    streams = [streams[0], streams[1], streams[0]]
    agree(comp, streams, [len(data)] * 3, "raw", [data] * 3, gran=4)
    ix, st = recovered(comp, streams, [len(data)] * 3, "raw")
    assert st == [OK] * 3
    for got, name in zip(ix, names + names[:1]):
        assert got == np.fromfile(os.path.join(GOLDEN, name + ".index"), dtype="<u8").tolist()


# ---- what is refused before anything is enqueued, on a real context ----
def test_refusals_on_a_context(comp):
    lib, h = comp._lib, comp._h
    src = torch.zeros(256, dtype=torch.uint8, device="cuda")
    dst = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    ixb = torch.zeros(64, dtype=torch.int64, device="cuda")
    k = 2
    sp, dp = src.data_ptr(), dst.data_ptr()
    n = (C.c_uint64 * k)(8, 8)
    out = (C.c_uint64 * k)()
    st = (C.c_uint32 * k)(9, 9)

    def dec(srcs, dsts, caps, wants, container=0, count=k, src_n=n):
        return lib.sfh_decompress_any_batch_device(h, count, (C.c_void_p * k)(*srcs) if srcs else None, src_n, container,
                                                   (C.c_void_p * k)(*dsts) if dsts else None, (C.c_uint64 * k)(*caps) if caps else None,
                                                   (C.c_uint64 * k)(*wants) if wants else None, out, st, None)

    def rec(srcs, wants, ix, container=0):
        return lib.sfh_recover_index_batch_device(h, k, (C.c_void_p * k)(*srcs), n, container, (C.c_uint64 * k)(*wants), ix, st, None)

    good = ([sp, sp + 64], [dp, dp + 64], [16, 16], [16, 16])
    assert dec(*good, container=3) == -1 and dec(None, None, None, None, container=3, count=0) == -1  # an unknown container
    assert dec(None, None, None, None, count=0) == 0                                               # count == 0
    assert dec(None, good[1], good[2], good[3]) == -1 and dec(good[0], None, good[2], good[3]) == -1  # null arrays
    assert dec(good[0], good[1], None, good[3]) == -1 and dec(good[0], good[1], good[2], None) == -1
    assert dec([sp + 2, sp + 64], *good[1:]) == -1                 # source not 4-byte aligned
    assert dec(good[0], [dp + 8, dp + 64], *good[2:]) == -1        # destination not 16-byte aligned
    assert rec(good[0], [16, 16], C.c_void_p(ixb.data_ptr() + 4)) == -1  # index not 8-byte aligned
    assert rec(good[0], [16, 16], None) == -1
    assert dec(good[0], good[1], [16, (1 << 44) + 1], good[3]) == -1   # sizes above 2^44
    assert dec(good[0], good[1], good[2], [16, (1 << 44) + 1]) == -1
    assert dec(*good, src_n=(C.c_uint64 * k)(8, (1 << 44) + 1)) == -1
    assert dec(good[0], good[1], good[2], [TRAILER, 16], container=0) == -1  # the trailer's size: gzip only
    assert dec(good[0], good[1], good[2], [TRAILER, 16], container=1) == -1
    assert rec(good[0], [TRAILER, 16], C.c_void_p(ixb.data_ptr()), container=2) == -1
    assert dec(good[0], [dp, dp + 16], [32, 16], good[3]) == -1     # overlapping destinations
    # more than 2^31 - 1 segments (the sizes alone say so: nothing is read)
    m = 5  # (5 x 2^44 bytes are 5 x 2^29 segments)
    assert lib.sfh_recover_index_batch_device(h, m, (C.c_void_p * m)(*[sp] * m), (C.c_uint64 * m)(*[8] * m), 0,
                                              (C.c_uint64 * m)(*[1 << 44] * m), C.c_void_p(ixb.data_ptr()), (C.c_uint32 * m)(), None) == -1
    assert lib.sfh_decompress_any_batch_device(h, m, (C.c_void_p * m)(*[sp] * m), (C.c_uint64 * m)(*[8] * m), 0,
                                               (C.c_void_p * m)(*[dp + 16 * i for i in range(m)]), (C.c_uint64 * m)(*[16] * m),
                                               (C.c_uint64 * m)(*[1 << 44] * m), None, (C.c_uint32 * m)(), None) == 0  # (each DstTooSmall)
    # the single calls run on the same driver, which counts scan waves in 32 bits: a stream of 2^31 + 1 waves is refused
    one = C.c_uint32(9)
    assert lib.sfh_decompress_any_device(h, sp, (1 << 44) + 8192, 0, dp, 16, C.byref(one), None) == -1 and one.value == 9
    assert lib.sfh_recover_index_device(h, sp, (1 << 44) + 8192, 0, 16, C.c_void_p(ixb.data_ptr()), 1, None, None) == -1
    torch.cuda.synchronize()
    assert list(st) == [9, 9] and (dst.cpu().numpy() == FILL).all() and not ixb.cpu().numpy().any()
