"""The host-buffer entry points' one staging path (sf_capi.hip: staged_up / staged_down, host_up / host_down) on ONE context.

1. Every batched host call twice in a row: three items of 1, 32769 and 100000 bytes, then the same three in reverse order plus
   a zero-length item -- the layout changes, the device staging is regrown and reused.  The expected bytes are never the
   call's own: the inputs (what zlib decodes the streams to), the single call's and the specification's stream, the Python
   walk's index.  Destinations are filled with a byte first: behind an item's bytes, and in the whole destination of an item
   that failed, the fill must still be there.
2. A host call directly behind an asynchronous call on a caller's stream (sfh_decompress and sfh_decompress_dz: they wait for
   the context like every other host-buffer call)."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import oracle_lib as O
import unindexed_walk as W
from starflate_amd import Compressor, _capi, synth

pytestmark = pytest.mark.gpu

SEG = 32768
SIZES = (1, 32769, 100000)
FILL, GUARD = 0xA5, 32
WORDS = _capi.SUBINDEX_WORDS


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


class Item:
    """one input with its raw stream at block_bytes = 32768 (index, sub-index), and zlib's own stream of it"""

    def __init__(self, comp, n, seed):
        self.data = synth.gen_text(n, seed=seed) if n != SIZES[1] else synth.gen_mixed(n, seed=seed)
        self.n = n
        self.raw = comp.compress(self.data, block_bytes=SEG)
        self.index = comp.last_index().astype(np.uint64)
        self.sub = comp.last_subindex().astype(np.uint32).ravel()
        self.zlib = zlib.compress(self.data.tobytes(), 6)
        assert zlib.decompress(self.raw, -15) == self.data.tobytes()


class Empty:
    """the zero-length item: no input to compress; no stream to decode (a decoder's item of no source bytes fails)"""
    data = np.zeros(0, np.uint8)
    n = 0
    raw = b""


@pytest.fixture(scope="module")
def rounds(comp):
    items = [Item(comp, n, 11 + i) for i, n in enumerate(SIZES)]
    return [items, items[::-1] + [Empty()]]


def nseg_of(n):
    return max(1, -(-n // SEG))


def u64(v):
    return (C.c_uint64 * max(len(v), 1))(*v)


def ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data if a.size else None for a in arrays])


def sources(streams):
    return [np.frombuffer(s, np.uint8) for s in streams]


def filled(caps):
    return [np.full(m + GUARD, FILL, np.uint8) for m in caps]


def check_dsts(dsts, want):
    """want[i]: the bytes item i must hold, None for an item that failed -- the rest of every destination is still the fill"""
    for i, (d, w) in enumerate(zip(dsts, want)):
        w = b"" if w is None else w
        assert d[:len(w)].tobytes() == w, i
        assert (d[len(w):] == FILL).all(), f"item {i}: bytes behind its output (or of a failed item) were written"


def test_compress_batch_twice(comp, rounds):
    for items in rounds:
        k = len(items)
        srcs = [it.data for it in items]
        caps = [comp.compress_bound(it.n) for it in items]
        dsts = filled(caps)
        out_n = (C.c_uint64 * k)()
        opt = _capi.make_options()
        assert comp._lib.sfh_compress_batch(comp._h, k, ptrs(srcs), u64([it.n for it in items]), ptrs(dsts), u64(caps), out_n,
                                            C.byref(opt)) == 0, comp.last_error()
        got = [d[:out_n[i]].tobytes() for i, d in enumerate(dsts)]
        check_dsts(dsts, got)
        for it, g in zip(items, got):
            want = O.compress(it.data, O.default_params(strategy=_capi.STRATEGY["auto"], final_stream=1, lazy=3, fast_skip=1, strip_bytes=0))
            assert g == want.tobytes(), it.n
            assert zlib.decompress(g, -15) == it.data.tobytes()


def test_decompress_batch_twice(comp, rounds):
    for items in rounds:
        k = len(items)
        # the zero-length item: no source bytes for 16 bytes of output, one segment with the entries [0, 0] -- it fails
        dst_n = [it.n if it.n else 16 for it in items]
        index = np.concatenate([it.index if it.n else np.zeros(2, np.uint64) for it in items])
        sub = np.concatenate([it.sub if it.n else np.zeros(WORDS, np.uint32) for it in items])
        bb = np.full(k, SEG, np.uint32)
        srcs = sources([it.raw for it in items])
        dsts = filled(dst_n)
        st = np.full(k, 99, np.uint32)
        assert comp._lib.sfh_decompress_batch(comp._h, k, ptrs(srcs), u64([s.size for s in srcs]), index.ctypes.data, sub.ctypes.data,
                                              ptrs(dsts), u64(dst_n), bb.ctypes.data, 0, st.ctypes.data) == 0, comp.last_error()
        assert [int(v) == 0 for v in st] == [it.n > 0 for it in items], st
        check_dsts(dsts, [it.data.tobytes() if it.n else None for it in items])


def test_decompress_ranges_twice(comp):
    """the items are ranges of one stream: 1, 32769 and 100000 bytes, then the reverse with a range of no bytes -- and with the
    stream's first block header made invalid, so that the 1-byte range (alone in segment 0) fails and the others do not"""
    total = 7 * SEG + 5000
    data = synth.gen_text(total, seed=5)
    stream = np.frombuffer(comp.compress(data, block_bytes=SEG), np.uint8)
    index, sub = comp.last_index().astype(np.uint64), comp.last_subindex().astype(np.uint32).ravel()
    assert zlib.decompress(stream.tobytes(), -15) == data.tobytes() and index[0] == 0
    ranges = [(5, 1), (SEG + 7000, 32769), (3 * SEG + 1, 100000)]
    damaged = stream.copy()
    damaged[0] |= 0x06  # BTYPE = 3
    for src, rs, fails in ((stream, ranges, ()), (damaged, ranges[::-1] + [(2 * SEG, 0)], (2,))):
        k = len(rs)
        dsts = filled([ln for _, ln in rs])
        st = np.full(k, 99, np.uint32)
        assert comp._lib.sfh_decompress_ranges(comp._h, src.ctypes.data, src.size, index.ctypes.data, sub.ctypes.data, nseg_of(total),
                                               total, SEG, k, u64([o for o, _ in rs]), u64([ln for _, ln in rs]), ptrs(dsts),
                                               st.ctypes.data) == 0, comp.last_error()
        assert [int(v) != 0 for v in st] == [i in fails for i in range(k)], st
        check_dsts(dsts, [None if i in fails else data[o:o + ln].tobytes() for i, (o, ln) in enumerate(rs)])


def test_recover_index_batch_twice(comp, rounds):
    for items in rounds:
        k = len(items)
        want_n = [it.n if it.n else 16 for it in items]
        srcs = sources([it.raw for it in items])
        entries = sum(nseg_of(n) + 1 for n in want_n)
        ix = np.full(entries + 1, 77, np.uint64)  # (+1: a guard entry)
        st = (C.c_uint32 * k)(*([99] * k))
        assert comp._lib.sfh_recover_index_batch(comp._h, k, ptrs(srcs), u64([s.size for s in srcs]), 0, u64(want_n), ix.ctypes.data,
                                                 st) == 0, comp.last_error()
        assert ix[entries] == 77
        at = 0
        for i, it in enumerate(items):
            m = nseg_of(want_n[i]) + 1
            if it.n:
                assert st[i] == 0 and ix[at:at + m].tolist() == W.recover_index(it.raw, it.n), i
            else:  # (no source bytes: whether or not one segment of nothing counts as indexable, its two entries are 0)
                assert st[i] in (0, _capi.ITEM_NOT_INDEXABLE) and not ix[at:at + m].any(), i
            at += m


def test_decompress_any_batch_twice(comp, rounds):
    for items in rounds:
        k = len(items)
        want_n = [it.n if it.n else 16 for it in items]
        srcs = sources([it.raw for it in items])
        dsts = filled(want_n)
        out_n = (C.c_uint64 * k)()
        st = (C.c_uint32 * k)(*([99] * k))
        assert comp._lib.sfh_decompress_any_batch(comp._h, k, ptrs(srcs), u64([s.size for s in srcs]), 0, ptrs(dsts), u64(want_n),
                                                  u64(want_n), out_n, st) == 0, comp.last_error()
        assert [v == 0 for v in st] == [it.n > 0 for it in items], list(st)
        assert [out_n[i] for i in range(k) if items[i].n] == [it.n for it in items if it.n]
        check_dsts(dsts, [it.data.tobytes() if it.n else None for it in items])


def test_inflate_stream_batch_twice(comp, rounds):
    """zlib's own streams (no flush points); the zero-length item has no header to read"""
    for items in rounds:
        k = len(items)
        caps = [it.n if it.n else 16 for it in items]
        streams = [it.zlib if it.n else b"" for it in items]
        srcs = sources(streams)
        dsts = filled(caps)
        out_n = (C.c_uint64 * k)()
        st = (C.c_uint32 * k)(*([99] * k))
        assert comp._lib.sfh_inflate_stream_batch(comp._h, k, ptrs(srcs), u64([s.size for s in srcs]), 1, ptrs(dsts), u64(caps), out_n,
                                                  st) == 0, comp.last_error()
        assert [v == 0 for v in st] == [it.n > 0 for it in items], list(st)
        assert [out_n[i] for i in range(k) if items[i].n] == [it.n for it in items if it.n]
        check_dsts(dsts, [zlib.decompress(s) if s else None for s in streams])


def test_host_calls_behind_an_async_call(comp, rounds):
    """sfh_compress_device_async on a caller's stream, then at once sfh_decompress (and again, then sfh_decompress_dz) on host
    buffers of 100000 bytes: both host calls and both asynchronous ones give what they give alone"""
    item = rounds[0][2]
    assert item.n == 100000
    dz = comp.compress(item.data, container="dictzip")
    assert zlib.decompress(dz, 31) == item.data.tobytes()
    big = synth.gen_text(8 << 20, seed=3)
    d_big = torch.from_numpy(big).cuda()
    alone, alone_n = comp.compress_tensor(d_big)
    want = alone[:alone_n].cpu().numpy().tobytes()
    assert zlib.decompress(want, -15) == big.tobytes()
    side = torch.cuda.Stream()
    outs = [torch.zeros(comp.compress_bound(big.size), dtype=torch.uint8, device="cuda") for _ in range(2)]
    sizes = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    comp.compress_tensor_async(d_big, outs[0], sizes[0], stream=side.cuda_stream)
    back, st = comp.decompress(item.raw, item.index, item.n, item.sub, block_bytes=SEG)
    assert st == 0 and back == item.data.tobytes()
    comp.compress_tensor_async(d_big, outs[1], sizes[1], stream=side.cuda_stream)
    back, st = comp.decompress_dictzip(dz)
    assert st == 0 and back == item.data.tobytes()
    side.synchronize()
    for o, n in zip(outs, sizes):
        assert o[:int(n.item())].cpu().numpy().tobytes() == want
