"""The compressor at the ends of the caller's buffers.

Behind an input's last byte: k_lz77 takes a strip's bytes with `load4`, one dword where the word lies inside the strip and
byte by byte, zeros beyond the end, where it does not; the specification never sees a byte behind n.  A kernel that read a
word too far would still give the right stream whenever those bytes happen to be zero.  Here they never are: every item is
a view into a POOL, one device tensor of one content without a zero byte, so behind an item's last byte lies the content's
own continuation -- and, in a batch, at most 15 bytes further on, the next item.  (Today's kernels cap every reader of the
staged bytes at the strip's end on their own, DESIGN.md §3: with `load4` unguarded these tests still pass, as they should;
what they catch is a reader that leans on the zeros, once the bytes are no zeros.)

Which kernels: every effort, through the single call (k_lz77<...>) and through the batch (k_lz77<..., BATCH>, the strip
from a table), at the lengths of test_k1_round_edges -- one, two and four rounds plus the look-ahead, give or take nine
bytes -- with strips of 64 KiB and of 32 KiB (a second strip of 23 to 40 bytes, shorter than the look-ahead or just past it),
through BGZF (every chunk its own strip and member) and dictzip (32 KiB strips).

Where the compressor writes: every destination lies in an ARENA filled with 0xA5, 4 mod 16 (the contract asks for 4-byte
alignment, no more), with a capacity of exactly the call's bound, the destinations of a batch packed back to back, guards
in front of the first and behind the last.  k_emit flushes whole aligned dwords and 16-byte blocks, k_wrap, k_wrap_batch and
k_bgzf_wrap write headers, tables and trailers: none may touch a guard.  (Between a stream's end and its capacity the
bytes are the call's own to write: nothing is asserted about them.)

The specification's side is checked alone first, on the CPU: the layout is what this text says, and every input round-trips
through the oracle's decoder, so a GPU failure here can only be the kernel's."""
import functools
import gzip
import struct
import zlib

import numpy as np
import pytest

import bgzf_files
import oracle_lib as O
from starflate_amd import Compressor, _capi, synth
from test_gpu_parity import EFFORT_PARAMS, _params
from test_k1_round_edges import CHUNK, DELTAS, LENGTHS, LOOK, ROUND

EFFORTS = tuple(EFFORT_PARAMS)
CONTENTS = ("text", "period7", "period300")
STRIPS = (32768, 65536)
SLACK = 65536        # bytes of the same content behind the last byte any item uses
FILL = 0xA5
FIRST_DST = 68       # 4 mod 16
GUARD = 64
BATCH_EXTRA = (1, 31, 3 * CHUNK + 5, CHUNK)
# one member / one 32 KiB strip, give or take a byte, and a second one of 23 to 40 bytes
SHORT_SECOND = tuple(sorted({CHUNK - 1, CHUNK, CHUNK + 1} | {CHUNK + LOOK + d for d in DELTAS}))
DICTZIP = _capi.COMPRESS_CONTAINER["dictzip"]


def _batch_lengths():
    """every entry of LENGTHS in a seeded shuffle, then the extra items"""
    order = np.random.default_rng(47).permutation(len(LENGTHS))
    return [LENGTHS[i] for i in order] + list(BATCH_EXTRA)


@functools.lru_cache(maxsize=None)
def _batch_items():
    """(a, n) of every batch item: consecutive slices of the pool, each starting at the next multiple of 16"""
    items, a = [], 0
    for n in _batch_lengths():
        items.append((a, n))
        a = (a + n + 15) & ~15
    return tuple(items)


def _pool_bytes():
    used = max(max(a + n for a, n in _batch_items()), max(LENGTHS), max(SHORT_SECOND))
    return (used + SLACK + 15) & ~15


@functools.lru_cache(maxsize=None)
def _content(kind):
    """a pool's bytes (never written to): no zero byte anywhere"""
    n = _pool_bytes()
    if kind == "text":
        data = synth.gen_text(n, seed=31)
    elif kind == "period7":  # maximum-length matches run up to an item's last byte: the length cap at n is what counts
        data = np.tile(np.arange(1, 8, dtype=np.uint8), n // 7 + 1)[:n].copy()
    else:
        data = np.tile(np.random.default_rng(300).integers(1, 256, 300, dtype=np.uint8), n // 300 + 1)[:n].copy()
    data.setflags(write=False)
    return data


def _dst_offsets(caps):
    """destinations packed back to back from FIRST_DST on -> (offsets, arena bytes)"""
    offs = [FIRST_DST]
    for c in caps:
        offs.append(offs[-1] + c)
    return offs[:-1], offs[-1] + GUARD


def _oracle_params(effort, bb, **kw):
    p = _params(block_bytes=bb)
    for k, v in dict(EFFORT_PARAMS[effort], **kw).items():
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def _want(kind, a, n, effort, bb, container=0):
    """The specification's stream for content[a : a + n] (computed once, shared by the tests, never written to)."""
    want = O.compress(_content(kind)[a: a + n], _oracle_params(effort, bb, container=container))
    want.setflags(write=False)
    return want


def _diff(got, want):
    """None when equal, else what a failure reports: the sizes, or the first differing offsets"""
    if got.size != want.size:
        return f"size {got.size} != {want.size}"
    if not np.array_equal(got, want):
        return f"first diff at {np.flatnonzero(got != want)[:4]}"
    return None


# ---- the reference alone (CPU) ----

def test_layout():
    items = _batch_items()
    lens = [n for _, n in items]
    assert sorted(lens[: len(LENGTHS)]) == LENGTHS and tuple(lens[len(LENGTHS):]) == BATCH_EXTRA
    assert lens[: len(LENGTHS)] != LENGTHS  # shuffled
    assert set(EFFORTS) == set(_capi.EFFORT) and len(EFFORTS) == 10
    for (a, n), (b, _) in zip(items, items[1:]):
        assert a % 16 == 0 and 0 <= b - (a + n) <= 15
    caps = [Compressor.compress_bound(n) for n in lens]
    offs, total = _dst_offsets(caps)
    assert all(c % 16 == 0 for c in caps) and all(o % 16 == 4 for o in offs) and FIRST_DST % 16 == 4
    assert total == FIRST_DST + sum(caps) + GUARD
    assert 2 * ROUND + LOOK <= SLACK  # what a load a round ahead could reach behind an item lies inside the pool
    last_used = max(max(a + n for a, n in items), max(LENGTHS), max(SHORT_SECOND))
    for kind in CONTENTS:
        data = _content(kind)
        assert data.size % 16 == 0 and data.size - last_used >= SLACK
        assert int(data.min()) > 0  # zeros put behind an item's end always differ from what lies there
        for a, n in items + tuple((0, n) for n in LENGTHS + list(SHORT_SECOND)):
            assert a + n + LOOK + 8 <= data.size
    # a second strip (or member) shorter than the look-ahead, and just past it
    assert min(SHORT_SECOND) == CHUNK - 1 and {n - CHUNK for n in SHORT_SECOND if n > CHUNK + 1} == {LOOK + d for d in DELTAS}
    assert min(LOOK + d for d in DELTAS) == 23 and max(LOOK + d for d in DELTAS) == 40


@pytest.mark.parametrize("effort", EFFORTS)
def test_oracle_streams_round_trip(effort):
    for kind in CONTENTS:
        for bb in STRIPS:
            for n in LENGTHS:
                data = _content(kind)[:n]
                st, w, back = O.decompress(_want(kind, 0, n, effort, bb), n)
                assert st == 0 and w == n and np.array_equal(back, data), (kind, bb, n, effort)


# ---- the kernels (GPU) ----

@pytest.fixture(scope="module")
def pools():
    """kind -> the content in one device tensor (16-byte aligned, never written to)"""
    import torch

    out = {kind: torch.from_numpy(_content(kind).copy()).cuda() for kind in CONTENTS}
    assert all(t.data_ptr() % 16 == 0 for t in out.values())
    return out


class _Arena:
    """One device tensor of 0xA5: destinations of exactly their capacities packed from FIRST_DST on, a guard behind"""

    def __init__(self, caps):
        import torch

        self.offs, total = _dst_offsets(caps)
        self.caps = list(caps)
        self.t = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.end = self.offs[-1] + self.caps[-1]

    def dst(self, i=0):
        return self.t[self.offs[i]: self.offs[i] + self.caps[i]]

    def guards_intact(self):
        return bool((self.t[:FIRST_DST] == FILL).all()) and bool((self.t[self.end:] == FILL).all())


@pytest.fixture(scope="module")
def arenas():
    """capacity -> arena with that one destination (the single calls' capacities are few: made once, filled again per call)"""
    made = {}

    def get(cap):
        if cap not in made:
            made[cap] = _Arena([cap])
        made[cap].t.fill_(FILL)
        return made[cap]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("effort", EFFORTS)
def test_single_call_live_tail(compressor, pools, arenas, effort):
    bad = []
    for kind in CONTENTS:
        for bb in (65536, 32768) if kind == "text" else (65536,):
            for n in LENGTHS:
                cap = compressor.compress_bound(n)
                arena = arenas(cap)
                out, size = compressor.compress_tensor(pools[kind][:n], out=arena.dst(), block_bytes=bb, effort=effort)
                assert out.numel() == cap and out.data_ptr() % 16 == 4
                assert arena.guards_intact(), f"{kind}/{bb}/n{n}/{effort}: a guard was written"
                d = _diff(out[:size].cpu().numpy(), _want(kind, 0, n, effort, bb))
                if d:
                    bad.append(f"{kind}/{bb}/n{n}: {d}")
    assert not bad, f"{effort}: {len(bad)} streams differ from the oracle's: " + "; ".join(bad)


def _batch(compressor, pool, **opt):
    """one compress_batch_tensors call over the pool's items into one packed arena -> (arena, streams)"""
    import torch

    items = _batch_items()
    arena = _Arena([compressor.compress_bound(n) for _, n in items])
    srcs = [pool[a: a + n] for a, n in items]
    outs = [arena.dst(i) for i in range(len(items))]
    assert all(s.data_ptr() % 16 == 0 for s in srcs) and all(o.data_ptr() % 16 == 4 for o in outs)
    _, sizes = compressor.compress_batch_tensors(srcs, outs=outs, **opt)
    torch.cuda.synchronize()
    sizes = sizes.cpu().tolist()
    whole = arena.t.cpu().numpy()
    assert all(0 < s <= c for s, c in zip(sizes, arena.caps)), sizes
    return arena, [whole[o: o + s] for o, s in zip(arena.offs, sizes)]


@pytest.mark.gpu
@pytest.mark.parametrize("bb", STRIPS)
@pytest.mark.parametrize("effort", EFFORTS)
def test_batch_live_tails(compressor, pools, effort, bb):
    bad = []
    for kind in CONTENTS:
        arena, streams = _batch(compressor, pools[kind], block_bytes=bb, effort=effort)
        assert arena.guards_intact(), f"{kind}/{bb}/{effort}: a guard was written"
        for i, ((a, n), got) in enumerate(zip(_batch_items(), streams)):
            d = _diff(got, _want(kind, a, n, effort, bb))
            if d:
                bad.append(f"{kind}/item{i}/n{n}: {d}")
    assert not bad, f"{effort}/{bb}: {len(bad)} streams differ from the oracle's: " + "; ".join(bad)
    if effort == "default" and bb == 65536:  # once, wrapped: k_wrap_batch writes a header in front and a trailer behind
        for kind in CONTENTS:
            arena, streams = _batch(compressor, pools[kind], block_bytes=bb, effort=effort, container="gzip")
            assert arena.guards_intact(), f"{kind}/gzip: a guard was written"
            for i, ((a, n), got) in enumerate(zip(_batch_items(), streams)):
                data = _content(kind)[a: a + n].tobytes()
                s = got.tobytes()
                assert s[:4] == b"\x1f\x8b\x08\x00" and len(s) >= 18, (kind, i, n)
                assert struct.unpack("<II", s[-8:]) == (zlib.crc32(data), n), (kind, i, n)
                d = _diff(got[10:-8], _want(kind, a, n, effort, bb))
                assert d is None, f"{kind}/gzip/item{i}/n{n}: {d}"
                assert zlib.decompress(s, 31) == data, (kind, i, n)


def _bgzf_want(kind, n, effort):
    """the file, from the oracle alone: per 32 KiB slice the BGZF header with its BSIZE, the slice's stream, CRC-32, ISIZE"""
    data = _content(kind)[:n]
    out = b""
    for a in range(0, n, CHUNK):
        m = min(CHUNK, n - a)
        body = O.compress(data[a: a + m], _oracle_params(effort, 32768, final_stream=1)).tobytes()
        out += bgzf_files.EOF[:16] + struct.pack("<H", 18 + len(body) + 8 - 1) + body
        out += struct.pack("<II", zlib.crc32(data[a: a + m].tobytes()), m)
    return out + bgzf_files.EOF


@pytest.mark.gpu
@pytest.mark.parametrize("effort", ["default", "max", "best"])
def test_bgzf_live_tail(compressor, pools, arenas, effort):
    bad = []
    for kind in ("text", "period7"):
        for n in SHORT_SECOND:
            cap = compressor.bgzf_bound(n)
            arena = arenas(cap)
            assert arena.dst().data_ptr() % 16 == 4
            out, size = compressor.compress_bgzf_tensor(pools[kind][:n], out=arena.dst(), effort=effort)
            assert arena.guards_intact(), f"{kind}/n{n}/{effort}: a guard was written"
            got = out[:size].cpu().numpy()
            d = _diff(got, np.frombuffer(_bgzf_want(kind, n, effort), np.uint8))
            if d:
                bad.append(f"{kind}/n{n}: {d}")
            else:
                assert gzip.decompress(got.tobytes()) == _content(kind)[:n].tobytes(), (kind, n)
    assert not bad, f"{effort}: {len(bad)} files differ from the oracle's: " + "; ".join(bad)


@pytest.mark.gpu
def test_dictzip_live_tail(compressor, pools, arenas):
    lib = _capi.lib()
    bad = []
    for n in SHORT_SECOND:
        cap = lib.sfh_compress_bound_container(n, 32768, DICTZIP)
        arena = arenas(cap)
        assert arena.dst().data_ptr() % 16 == 4
        out, size = compressor.compress_tensor(pools["text"][:n], out=arena.dst(), container="dictzip", block_bytes=32768)
        assert arena.guards_intact(), f"n{n}: a guard was written"
        got = out[:size].cpu().numpy()
        hdr = lib.sfh_dz_header_bytes(n)
        d = _diff(got[hdr:], _want("text", 0, n, "default", 32768, container=_capi.CONTAINER["gzip"])[10:])
        if d:
            bad.append(f"n{n}: {d}")
        else:
            assert zlib.decompress(got.tobytes(), 31) == _content("text")[:n].tobytes(), n
    assert not bad, f"{len(bad)} files differ from the oracle's behind the header: " + "; ".join(bad)
