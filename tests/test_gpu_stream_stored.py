"""Stored blocks as chunk starts of the stream decoder (stored_header_candidate in k_stream_find, copy_stored in the write pass;
DESIGN.md 3a "Stored block starts").  Every result is compared with the serial decoder (container.hpp through stream_host.serial):
status, size and bytes.  A stored candidate, true or false, may change the time and the chunk counts only.  `small` has 512-byte
nominal chunks, so that small streams are cut into many chunks."""
import zlib

import numpy as np
import pytest
import torch

import deflate_writer as W
import stream_host as H
from starflate_amd import Compressor, synth
from stream_cases import write_fixed
from stream_lookalikes import look, stored_look_alikes

pytestmark = pytest.mark.gpu

OK, DST_TOO_SMALL = 0, 4
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
CONTAINERS = ("raw", "zlib", "gzip")


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(monkeypatch_module):
    monkeypatch_module.setenv("SFH_STREAM_CHUNK", "512")
    c = Compressor(0)
    monkeypatch_module.delenv("SFH_STREAM_CHUNK")
    yield c
    c.close()


def _zlib(data, container="raw", level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[container])
    return c.compress(data) + c.flush()


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _serial(stream, container, cap):
    """-> (status, the serial decoder's bytes when it succeeded)"""
    st, _, dst = H.serial(stream, container, cap)
    return st, dst


def _check(c, stream, container, cap):
    """one stream: the GPU's status, size and bytes are the serial decoder's -> status"""
    want_st, want = _serial(stream, container, cap)
    out, st = c.decompress_stream(stream, cap, container)
    assert st == want_st, (st, want_st, container, cap)
    if st == OK:
        if container == "zlib":  # (container.hpp wants a zlib dst of exactly the output size: cap is that)
            assert len(out) == cap
        assert out == want[: len(out)].tobytes()
        assert out == zlib.decompressobj(WBITS[container]).decompress(stream)
    return st


def _check_batch(c, streams, caps, container="raw"):
    """one batched call: every item's status, size and bytes are the serial decoder's -> (outputs, statuses)"""
    outs, sts = c.decompress_stream_batch(streams, caps, container)
    for k, s in enumerate(streams):
        want_st, want = _serial(s, container, caps[k])
        assert sts[k] == want_st, (k, sts[k], want_st)
        if want_st == OK:
            assert len(outs[k]) == caps[k] and outs[k] == want[: caps[k]].tobytes(), k
    return outs, sts


# ---- 1. a level-0 stream is cut at its blocks ----

@pytest.mark.parametrize("container", CONTAINERS)
def test_level0_cut_at_blocks(comp, container):
    data = synth.gen_text(1 << 20, seed=3).tobytes()
    stream = _zlib(data, container, 0)
    raw = _zlib(data, "raw", 0)
    assert H.scan(raw) == []  # no dynamic-header candidate anywhere in it
    _, blocks = W.inflate(np.frombuffer(raw, np.uint8))
    lens = [b2["out"] - b1["out"] for b1, b2 in zip(blocks, blocks[1:])]
    k, L = len(blocks) - 1, max(lens)
    assert all(b["type"] == 0 for b in blocks) and k >= 16 and L == 65535
    assert _check(comp, stream, container, len(data)) == OK
    s = comp.last_stream_stats()
    print(container, "non-final stored blocks", k, "largest LEN", L, s)
    assert s["confirmed"] >= k // 2, s
    assert s["longest_chunk"] <= 2 * L, s
    assert s["repair_rounds"] <= 1, s
    assert comp.decompress_stream(stream, None, container) == (data, OK)  # the size query gives the same size


@pytest.mark.parametrize("mem,n", [(1, 300000), (6, 1 << 20), (7, 1 << 20), (8, 1 << 20)])
def test_short_stored_blocks_cut(comp, mem, n):
    """level 6 of noise at memLevel 1, 6, 7 and 8: stored blocks of 127 bytes, 4, 8 and 16 KiB.  Every nominal chunk (16 KiB)
    holds at most one chunk start.  Blocks longer than a nominal chunk have their headers in different chunks, so all of them
    but the last are starts; with shorter blocks every nominal chunk holds a header, but for the last two, which may hold
    only the run's last block and the final one"""
    data = _noise(n, 21 + mem)
    c = zlib.compressobj(6, zlib.DEFLATED, 15, mem)
    stream = c.compress(data) + c.flush()
    assert H.scan(stream[2:-4]) == []
    assert _check(comp, stream, "zlib", n) == OK
    s = comp.last_stream_stats()
    print(mem, s)
    _, blocks = W.inflate(np.frombuffer(stream[2:-4], np.uint8))
    assert all(b["type"] == 0 for b in blocks)
    assert s["confirmed"] >= min(s["chunks"] - 2, len(blocks) - 2), (s, len(blocks))
    assert s["longest_chunk"] <= 2 * 16384 + 65535 // 2, s
    assert s["repair_rounds"] <= 1, s


# ---- 2. a stored header at every bit offset, behind a block ending in zeros and behind one ending in a one ----

LENS = (65535, 0, 1, 5, 507, 508, 509, 512, 1024)  # (the long one first: the others then lie behind chunk 0 on a default context too)
ONES_LL = [1 if s == 97 else 2 if s in (98, 256) else 0 for s in range(286)]  # codes 0, 10 and, for end-of-block, 11


def _lead(bw, kind, n, final=False):
    """a Huffman block in front of a stored one: fixed (its end-of-block is seven zero bits) with n 9-bit literals, or dynamic
    with n 1-bit literals and an end-of-block code of two one bits -> its output"""
    if kind == "fixed":
        toks = [120, 121] + [200] * n
        write_fixed(bw, toks, final)
    else:
        toks = [98] + [97] * n
        W.write_dynamic(bw, toks, ONES_LL, [1, 1] + [0] * 28, final=final)
    return bytes(toks)


def _lead_to(bw, kind, offset):
    """a lead block, written at a byte boundary, that ends at bit `offset` of a byte -> its output"""
    for n in range(1, 9):
        probe = W.BitWriter()
        out = _lead(probe, kind, n)
        if probe.n % 8 == offset:
            assert bw.n % 8 == 0
            _lead(bw, kind, n)
            return out
    raise AssertionError((kind, offset))


def _every_bit(kind, offset, seed):
    bw, out = W.BitWriter(), bytearray()
    rng = np.random.default_rng(seed)
    for ln in LENS:
        out += _lead_to(bw, kind, offset)
        assert bw.n % 8 == offset
        piece = rng.integers(32, 256, ln, dtype=np.uint8).tobytes()  # (no byte below 32: no look-alike here)
        W.write_stored(bw, piece)  # a candidate: a stored block follows it
        W.write_stored(bw, b"+-+")  # none: the lead block follows
        out += piece + b"+-+"
    out += _lead(bw, kind, 3, final=True)
    return bw.bytes().tobytes(), bytes(out)


def _empties():
    bw, out = W.BitWriter(), bytearray()
    out += _lead(bw, "dynamic", 2)
    for _ in range(10):
        W.write_stored_empty(bw)
    out += _lead(bw, "fixed", 2)
    for _ in range(10):
        W.write_stored_empty(bw)
    W.write_stored(bw, b"the end", final=True)
    return bw.bytes().tobytes(), bytes(out) + b"the end"


def _nonzero_padding(seed):
    """stored blocks whose padding bits are not zero (the format allows it): never candidates, decoded all the same"""
    bw, out = W.BitWriter(), bytearray()
    rng = np.random.default_rng(seed)
    for pad in (0b11111, 0b00001, 0b10000, 0b01010):
        piece = rng.integers(32, 256, 700, dtype=np.uint8).tobytes()
        bw.put(0, 1)
        bw.put(0, 2)
        bw.put(pad, 5)
        bw.put(len(piece), 16)
        bw.put(len(piece) ^ 0xFFFF, 16)
        bw.put(int.from_bytes(piece, "little"), 8 * len(piece))
        out += piece
    out += _lead(bw, "fixed", 1, final=True)
    return bw.bytes().tobytes(), bytes(out)


def _header_streams():
    made = [_every_bit(kind, offset, 8 * (kind == "fixed") + offset) for kind in ("fixed", "dynamic") for offset in range(8)]
    return made + [_empties(), _nonzero_padding(5)]


def test_header_at_every_bit(comp, small):
    made = _header_streams()
    streams, datas = [s for s, _ in made], [d for _, d in made]
    for s, d in made:
        st, n, want = H.serial(s, "raw", len(d))
        assert st == OK and n == len(d) and want.tobytes() == d  # (the writer and the serial decoder agree)
    for c in (comp, small):
        sts = _check_batch(c, streams, [len(d) for d in datas])[1]
        s = c.last_stream_stats()
        assert all(st == OK for st in sts), sts
        print(s)
        assert s["repair_rounds"] <= 2, s
        for stream, d in made[::5]:  # (and singly, with a size query)
            assert c.decompress_stream(stream, None, "raw") == (d, OK)
            assert c.last_stream_stats()["repair_rounds"] <= 2


# ---- 3. look-alikes: `v LEN NLEN` with v < 32 inside payloads ----

def _rev8(b):
    return int(f"{b:08b}"[::-1], 2)


def _fixed_look_alikes(nblocks=6):
    """fixed blocks of literals only: five 9-bit literals behind the 3 header bits put every 8-bit literal code on a stream byte
    of its own, the code's bits reversed.  The stream then holds `0x09 LEN NLEN` wherever the literals say so (bytes whose
    reversed value is a literal's code: both bytes of LEN have their two low bits 01 or 10).  0x09 in front of LEN reads as a
    stored header (a final one) where another look-alike's payload ends, so the finder takes those"""
    def lit(stream_byte):
        code = _rev8(stream_byte)
        assert 0x30 <= code <= 0xBF, stream_byte
        return code - 0x30

    bw, out = W.BitWriter(), bytearray()
    for b in range(nblocks):
        assert bw.n % 8 == 0
        body = bytearray([(0x55, 0x5A, 0x65)[j % 3] for j in range(1400)])  # (stream bytes)
        far = 0x0009 + 0x100 * (0x0A, 0x0D, 0x0E, 0x11, 0x12, 0x15)[b % 6]  # past the next true header
        # one that ends on the next (292 = 35 + 0x0101), which runs past the block; three in a row, each ending on the next
        # one's first byte (862 = 605 + 0x0101, 1381 = 867 + 0x0202)
        for at, ln in ((30, 0x0101), (292, far), (600, 0x0101), (862, 0x0202), (1381, 0x0205)):
            body[at: at + 5] = look(0x09, ln)
        toks = [200] * 5 + [lit(x) for x in body]
        write_fixed(bw, toks)
        out += bytes(toks)
        W.write_stored(bw, b"")  # (realigns; its own header is a true candidate)
    W.write_stored(bw, b"tail", final=True)
    return bw.bytes().tobytes(), bytes(out) + b"tail"


def _past_the_body():
    """look-alikes whose LEN ends exactly on the body's last byte (a candidate) and one byte past it (none)"""
    made = []
    for extra in (0, 1):
        bw = W.BitWriter()
        p = bytearray(_noise(3000, 40 + extra).replace(b"\x00", b"\x01"))
        W.write_stored(bw, bytes(p))
        W.write_stored(bw, b"xyz", final=True)
        n = len(bw.bytes())
        at = 5 + 600  # the look-alike's v byte, in stream bytes
        ln = n - (at + 5) + extra
        p[600:605] = look(0, ln)
        bw = W.BitWriter()
        W.write_stored(bw, bytes(p))
        W.write_stored(bw, b"xyz", final=True)
        assert len(bw.bytes()) == n
        made.append((bw.bytes().tobytes(), bytes(p) + b"xyz"))
    return made


def test_look_alikes(small):
    made = [stored_look_alikes(1), stored_look_alikes(2, nblocks=3, size=1300), _fixed_look_alikes()] + _past_the_body()
    for s, d in made:
        st, n, want = H.serial(s, "raw", len(d))
        assert st == OK and n == len(d) and want.tobytes() == d
    for s, d in made:
        assert _check(small, s, "raw", len(d)) == OK
        st = small.last_stream_stats()
        print(st)
        assert st["repair_rounds"] <= 2, st
    sts = _check_batch(small, [s for s, _ in made], [len(d) for _, d in made])[1]
    assert all(x == OK for x in sts)


# ---- 4. damage ----

def _damaged(container):
    """[(stream, capacity)] for level 0 and level 6 of 200 KB of noise in `container`"""
    data = _noise(200000, 9)
    off = {"raw": 0, "zlib": 2, "gzip": 10}[container]
    out = []
    for level in (0, 6):
        good = _zlib(data, container, level)
        _, blocks = W.inflate(np.frombuffer(_zlib(data, "raw", level), np.uint8))
        assert all(b["type"] == 0 for b in blocks) and len(blocks) >= 4
        B = off + (blocks[len(blocks) // 2]["start"] + 10) // 8  # a true LEN in the middle of the stream
        for at, bit in ((B, 0), (B + 1, 6), (B + 2, 3), (B + 3, 7)):  # one bit of LEN, of NLEN
            bad = bytearray(good)
            bad[at] ^= 1 << bit
            out.append((bytes(bad), len(data)))
        out += [(good[: B + 4 + 100], len(data)), (good[: B + 1], len(data)), (good[: B + 3], len(data)), (good[:B], len(data))]
        out += [(good, len(data) - 1), (good, len(data))]
        if container != "raw":
            for back in (1, 4) + ((5, 8) if container == "gzip" else ()):  # Adler-32; CRC-32 and ISIZE
                bad = bytearray(good)
                bad[-back] ^= 0x10
                out.append((bytes(bad), len(data)))
    return out


@pytest.mark.parametrize("container", CONTAINERS)
def test_damage(comp, small, container):
    cases = _damaged(container)
    seen = set()
    for c in (comp, small):
        for stream, cap in cases:
            seen.add(_check(c, stream, container, cap))
        seen |= set(_check_batch(c, [s for s, _ in cases], [cap for _, cap in cases], container)[1])
    assert OK in seen and DST_TOO_SMALL in seen and len(seen) >= 4, seen


# ---- 5. the wide copy: every head and tail at every source byte phase ----

GRID_K = range(16)
GRID_J = range(4)
GRID_L = tuple(range(1, 34)) + (4095, 4096, 4097)


def _copy_stream(k, j, L, rng):
    """k literals move the payload's place in the plane (the copy's head), j empty stored blocks of 5 bytes in front move its
    place in the stream against that (the source's dword phase)"""
    bw = W.BitWriter()
    for _ in range(j):
        W.write_stored_empty(bw)
    lits = [int(x) for x in rng.integers(0, 144, k)]
    write_fixed(bw, lits)
    piece = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
    W.write_stored(bw, piece)
    toks = [W.match(258, L if L >= 3 else L + k)]  # (reads the plane entries the copy wrote)
    write_fixed(bw, toks)
    W.write_stored(bw, b"end", final=True)
    return bw.bytes().tobytes(), W.expand(lits + [int(x) for x in piece] + toks) + b"end"


@pytest.fixture(scope="module")
def grid():
    rng = np.random.default_rng(77)
    made = [_copy_stream(k, j, L, rng) for k in GRID_K for j in GRID_J for L in GRID_L]
    phases = {(k, (6 + 5 * j + k) % 4) for k in GRID_K for j in GRID_J}  # (head, source byte phase of the payload)
    assert len(phases) == 64
    return made


def test_wide_copy(comp, small, grid):
    """the whole grid on both contexts, one batched call each"""
    streams, datas = [s for s, _ in grid], [d for _, d in grid]
    for c in (comp, small):
        outs, sts = _check_batch(c, streams, [len(d) for d in datas])
        assert all(st == OK for st in sts), [k for k, st in enumerate(sts) if st != OK][:5]
        assert outs == datas  # (and the writer's own bytes)


def test_wide_copy_source_offsets(comp, grid):
    """the stream at device addresses 0, 4, 8 and 12 past a 16-byte boundary (d_src is 4-byte aligned), and ending on the last
    byte of its tensor"""
    for stream, d in (grid[0], grid[len(GRID_L) * 21 + 20], grid[-1], grid[-2]):
        for off in (0, 4, 8, 12):
            t = torch.zeros(off + len(stream), dtype=torch.uint8)
            t[off:] = torch.from_numpy(np.frombuffer(stream, np.uint8).copy())
            t = t.cuda()
            assert t.data_ptr() % 16 == 0
            out, st = comp.decompress_stream_tensor(t[off:], len(d), "raw")
            assert st == OK and out.cpu().numpy().tobytes() == d, (off, len(stream))


# ---- 6. a batch equals its singles ----

def test_batch_equals_singles(comp, small):
    text, noise = synth.gen_text(300000, seed=4).tobytes(), _noise(300000, 6)
    level0 = _zlib(text, "zlib", 0)
    bad = bytearray(level0)
    bad[len(bad) // 2] ^= 0x40
    hit = bytearray(level0)
    hit[2 + 65540 + 3] ^= 0x01  # the second block's NLEN
    streams = [level0, _zlib(noise, "zlib", 6), _zlib(text, "zlib", 6), zlib.compress(b""), _zlib(text[:59], "zlib", 0),
               bytes(bad), bytes(hit)]
    assert len(streams[4]) == 70
    caps = [len(text), len(noise), len(text), 0, 59, len(text), len(text)]
    for c in (comp, small):
        outs, sts = c.decompress_stream_batch(streams, caps, "zlib")
        for k, s in enumerate(streams):
            out1, st1 = c.decompress_stream(s, caps[k], "zlib")
            want = H.serial(s, "zlib", caps[k])[0]
            assert sts[k] == st1 == want, (k, sts[k], st1, want)
            assert outs[k] == out1 and len(out1) == (caps[k] if st1 == OK else 0), k
        assert sts[:5] == [OK] * 5 and sts[5] != OK and sts[6] != OK, sts
        assert outs[0] == text and outs[1] == noise and outs[2] == text
        sizes, sts2 = c.decompress_stream_batch(streams, None, "zlib")
        assert sts2 == sts and [len(x) for x in sizes] == [len(x) for x in outs]
