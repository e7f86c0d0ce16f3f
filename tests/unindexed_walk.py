"""The walk rule of DESIGN.md 3a in plain Python: the segment index of a block-flushed DEFLATE stream, from the stream alone.

TEST INFRASTRUCTURE: the specification the GPU's recovered index (sfh_recover_index*) is compared with.
"""
import functools
import struct
import zlib

import numpy as np

SEG = 32768
STORED_SEG = SEG + 5  # header byte, LEN, NLEN, 32 KiB
MARK = b"\x00\x00\xff\xff"
EMPTY_STORED = b"\x00\x00\x00\xff\xff"


class NotIndexable(Exception):
    """The stream is not block-flushed every 32 KiB of output (SFH_E_NOT_INDEXABLE)."""


def body_range(stream, container="raw"):
    """[b0, e): the stream without its wrapper (zlib: 2-byte header, 4-byte trailer; gzip: FEXTRA / FNAME / FCOMMENT / FHCRC)."""
    n = len(stream)
    if container == "raw":
        return 0, n
    if container == "zlib":
        return 2, n - 4
    flg, at = stream[3], 10
    if flg & 0x04:
        at += 2 + (stream[at] | stream[at + 1] << 8)
    for bit in (0x08, 0x10):
        if flg & bit:
            at = stream.index(b"\x00", at) + 1
    if flg & 0x02:
        at += 2
    return at, n - 8


def is_stored_header(stream, h, e):
    return h + 5 <= e and stream[h] in (0, 1) and stream[h + 1:h + 5] == b"\x00\x80\xff\x7f"


def landing(stream, s, e):
    t = s + STORED_SEG
    while t + 5 <= e and stream[t:t + 5] == EMPTY_STORED:
        t += 5
    return t


def recover_index(stream, dst_n, container="raw"):
    """-> list of nseg + 1 offsets (wrapper header included).  Raises NotIndexable."""
    stream = bytes(stream)
    b0, e = body_range(stream, container)
    nseg = max(1, -(-dst_n // SEG))
    starts = [b0]
    s = b0
    while len(starts) < nseg:
        if is_stored_header(stream, s, e):
            s = landing(stream, s, e)
        else:
            p = stream.find(MARK, max(s - 3, b0))  # the first marker ending after s, inside the body
            if p == -1 or p + 4 >= e:
                raise NotIndexable(f"{len(starts)} of {nseg} segments")
            s = p + 4
        if s >= e:
            raise NotIndexable(f"{len(starts)} of {nseg} segments")
        starts.append(s)
    return starts + [e]


def zlib_flushed(data, level=6, flush=zlib.Z_FULL_FLUSH, wbits=-15, finish_block=True, every=SEG):
    """zlib's stream of `data` with `flush` after every `every` input bytes (finish_block: Z_FINISH behind the last flush,
    which writes an empty final block; else the last piece is compressed with Z_FINISH directly)."""
    c = zlib.compressobj(level, zlib.DEFLATED, wbits)
    out = []
    pieces = [data[i:i + every] for i in range(0, len(data), every)] or [b""]
    for k, piece in enumerate(pieces):
        out.append(c.compress(piece))
        if k + 1 < len(pieces) or finish_block:
            out.append(c.flush(flush))
    out.append(c.flush(zlib.Z_FINISH))
    return b"".join(out)


def scan_nodes(stream, b0, e):
    """The nodes of the device scan, counted by its rule: the body's first byte b0, every p in [b0 + 4, e) behind
    a flush marker, every p with p + 5 <= e where a stored block of 32 KiB starts."""
    stream = bytes(stream)
    nodes = {b0}
    p = stream.find(MARK, b0)
    while p != -1 and p + 4 < e:
        nodes.add(p + 4)
        p = stream.find(MARK, p + 1)
    for first in (b"\x00", b"\x01"):
        pat = first + b"\x00\x80\xff\x7f"
        p = stream.find(pat, b0)
        while p != -1 and p + 5 <= e:
            nodes.add(p)
            p = stream.find(pat, p + 1)
    return len(nodes)


# ---- streams for the flush-point walk beyond one workgroup, one scan tile and at the scan's seams
# (tests/test_gpu_walk_scale.py; tests/test_walk_scale_inputs.py holds every count and position stated here, without a GPU) ----
CHAIN_NODES = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097)
WRAPPED_NODES = (256, 1024, 1025)  # ... of which these also as zlib and gzip streams
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
FINAL = b"\x03\x00"  # an empty final block of fixed codes
ROW_SEGMENTS, ROW_FULL_EVERY = 1300, 7


@functools.lru_cache(maxsize=None)
def chain_stream(nodes, container="raw"):
    """-> (data, stream): nodes - 1 segments of zeros, a full flush behind each: b0 and nodes - 1 markers"""
    data = bytes((nodes - 1) * SEG)
    return data, zlib_flushed(data, 6, zlib.Z_FULL_FLUSH, WBITS[container], True)


@functools.lru_cache(maxsize=None)
def rows_stream():
    """-> (data, stream): ROW_SEGMENTS segments of zeros, a full flush behind segment k where k % ROW_FULL_EVERY == 0, a sync
    flush behind the others"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    out = []
    for k in range(ROW_SEGMENTS):
        out.append(c.compress(bytes(SEG)))
        out.append(c.flush(zlib.Z_FULL_FLUSH if k % ROW_FULL_EVERY == 0 else zlib.Z_SYNC_FLUSH))
    out.append(c.flush(zlib.Z_FINISH))
    return bytes(ROW_SEGMENTS * SEG), b"".join(out)


def independent_segments(stream, index):
    """how many segments zlib decodes from their own bytes alone: all but those it refuses with 'distance too far back'"""
    rows = 0
    for k in range(len(index) - 1):
        try:
            zlib.decompressobj(-15).decompress(stream[index[k]: index[k + 1]])
            rows += 1
        except zlib.error as err:
            if "distance too far back" not in str(err):
                raise
    return rows


def coded_segment(piece, level=6):
    """one segment of a raw stream: its blocks, none final, and the marker of a full flush"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(piece) + c.flush(zlib.Z_FULL_FLUSH)


def stored_segment(piece):
    assert len(piece) == SEG
    return b"\x00\x00\x80\xff\x7f" + piece


def assemble(parts):
    """parts: ("coded" | "stored", 32 KiB of data) in stream order -> (data, stream, the segments' first bytes and the body's
    end); the stream closes with an empty final block"""
    out, starts, at = [], [], 0
    for kind, piece in parts:
        seg = stored_segment(piece) if kind == "stored" else coded_segment(piece)
        starts.append(at)
        at += len(seg)
        out.append(seg)
    out.append(FINAL)
    return b"".join(p for _, p in parts), b"".join(out), starts + [at + len(FINAL)]


def _texts(count, seed):
    from starflate_amd import synth

    return [synth.gen_text(SEG, seed=seed + k).tobytes() for k in range(count)]


@functools.lru_cache(maxsize=None)
def decoy_stream(kind, stored=10):
    """-> (data, stream, index): coded segments of text and, between them, `stored` stored segments whose 32 KiB are
    kind "markers": 00 00 FF FF repeated -- 8192 marker nodes each, the last of them the next segment's first byte;
    kind "headers": 00 00 80 FF 7F every 5 bytes -- 6553 stored-header nodes each, nobody's successor"""
    fill = (MARK * (SEG // 4)) if kind == "markers" else (b"\x00\x00\x80\xff\x7f" * (SEG // 5 + 1))[:SEG]
    texts = _texts(4, 70)
    parts = []
    for k in range(stored):
        parts += [("coded", texts[k % 4]), ("stored", fill)]
    parts.append(("coded", texts[0]))
    return assemble(parts)


@functools.lru_cache(maxsize=None)
def alternating_stream(pairs=300):
    """-> (data, stream, index): a stored segment of random bytes, then a coded one, `pairs` times: every stored header's
    landing is a coded segment's first byte, which is no node -- an edge over two segments, pairs + 1 nodes in all"""
    rng = np.random.default_rng(80)
    texts = _texts(8, 90)
    noise = [rng.integers(0, 256, SEG, dtype=np.uint8).tobytes() for _ in range(8)]
    parts = []
    for k in range(pairs):
        parts += [("stored", noise[k % 8]), ("coded", texts[(k // 8 + k) % 8])]
    return assemble(parts)


def gzip_wrap(body, data, fname=None, extra=None):
    flg = (4 if extra is not None else 0) | (8 if fname is not None else 0)
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff"
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if fname is not None:
        head += fname + b"\0"
    return head + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


SEAM_MODULI = (8192, 256)  # k_any_scan: a wave's piece of an item's stream, and one round of it (64 lanes x 4 positions)
SEAM_REACH = 4


@functools.lru_cache(maxsize=None)
def _seam_body():
    """coded, stored, stored, coded, coded: segment 2's first byte is a stored header no marker ends at, segment 4's the end
    of a marker where no stored block starts"""
    texts = _texts(3, 100)
    rnd = np.random.default_rng(101).integers(0, 256, 2 * SEG, dtype=np.uint8).tobytes()
    return assemble([("coded", texts[0]), ("stored", rnd[:SEG]), ("stored", rnd[SEG:]), ("coded", texts[1]), ("coded", texts[2])])


def seam_stream(name_bytes):
    """-> (data, gzip stream, index): _seam_body() behind a header with a file name of `name_bytes` letters"""
    data, body, starts = _seam_body()
    b0 = 10 + name_bytes + 1
    return data, gzip_wrap(body, data, fname=b"n" * name_bytes), [b0 + s for s in starts]


def seam_cases():
    """(what, modulus, d, name_bytes): the name's length that puts the stored header ("H", segment 2) or the marker's end ("M",
    segment 4) d bytes from a multiple of the modulus -- for 256 one that is no multiple of 8192"""
    _, _, starts = _seam_body()
    out = []
    for what, seg in (("H", 2), ("M", 4)):
        for mod in SEAM_MODULI:
            for d in range(-SEAM_REACH, SEAM_REACH + 1):
                name = (d - (11 + starts[seg])) % mod
                if mod == 256 and (11 + name + starts[seg] - d) % 8192 == 0:
                    name += 256
                out.append((what, mod, d, name))
    return out


def marker_at_b0_stream():
    """-> (data, gzip stream): an extra field whose last four bytes are a marker: it ends at b0, inside [b0, b0 + 4)"""
    data = _texts(1, 110)[0] * 3
    return data, gzip_wrap(zlib_flushed(data, 6, zlib.Z_SYNC_FLUSH, -15, True), data, extra=b"XY\x04\x00" + MARK)


def marker_across_b0_stream():
    """-> (data, gzip stream): the name's closing zero and a stored block of 65535 bytes (00 FF FF 00 00) make a marker that
    ends at b0 + 3: by the scan's rule no node.  Behind the block 65537 bytes flushed every 32 KiB: b0 and three markers for
    the four segments of 131072 bytes"""
    data = (_texts(1, 120)[0] * 5)[: 4 * SEG]
    body = b"\x00\xff\xff\x00\x00" + data[:65535] + zlib_flushed(data[65535:], 6, zlib.Z_FULL_FLUSH, -15, True)
    return data, gzip_wrap(body, data, fname=b"a")


MANY_ITEMS, MANY_LONG, MANY_BAD = 700, (100, 450), tuple(range(35, 700, 70))


@functools.lru_cache(maxsize=None)
def many_items():
    """-> MANY_ITEMS x (data size, raw stream): items of one segment, of two to five, two of 600 (at MANY_LONG), and at MANY_BAD
    items of several segments that have no marker to spare (no flush behind the last one) and one of them cut"""
    texts = _texts(5, 130)
    pool = {n: zlib_flushed(b"".join(texts[:n]), 1, zlib.Z_FULL_FLUSH, -15, True) for n in range(1, 6)}
    bare = {n: zlib_flushed(b"".join(texts[:n]), 1, zlib.Z_FULL_FLUSH, -15, False) for n in range(2, 6)}
    short = zlib_flushed(texts[0][:1000], 1, zlib.Z_FULL_FLUSH, -15, True)
    out = []
    for i in range(MANY_ITEMS):
        if i in MANY_LONG:
            out.append((600 * SEG, zlib_flushed(bytes(600 * SEG), 6, zlib.Z_FULL_FLUSH, -15, True)))
        elif i in MANY_BAD:
            n = 2 + i % 4
            s = bare[n]
            at = s.find(MARK)
            out.append((n * SEG, s[: at + 3] + b"\xef" + s[at + 4:]))
        elif i % 3 == 0:
            out.append((1000, short) if i % 2 else (SEG, pool[1]))
        else:
            n = 2 + i % 4
            out.append((n * SEG, pool[n]))
    return out
