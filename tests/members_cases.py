"""Multi-member gzip files for the tests of Container::GzipMembers / SFH_GZIP_MEMBERS (tests/test_stream_members_host.py on
the CPU, tests/test_gpu_stream_members.py on the GPU): seeded, nothing on disk.  good(): files gzip.decompress reads;
bad(): one file per malformation class with the status the specification gives it.  TEST INFRASTRUCTURE ONLY."""
import zlib

import numpy as np

import bgzf_files as B
import deflate_writer as W
import stream_cases as SC

HEAD = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"
BIG = 1 << 20


def text(n, seed=0):
    return B.text(n, seed)


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def member(data, body=None, flg=0, extra=b"", name=b"", comment=b"", crc=None, isize=None, **kw):
    """one member around `body` (default: zlib's raw stream of data); the optional fields follow flg, FHCRC holds two zero bytes
    (nobody verifies it)"""
    h = bytearray(HEAD)
    h[3] = flg
    if flg & 4:
        h += len(extra).to_bytes(2, "little") + extra
    if flg & 8:
        h += name + b"\0"
    if flg & 16:
        h += comment + b"\0"
    if flg & 2:
        h += b"\0\0"
    body = raw(data, **kw) if body is None else body
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) if isize is None else isize
    return bytes(h) + body + crc.to_bytes(4, "little") + (isize & 0xFFFFFFFF).to_bytes(4, "little")


def join(parts, level=6):
    return b"".join(member(p, level=level) for p in parts)


def pieces(n, size, seed):
    t = text(n, seed)
    return [t[i: i + size] for i in range(0, n, size)]


def stored_first(data, cut=100):
    """a raw stream whose first block is a stored one"""
    b = SC.Builder()
    b.stored(data[:cut])
    b.stored(data[cut:], final=True)
    return b.bw.bytes().tobytes()


def fixed_first(data):
    """a raw stream of one fixed block of literals"""
    b = SC.Builder()
    b.fixed(list(data), final=True)
    return b.bw.bytes().tobytes()


def reach_back(fill=0, dist=5):
    """a raw stream of `fill` literals in dynamic blocks, then a block that opens with a match of distance fill + dist"""
    rng = np.random.default_rng(fill + dist)
    b = SC.Builder()
    for at in range(0, fill, 4000):
        b.dynamic([int(x) for x in rng.integers(97, 123, min(4000, fill - at))])
    b.dynamic([W.match(10, fill + dist)] + [int(x) for x in rng.integers(97, 123, 300)], final=True, expand=False)
    return b.bw.bytes().tobytes()


def good():
    """{name: file}"""
    t = text(9000, 1)
    a, b, c = t[:3000], t[3000:6000], t[6000:]
    out = {
        "one": join([a]),
        "three": join([a, b, c]),
        "flags": member(a, flg=8, name=b"a.txt") + member(b, flg=4, extra=b"XY\x03\x00abc") +
                 member(c, flg=16, comment=b"a comment") + member(a[:10], flg=2) +
                 member(b[:10], flg=30, extra=b"", name=b"n", comment=b""),
        "empties": member(b"") + join([a]) + member(b"") + member(b"") + B.EOF,
        "bgzf_eof_alone": B.EOF,
        "zeros": join([a]) + bytes(1) + join([b]) + bytes(7) + join([c]) + bytes(1000),
        "stored_second": join([a]) + member(b, body=stored_first(b)) + join([c]),
        "fixed_second": join([a]) + member(b[:500], body=fixed_first(b[:500])) + join([c]),
        "z_fixed": join([a]) + member(b, strategy=zlib.Z_FIXED),
    }
    return out


def bad():
    """{name: (file, capacity, status)}"""
    t = text(6000, 2)
    a, b, c = t[:2000], t[2000:4000], t[4000:]
    three = join([a, b, c])
    ma, mb = member(a), member(b)
    type3 = bytes([0x07])  # BFINAL, BTYPE 3
    return {
        "empty": (b"", BIG, SC.SRC_TOO_SMALL),
        "garbage_behind": (ma + b"\x01" + bytes(range(2, 40)), BIG, SC.ERROR),
        "short_tail": (ma + bytes(9) + HEAD + b"\x03\x00" + bytes(5), BIG, SC.SRC_TOO_SMALL),
        "cut_in_trailer": (three[:-3], BIG, SC.SRC_TOO_SMALL),
        "wrong_isize": (ma + member(b, isize=len(b) + 1) + member(c), BIG, SC.ERROR),
        "wrong_crc_2_of_3": (ma + member(b, crc=zlib.crc32(b) ^ 1) + member(c), BIG, SC.ERROR),
        "reach_into_member_1": (ma + member(b"", body=reach_back()), BIG, SC.INVALID_DISTANCE),
        "capacity_one_short": (three, len(t) - 1, SC.DST_TOO_SMALL),
        "type3_in_member_3": (ma + mb + member(b"", body=type3 + bytes(8)), BIG, SC.INVALID_BLOCK_HEADER),
    }
