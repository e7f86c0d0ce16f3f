"""Raw DEFLATE bodies that decode to more than 32 KiB -- what a BGZF member of bgzip's 65280 bytes, or of the format's 65536,
holds -- for the tests of the decoder's wide rows: made with Python's zlib in every block shape, and by hand
(tests/deflate_writer.py) with the matches a 32 KiB segment never sees.  hand_member() wraps a body as a BGZF member.
TEST INFRASTRUCTURE ONLY."""
import struct
import zlib

import numpy as np

import bgzf_files as BZ
import deflate_writer as W

WIDE = 65280  # what bgzip and htslib put into a member


def hand_member(body, payload):
    """a BGZF member around a raw DEFLATE body that decodes to `payload` (or is meant to: CRC-32 and ISIZE are payload's)"""
    body = bytes(body)
    size = 18 + len(body) + 8
    assert size <= 65536, size
    return BZ.EOF[:16] + struct.pack("<H", size - 1) + body + struct.pack("<II", zlib.crc32(payload), len(payload))


def zlib_body(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if not flush_every:
        return c.compress(payload) + c.flush()
    body = b"".join(c.compress(payload[k: k + flush_every]) + c.flush(zlib.Z_SYNC_FLUSH) for k in range(0, len(payload), flush_every))
    return body + c.flush()


def nibbles(n, seed):
    """random bytes of a 16-symbol alphabet: zlib -6 finds little to match and cuts a block every 16383 symbols"""
    return bytes(np.random.default_rng(seed).integers(0, 16, n, dtype=np.uint8) * 17)


def shape_cases():
    """name -> (payload, body): the block shapes of a 65280-byte member"""
    out = {}
    txt = BZ.text(WIDE, seed=5)
    out["one coded block"] = (txt, zlib_body(txt))
    nib = nibbles(WIDE, 6)
    out["nibbles, four blocks or more"] = (nib, zlib_body(nib))
    assert len(out["nibbles, four blocks or more"][1]) > 30000
    out["fixed"] = (txt, zlib_body(txt, strategy=zlib.Z_FIXED))
    rnd = np.random.default_rng(8).integers(0, 256, WIDE, dtype=np.uint8).tobytes()
    body = zlib_body(rnd, level=0)
    assert len(body) == WIDE + 10 and body[:5] == b"\x00\x00\xff\xff\x00"  # LEN 0xFF00, then the empty final block
    out["one stored block above the window"] = (rnd, body)
    bw = W.BitWriter()
    W.write_stored(bw, rnd[:40000])
    W.write_stored(bw, rnd[40000:], final=True)
    out["two stored blocks"] = (rnd, bw.bytes().tobytes())
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    head = c.compress(txt[:30000]) + c.flush(zlib.Z_FULL_FLUSH)
    bw = W.BitWriter()
    W.write_stored(bw, txt[30000:], final=True)
    out["a coded block, then a stored one"] = (txt, head + bw.bytes().tobytes())
    out["14 flushed blocks"] = (txt, zlib_body(txt, flush_every=5000))
    return out


def _lits(n, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 16, n, dtype=np.uint8) * 17]


def body_of_tokens(tokens):
    """one final dynamic block of the tokens, whatever they stand for"""
    tk, ll, d, _ = W.huffman_block(tokens)
    bw = W.BitWriter()
    W.write_dynamic(bw, tk, ll, d, final=True)
    return bw.bytes().tobytes()


def far_cases():
    """name -> (payload, body): matches beyond a narrow row's reach"""
    out = {}
    # distance 32768 at output positions 32768, 40000 and 65535 - 258
    t = _lits(32768, 1) + [W.match(258, 32768)]
    t += _lits(40000 - (32768 + 258), 2) + [W.match(258, 32768)]
    t += _lits(65535 - 258 - (40000 + 258), 3) + [W.match(258, 32768)] + _lits(1, 4)
    out["distance 32768 at 32768, 40000, 65277"] = (W.expand(t), body_of_tokens(t))
    # distance 1 runs across byte 32768; a match of 258 that ends exactly on byte 65536
    t = _lits(32500, 5) + [W.match(258, 1), W.match(258, 1)]
    t += _lits(65536 - 258 - 33016, 6) + [W.match(258, 32768)]
    out["runs across 32768, a match ending on 65536"] = (W.expand(t), body_of_tokens(t))
    # a match of 258 that straddles byte 32768
    t = _lits(32700, 7) + [W.match(258, 1234)] + _lits(WIDE - 32958, 8)
    out["a match straddling 32768"] = (W.expand(t), body_of_tokens(t))
    assert [len(p) for p, _ in out.values()] == [65536, 65536, WIDE]
    for p, b in out.values():
        assert zlib.decompress(b, -15) == p
    return out


def invalid_distance():
    """-> (body, bytes it claims): a match at position 100 with distance 101"""
    t = _lits(100, 9) + [W.match(10, 101)] + _lits(40000 - 110, 10)
    return body_of_tokens(t), 40000
