"""The walk rule of DESIGN.md 3a in plain Python: the segment index of a block-flushed DEFLATE stream, from the stream alone.

TEST INFRASTRUCTURE: the specification the GPU's recovered index (sfh_recover_index*) is compared with.
"""
import zlib

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
