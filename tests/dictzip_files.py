"""A dictzip writer in Python for the tests of the table reader: zlib raw deflate, Z_FULL_FLUSH after every chunk, Z_FINISH,
and a gzip header whose FEXTRA field carries the 'RA' table -- with the variations real files show (the final block inside
or outside the last chunk's size, a file name, foreign subfields around 'RA', no chunk at all for an empty input)."""
import functools
import struct
import zlib

import numpy as np

CHLEN = 32768
SIZES = (0, 1, 32767, 32768, 32769, 3 * 32768 + 5)


def text(n, seed=1):
    """n bytes of compressible pseudo-text (words from a small vocabulary)"""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(300)]
    out = b" ".join(words[i] for i in rng.integers(0, len(words), n // 4 + 8))
    return out[:n]


def write(data, level=6, final="inside", fname=None, before=None, after=None, chcnt0=False, chlen=CHLEN, ver=1):
    """-> (file bytes, index): index[0] = the header's end, index[i + 1] = index[i] + the table's size[i], index[-1] =
    len(file) - 8 (the reader's convention: the last segment reaches to the trailer).
    final: "inside" -- the last chunk's size takes in the final block; "outside" -- it does not (dictzip(1) itself).
    fname: a file name (FNAME); before / after: (b"XY", payload) subfields in front of / behind 'RA'; chcnt0: an empty input
    written as CHCNT = 0."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    parts = []
    nch = max(1, -(-len(data) // chlen))
    for k in range(0 if chcnt0 else nch):
        parts.append(co.compress(data[k * chlen: (k + 1) * chlen]) + co.flush(zlib.Z_FULL_FLUSH))
    tail = co.flush(zlib.Z_FINISH)
    if chcnt0:
        assert not data
        sizes = []
    elif final == "inside":
        parts[-1] += tail
        tail = b""
        sizes = [len(p) for p in parts]
    else:
        sizes = [len(p) for p in parts]
    assert all(s < 65536 for s in sizes)
    ra = b"RA" + struct.pack("<HHHH", 6 + 2 * len(sizes), ver, chlen, len(sizes)) + struct.pack(f"<{len(sizes)}H", *sizes)
    extra = b""
    if before:
        extra += before[0] + struct.pack("<H", len(before[1])) + before[1]
    extra += ra
    if after:
        extra += after[0] + struct.pack("<H", len(after[1])) + after[1]
    flg = 4 | (8 if fname is not None else 0)
    head = bytes([0x1F, 0x8B, 8, flg, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H", len(extra)) + extra
    if fname is not None:
        head += fname + b"\0"
    body = b"".join(parts) + tail
    out = head + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)
    index = [len(head)]
    for s in sizes[: max(1, len(sizes)) - 1]:
        index.append(index[-1] + s)
    index.append(len(out) - 8)
    return out, index


VARIANTS = {
    "inside": dict(),
    "outside": dict(final="outside"),
    "fname": dict(fname=b"words.txt"),
    "before": dict(before=(b"XY", b"hello")),
    "after": dict(after=(b"ZZ", b"")),
    "all": dict(final="outside", fname=b"a", before=(b"AB", b"\x01\x02\x03"), after=(b"CD", b"tail-of-extra")),
}


# ---- tables longer than k_dz_index's 1024 lanes (tests/test_gpu_walk_scale.py, tests/test_walk_scale_inputs.py) ----
SCALE_CHUNKS = (1023, 1024, 1025, 2048, 2049, 4100)
MAX_CHUNKS = 32762  # XLEN = 10 + 2 * CHCNT is 16 bits wide


@functools.lru_cache(maxsize=None)
def scale_file(chunks):
    """-> (file, index): `chunks` chunks of zeros, level 1"""
    return write(bytes(chunks * CHLEN), level=1)


@functools.lru_cache(maxsize=None)
def limit_file(chunks=MAX_CHUNKS, seed=3):
    """-> (file, index): a header whose table holds `chunks` sizes of 20 .. 60 and an ISIZE to match, in front of that many
    placeholder bytes: for the table reader alone, nothing in it decodes"""
    sizes = [int(v) for v in np.random.default_rng(seed).integers(20, 61, chunks)]
    ra = b"RA" + struct.pack("<HHHH", 6 + 2 * chunks, 1, CHLEN, chunks) + struct.pack(f"<{chunks}H", *sizes)
    head = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF]) + struct.pack("<H", len(ra)) + ra
    out = head + bytes(sum(sizes)) + struct.pack("<II", 0, chunks * CHLEN)
    index = [len(head)]
    for s in sizes:
        index.append(index[-1] + s)
    assert index[-1] == len(out) - 8
    return out, index


def good_files(levels=(0, 6), sizes=SIZES):
    """{name: (data, file, index)} over sizes x variants x levels, plus CHCNT = 0 for the empty input"""
    out = {}
    for n in sizes:
        data = text(n, seed=n + 1)
        for level in levels:
            for vn, kw in VARIANTS.items():
                out[f"{n}-{vn}-l{level}"] = (data,) + write(data, level=level, **kw)
    out["0-chcnt0"] = (b"",) + write(b"", chcnt0=True)
    return out
