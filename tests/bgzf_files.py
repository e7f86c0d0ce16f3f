"""BGZF files made with Python's zlib (raw deflate per member), for the tests of the BGZF reader: members of chosen ISIZE,
with foreign extra subfields, of bgzip's 65280 bytes, stored members whose payload holds a byte-exact fake member header, and
damaged ones.  walk() is a pure-Python BGZF walker, the yardstick the parsers (sf_bgzf_plan.h on the host, the device walk)
are held against."""
import struct
import zlib

import numpy as np

EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
ERROR, SRC_TOO_SMALL = 1, 5


def text(n, seed=0):
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, size=int(k), dtype=np.uint8)) for k in rng.integers(2, 9, size=300)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + b" "
    return bytes(out[:n])


def subfield(si, data):
    return si + struct.pack("<H", len(data)) + data


def member(payload, level=6, before=b"", behind=b"", flg=4):
    """one BGZF member of `payload`: before / behind are whole subfields around 'BC'"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(payload) + c.flush()
    xlen = len(before) + 6 + len(behind)
    size = 12 + xlen + len(body) + 8
    assert size <= 65536
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff" + struct.pack("<H", xlen)
    return (head + before + subfield(b"BC", struct.pack("<H", size - 1)) + behind + body +
            struct.pack("<II", zlib.crc32(payload), len(payload)))


def write(data, sizes, eof=True, **kw):
    """`data` cut into members of the given payload sizes (their sum is len(data)) -> (file, member_off, out_off)"""
    assert sum(sizes) == len(data)
    blob, moff, ooff, at = b"", [], [], 0
    for n in sizes:
        moff.append(len(blob))
        ooff.append(at)
        blob += member(data[at: at + n], **kw)
        at += n
    if eof:
        moff.append(len(blob))
        ooff.append(at)
        blob += EOF
    return blob, moff + [len(blob)], ooff + [at]


SIZES = [0, 1, 100, 32768, 31, 0]


def good_files():
    """name -> (data, file, member_off, out_off, has_eof); every member at most 32 KiB unless the name says 65280"""
    out = {}
    data = text(sum(SIZES), seed=1)
    for eof in (True, False):  # (the last, empty member is byte for byte the EOF member: has_eof holds without one appended)
        out[f"sizes eof={eof}"] = (data,) + write(data, SIZES, eof=eof) + (True,)
    out["no EOF member"] = (data[:131],) + write(data[:131], [100, 31], eof=False) + (False,)
    other = subfield(b"XY", b"hello")
    out["subfield before BC"] = (data,) + write(data, SIZES, before=other) + (True,)
    out["subfield behind BC"] = (data,) + write(data, SIZES, behind=other + subfield(b"ZZ", b"")) + (True,)
    out["a BC of three bytes before BC"] = (data,) + write(data, SIZES, before=subfield(b"BC", b"abc")) + (True,)
    rnd = np.random.default_rng(5).integers(0, 256, 3 * 32768 + 5, dtype=np.uint8).tobytes()
    out["stored members"] = (rnd,) + write(rnd, [32768, 32768, 32768, 5], level=0) + (True,)
    big = text(3 * 65280, seed=2)
    out["65280-byte members"] = (big,) + write(big, [65280] * 3) + (True,)
    for name, (d, f, m, o, e) in fake_header_files().items():
        out[name] = (d, f, m, o, e)
    return out


def fake_header_files():
    """A stored member whose payload holds a byte-exact member header: one whose BSIZE + 1 lands in the middle of the data,
    one whose BSIZE + 1 lands exactly on the next true member's first byte.  Neither is reached from byte 0."""
    out = {}
    tail = text(5000, seed=3)
    for name, land in (("fake header into the data", None), ("fake header onto a member start", "next")):
        payload = bytearray(np.random.default_rng(7).integers(0, 256, 20000, dtype=np.uint8).tobytes())
        k = 1001  # the fake header's place in the payload; a stored block's payload starts 5 bytes into the body
        first_size = len(member(bytes(payload), level=0))
        at = 18 + 5 + k
        bsize = (first_size - at - 1) if land == "next" else 3000
        payload[k: k + 18] = EOF[:16] + struct.pack("<H", bsize)
        data = bytes(payload) + tail
        blob, moff, ooff = write(data, [len(payload), len(tail)], level=0)
        assert blob[at: at + 16] == EOF[:16] and (land != "next" or at + bsize + 1 == moff[1])
        out[name] = (data, blob, moff, ooff, True)
    return out


class WalkError(Exception):
    def __init__(self, status):
        super().__init__(f"DecompressStatus {status}")
        self.status = status


def walk(blob):
    """-> (member_off, out_off, max_isize, has_eof) as include/starflate_hip.h states them; WalkError(1 or 5) otherwise"""
    n, at, out, moff, ooff, widest, last = len(blob), 0, 0, [], [], 0, None
    while at < n:
        if n - at < 12:
            raise WalkError(SRC_TOO_SMALL)
        if blob[at: at + 3] != b"\x1f\x8b\x08" or not blob[at + 3] & 4:
            raise WalkError(ERROR)
        xlen = struct.unpack_from("<H", blob, at + 10)[0]
        if n - at < 12 + xlen:
            raise WalkError(SRC_TOO_SMALL)
        x, bsize = 0, None
        while x < xlen:
            if x + 4 > xlen:
                raise WalkError(ERROR)
            slen = struct.unpack_from("<H", blob, at + 12 + x + 2)[0]
            if x + 4 + slen > xlen:
                raise WalkError(ERROR)
            if bsize is None and blob[at + 12 + x: at + 12 + x + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", blob, at + 12 + x + 4)[0]
            x += 4 + slen
        if bsize is None or bsize + 1 < 12 + xlen + 8:
            raise WalkError(ERROR)
        if n - at < bsize + 1:
            raise WalkError(SRC_TOO_SMALL)
        isize = struct.unpack_from("<I", blob, at + bsize + 1 - 4)[0]
        moff.append(at)
        ooff.append(out)
        last = blob[at: at + bsize + 1]
        widest = max(widest, isize)
        at += bsize + 1
        out += isize
    return moff + [n], ooff + [out], widest, last == EOF


def patched(blob, at, new):
    return blob[:at] + new + blob[at + len(new):]


def damaged():
    """(name, file, expected status): every outcome the header states for a file that does not parse"""
    data = text(40000, seed=4)
    good, moff, _ = write(data, [20000, 20000])
    second = moff[1]
    return [
        ("BSIZE too small", patched(good, second + 16, struct.pack("<H", 24)), ERROR),
        ("BSIZE past the end", patched(good, second + 16, struct.pack("<H", 0xFFFF)), SRC_TOO_SMALL),
        ("cut inside a header", good[: second + 7], SRC_TOO_SMALL),
        ("cut inside the extra field", good[: second + 14], SRC_TOO_SMALL),
        ("cut inside a body", good[: second + 500], SRC_TOO_SMALL),
        ("FEXTRA cleared", patched(good, second + 3, b"\0"), ERROR),
        ("bad magic", patched(good, 0, b"\x1e"), ERROR),
        ("bad CM", patched(good, second + 2, b"\x07"), ERROR),
        ("no BC subfield", patched(good, 12, b"BD"), ERROR),
        ("BC of three bytes only", patched(write(data, [20000, 20000], before=subfield(b"BC", b"abc"))[0], 19, b"BD"), ERROR),
        ("a subfield overrunning XLEN", patched(good, 14, struct.pack("<H", 3)), ERROR),
        ("a subfield header overrunning XLEN", patched(good, 10, struct.pack("<H", 3)), ERROR),
        ("garbage behind the EOF member", good + b"\0" * 40, ERROR),
    ]
