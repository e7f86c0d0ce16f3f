"""BGZF files made with Python's zlib (raw deflate per member), for the tests of the BGZF reader: members of chosen ISIZE,
with foreign extra subfields, of bgzip's 65280 bytes, stored members whose payload holds a byte-exact fake member header, and
damaged ones.  walk() is a pure-Python BGZF walker, the yardstick the parsers (sf_bgzf_plan.h on the host, the device walk)
are held against."""
import functools
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


def member(payload, level=6, before=b"", behind=b"", flg=4, body=None):
    """one BGZF member of `payload`: before / behind are whole subfields around 'BC'; body: its DEFLATE bytes where zlib is not
    to write them"""
    if body is None:
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


def parse_at(blob, at):
    """the member that starts at byte `at` < len(blob) -> (its bytes, its ISIZE); WalkError(1 or 5) when none parses there"""
    n = len(blob)
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
    return bsize + 1, struct.unpack_from("<I", blob, at + bsize + 1 - 4)[0]


def walk(blob):
    """-> (member_off, out_off, max_isize, has_eof) as include/starflate_hip.h states them; WalkError(1 or 5) otherwise"""
    n, at, out, moff, ooff, widest, last = len(blob), 0, 0, [], [], 0, None
    while at < n:
        size, isize = parse_at(blob, at)
        moff.append(at)
        ooff.append(out)
        last = blob[at: at + size]
        widest = max(widest, isize)
        at += size
        out += isize
    return moff + [n], ooff + [out], widest, last == EOF


def node_positions(blob):
    """every byte position at which walk()'s own parse of one member succeeds: the nodes of the device walk, whether the
    chain from byte 0 reaches them or not"""
    out, at = [], blob.find(b"\x1f\x8b\x08")
    while at != -1:
        try:
            parse_at(blob, at)
            out.append(at)
        except WalkError:
            pass
        at = blob.find(b"\x1f\x8b\x08", at + 1)
    return out


def parse_nodes(blob):
    return len(node_positions(blob))


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


# ---- files for the member walk beyond one workgroup, one scan tile and one run of k_bgzf_finish (tests/test_gpu_walk_scale.py;
# tests/test_walk_scale_inputs.py holds every count and position stated here, without a GPU) ----
CHAIN_NODES = (1, 2, 3, 4, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 5000)
HEAD = 18  # a member's header with the 'BC' subfield alone
SEAMS = (8192, 16384)  # k_bgzf_scan's workgroups of 256 lanes x 32 positions
SEAM_REACH = 35
CUTS = tuple(range(1, 13)) + (16, 17, 18)


@functools.lru_cache(maxsize=None)
def tiny_members(count=5055, seed=21):
    """-> (data, members, sizes): `count` members of 0 .. 79 bytes of text each, level 6"""
    rng = np.random.default_rng(seed)
    sizes = [int(v) for v in rng.integers(0, 80, count)]
    data = text(sum(sizes), seed=seed)
    members, at = [], 0
    for n in sizes:
        members.append(member(data[at: at + n]))
        at += n
    return data, members, sizes


@functools.lru_cache(maxsize=None)
def chain_file(nodes):
    """-> (data, file, member_off, out_off): nodes - 1 tiny members and the EOF member, nothing else that parses"""
    data, members, sizes = tiny_members()
    m = nodes - 1
    moff, ooff = [0], [0]
    for k in range(m):
        moff.append(moff[-1] + len(members[k]))
        ooff.append(ooff[-1] + sizes[k])
    blob = b"".join(members[:m]) + EOF
    return data[: ooff[-1]], blob, moff + [len(blob)], ooff + [ooff[-1]]


def stored_member(payload, **kw):
    """one member whose body is a single stored block: the payload lies at its bytes [HEAD + 5, HEAD + 5 + len) when it has
    no further subfield"""
    assert len(payload) < 65536
    return member(payload, body=b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xFFFF) + payload, **kw)


def fake_head(size):
    """18 bytes that parse as a member of `size` bytes wherever `size` bytes follow their first one"""
    assert 26 <= size <= 65536
    return EOF[:16] + struct.pack("<H", size - 1)


def decoy_payload(count):
    """`count` fake heads back to back: each lands on the one two ahead (two interleaved chains), the last of either chain on
    the first byte behind the stored member's trailer"""
    return b"".join(fake_head(36 if k + 2 < count else 18 * (count - k) + 8) for k in range(count))


@functools.lru_cache(maxsize=None)
def decoy_file(counts):
    """-> (data, file, member_off, out_off, nodes): one stored member of decoy_payload(c) per c in counts, a member of text
    whose own extra field holds a fake head (a foreign subfield 'XY' in front of 'BC') that lands on the member behind it,
    the EOF member.  nodes = sum(counts) + len(counts) + 3"""
    tail = text(3000, seed=9)
    payloads = [decoy_payload(c) for c in counts]
    parts = [stored_member(p) for p in payloads]
    size = len(member(tail, before=subfield(b"XY", fake_head(26))))
    parts.append(member(tail, before=subfield(b"XY", fake_head(size - 16))))  # (the subfield's data starts at byte 16)
    parts.append(EOF)
    moff, ooff = [0], [0]
    for p, n in zip(parts, [len(p) for p in payloads] + [len(tail), 0]):
        moff.append(moff[-1] + len(p))
        ooff.append(ooff[-1] + n)
    blob = b"".join(parts)
    return b"".join(payloads) + tail, blob, moff[:-1] + [len(blob)], ooff, sum(counts) + len(counts) + 3


def decoy_file_of(nodes):
    """a file of three members and exactly `nodes` nodes"""
    return decoy_file((nodes - 4,))


@functools.lru_cache(maxsize=None)
def _seam_parts():
    d = [text(n, seed=40 + k) for k, n in enumerate((14000, 14000, 500))]
    return d, len(member(d[0], behind=subfield(b"XY", b""))), len(member(d[1]))


def seam_file(which, start):
    """-> (data, file, member_off, out_off): three members of text and the EOF member; member `which` (1 or 2, counted from
    0) starts at byte `start`, moved there by the length of a foreign subfield in member 0"""
    d, base, second = _seam_parts()
    pad = start - base - (second if which == 2 else 0)
    assert 0 <= pad < 60000
    parts = [member(d[0], behind=subfield(b"XY", bytes(pad))), member(d[1]), member(d[2]), EOF]
    moff, ooff = [0], [0]
    for p, n in zip(parts, [len(x) for x in d] + [0]):
        moff.append(moff[-1] + len(p))
        ooff.append(ooff[-1] + n)
    assert moff[which] == start
    return b"".join(d), b"".join(parts), moff[:-1] + [moff[-1]], ooff


def seam_starts():
    return [(which, seam + d) for which, seam in zip((1, 2), SEAMS) for d in range(-SEAM_REACH, SEAM_REACH + 1)]


def no_eof_files():
    """four files without an EOF member, their lengths 0, 1, 2 and 3 above a multiple of 4 (in some order)"""
    a, b = text(100, seed=50), text(31, seed=51)
    out = []
    for k in range(4):
        blob = member(a) + member(b, behind=subfield(b"XY", bytes(k)))
        out.append((a + b, blob))
    return out


def cut_files():
    """(k, file, status): damaged()'s good file cut k bytes into its second member, and what walk() says of it"""
    data = text(40000, seed=4)
    good, moff, _ = write(data, [20000, 20000])
    out = []
    for k in CUTS:
        try:
            walk(good[: moff[1] + k])
            st = 0
        except WalkError as e:
            st = e.status
        out.append((k, good[: moff[1] + k], st))
    return out


@functools.lru_cache(maxsize=None)
def tile_file(members=300):
    """-> (data, file, member_off, out_off): stored members of 32768 random bytes, more than 1024 workgroups of the scan"""
    data = np.random.default_rng(60).integers(0, 256, members * 32768, dtype=np.uint8).tobytes()
    return (data,) + write(data, [32768] * members, level=0)
