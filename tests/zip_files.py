"""ZIP archives for the tests, in pure Python (struct): the writer's defining property restated (assemble), a walker that
finds the end record, the directory records and every entry's data the way sf_zip_plan.h states it, the foreign archives the
readers are checked on (made by zipfile and numpy) and the damage catalogue with one expected status each."""
import io
import struct
import zipfile
import zlib

import numpy as np

UNSUPPORTED = 0xFFFFFFF9  # SFH_ZIP_ENTRY_UNSUPPORTED
OK, ERROR, DST_TOO_SMALL, SRC_TOO_SMALL = 0, 1, 4, 5
ENTRY_BYTES = 64  # sizeof(sfh_zip_entry)
ENTRY_DTYPE = np.dtype([("local_off", "<u8"), ("data_off", "<u8"), ("csize", "<u8"), ("usize", "<u8"), ("out_off", "<u8"),
                        ("name_off", "<u8"), ("crc32", "<u4"), ("status", "<u4"), ("method", "<u2"), ("flags", "<u2"),
                        ("name_len", "<u2"), ("pad", "<u2")])
assert ENTRY_DTYPE.itemsize == ENTRY_BYTES


# ---- the writer, restated ----
def local_header(name, crc, csize, usize):
    return struct.pack("<4sHHHHHIIIHH", b"PK\3\4", 20, 0x0800, 8, 0, 0x0021, crc, csize, usize, len(name), 0) + name


def central_record(name, crc, csize, usize, local_off):
    return struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\1\2", 20, 20, 0x0800, 8, 0, 0x0021, crc, csize, usize, len(name), 0, 0, 0, 0, 0,
                       local_off) + name


def end_records(entries, cd_off, cd_size):
    out = b""
    if entries > 65535:
        out += struct.pack("<4sQHHIIQQQQ", b"PK\6\6", 44, 45, 45, 0, 0, entries, entries, cd_size, cd_off)
        out += struct.pack("<4sIQI", b"PK\6\7", 0, cd_off + cd_size, 1)
    n16 = min(entries, 0xFFFF) if entries <= 65535 else 0xFFFF
    return out + struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, n16, n16, cd_size, cd_off, 0)


def assemble(names, bodies, datas):
    """The archive the writer must produce: for every item its local header and raw DEFLATE body, the directory, the end."""
    out, cd = bytearray(), bytearray()
    for name, body, data in zip(names, bodies, datas):
        crc = zlib.crc32(data) & 0xFFFFFFFF
        cd += central_record(name, crc, len(body), len(data), len(out))
        out += local_header(name, crc, len(body), len(data))
        out += body
    cd_off = len(out)
    return bytes(out + cd + end_records(len(names), cd_off, len(cd)))


def compress_bound(n):
    return max(1, -(-n // 32768)) * (32768 + 4096 + 640)


def zip_bound(sizes, name_lens):
    return sum(30 + k + compress_bound(n) for n, k in zip(sizes, name_lens)) + sum(46 + k for k in name_lens) + 22 + 76


def test_names(count):
    """names of 1 to 17 bytes, then a 255-byte one and a non-ASCII one, cycled and made unique"""
    base = [("n%02d" % k + "x" * 17)[: k + 1] if k >= 2 else "ab"[: k + 1] for k in range(17)] + ["L" * 250 + "%05d", "grüße-世界.txt"]
    out = []
    for i in range(count):
        b = base[i % len(base)]
        if "%05d" in b:
            b = b % i
        elif i >= len(base):
            b = "%s.%d" % (b, i)
        out.append(b.encode("utf-8"))
    assert len(set(out)) == len(out)
    return out


# ---- the reader, restated ----
def _eocd(d):
    n = len(d)
    for q in range(n - 22, max(n - 22 - 65535, 0) - 1, -1):
        if d[q:q + 4] == b"PK\5\6" and q + 22 + struct.unpack_from("<H", d, q + 20)[0] == n:
            return q
    return None


def walk(d):
    """(index status, info dict, list of entry dicts): sf_zip_plan.h's rules, written independently"""
    d = bytes(d)
    n = len(d)
    if n < 22:
        return SRC_TOO_SMALL, None, []
    q = _eocd(d)
    if q is None:
        return ERROR, None, []
    disk, cd_disk, here, entries, cd_size, cd_off, _ = struct.unpack_from("<HHHHIIH", d, q + 4)
    if disk or cd_disk or here != entries:
        return ERROR, None, []
    end_at, z64 = q, 0
    if (entries == 0xFFFF or cd_size == 0xFFFFFFFF or cd_off == 0xFFFFFFFF) and q >= 20 and d[q - 20:q - 16] == b"PK\6\7":
        if q < 76:
            return ERROR, None, []
        ldisk, roff, disks = struct.unpack_from("<IQI", d, q - 16)
        end_at = q - 76
        if ldisk or disks > 1 or roff != end_at or d[end_at:end_at + 4] != b"PK\6\6":
            return ERROR, None, []
        size, _, _, rdisk, rcd, here, entries, cd_size, cd_off = struct.unpack_from("<QHHIIQQQQ", d, end_at + 4)
        if size != 44 or rdisk or rcd or here != entries:
            return ERROR, None, []
        z64 = 1
    if cd_off > end_at or cd_size != end_at - cd_off or entries > cd_size // 46:
        return ERROR, None, []
    at, out, o = cd_off, [], 0
    for _ in range(entries):
        if end_at - at < 46 or d[at:at + 4] != b"PK\1\2":
            return ERROR, None, []
        (_, _, flags, method, _, _, crc, csize, usize, nlen, xlen, clen, _, _, _, loff) = struct.unpack_from("<HHHHHHIIIHHHHHII", d, at + 4)
        if end_at - at - 46 < nlen + xlen + clen:
            return ERROR, None, []
        x, k = d[at + 46 + nlen: at + 46 + nlen + xlen], 0
        while xlen - k >= 4:
            sid, slen = struct.unpack_from("<HH", x, k)
            if slen > xlen - k - 4:
                return ERROR, None, []
            if sid == 1:
                u = 0
                vals = [usize, csize, loff]
                for j, v in enumerate(vals):
                    if v == 0xFFFFFFFF:
                        if slen - u < 8:
                            return ERROR, None, []
                        vals[j] = struct.unpack_from("<Q", x, k + 4 + u)[0]
                        u += 8
                usize, csize, loff = vals
            k += 4 + slen
        st = OK
        if method not in (0, 8) or flags & (1 | 1 << 5 | 1 << 6 | 1 << 13):
            st = UNSUPPORTED
        elif method == 0 and csize != usize:
            st = ERROR
        out.append(dict(local_off=loff, data_off=0, csize=csize, usize=usize, out_off=o, name_off=at + 46, crc32=crc, status=st,
                        method=method, flags=flags, name_len=nlen, name=d[at + 46: at + 46 + nlen]))
        o += (usize + 15) & ~15
        at += 46 + nlen + xlen + clen
    if at != end_at:
        return ERROR, None, []
    for e in out:
        if e["status"]:
            continue
        lo = e["local_off"]
        if lo > cd_off or cd_off - lo < 30:
            e["status"] = SRC_TOO_SMALL
        elif d[lo:lo + 4] != b"PK\3\4":
            e["status"] = ERROR
        else:
            nl, xl = struct.unpack_from("<HH", d, lo + 26)
            data = lo + 30 + nl + xl
            if data > cd_off or cd_off - data < e["csize"]:
                e["status"] = SRC_TOO_SMALL
            else:
                e["data_off"] = data
    return OK, dict(entries=entries, cd_off=cd_off, cd_size=cd_size, total_out=o, zip64=z64), out


# ---- foreign archives ----
def text(n, seed=0):
    rng = np.random.default_rng(seed)
    words = [b"archive", b"entry", b"deflate", b"central", b"directory", b"the", b"of", b"record", b"offset", b"stored", b"\n", b"zip"]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(len(words)))] + b" "
    return bytes(out[:n])


class _Unseekable(io.RawIOBase):
    """what zipfile writes data descriptors for (flag bit 3): a stream that cannot seek"""

    def __init__(self):
        self.buf = bytearray()

    def writable(self):
        return True

    def write(self, b):
        self.buf += b
        return len(b)


def _zip(entries, comment=b"", unseekable=False):
    """entries: (ZipInfo or name, data, kwargs of writestr)"""
    f = _Unseekable() if unseekable else io.BytesIO()
    with zipfile.ZipFile(f, "w") as z:
        for name, data, kw in entries:
            z.writestr(name, data, **kw)
        z.comment = comment
    return bytes(f.buf) if unseekable else f.getvalue()


def _info(name, method, extra=b"", comment=b""):
    zi = zipfile.ZipInfo(name, date_time=(2001, 2, 3, 4, 5, 6))
    zi.compress_type = method
    zi.extra = extra
    zi.comment = comment
    return zi


def foreign_archives():
    """name -> archive bytes: every kind of foreign archive the issue lists (small: the GPU tests add the large entries)"""
    D, S = zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED
    t = text(5000, 1)
    A = {}
    A["levels"] = _zip([("l1.txt", t, dict(compress_type=D, compresslevel=1)), ("l6.txt", t, dict(compress_type=D, compresslevel=6)),
                        ("l9.txt", t, dict(compress_type=D, compresslevel=9)), ("s.txt", t, dict(compress_type=S))])
    names = [("n%02d" % k + "y" * 17)[: k + 1] if k >= 2 else "cd"[: k + 1] for k in range(17)] + ["M" * 255, "grüße-世界.bin"]
    A["names"] = _zip([(nm, text(40 + 3 * i, i), dict(compress_type=S if i % 2 else D)) for i, nm in enumerate(names)])
    A["comments"] = _zip([(_info("a.txt", D, extra=struct.pack("<HH4s", 0x7075, 4, b"abcd"), comment=b"entry comment"), t, {}),
                          (_info("b.txt", S, comment=b"x" * 300), t[:100], {})], comment=b"the archive's comment")
    A["patterns"] = _zip([(_info("p.bin", S, extra=struct.pack("<HH8s", 0x6666, 8, b"PK\1\2PK\3\4"), comment=b"PK\1\2 not a record PK\5\6"),
                           b"PK\3\4" * 10 + b"PK\1\2" * 10 + b"PK\5\6" + bytes(18), {}), ("q.txt", t, dict(compress_type=D))],
                         comment=b"PK\1\2 inside the comment")
    A["descriptor"] = _zip([("d1.txt", t, dict(compress_type=D)), ("d2.bin", t[:333], dict(compress_type=S))], unseekable=True)
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w") as z:
        for nm, m in (("z64-deflated", D), ("z64-stored", S)):
            zi = zipfile.ZipInfo(nm)
            zi.compress_type = m
            with z.open(zi, "w", force_zip64=True) as w:
                w.write(t)
    A["zip64_entries"] = f.getvalue()
    # a directory record whose sizes and offset are all saturated and stand in its 0x0001 extra (behind another subfield)
    body = zlib.compress(t, 6)[2:-4]
    crc = zlib.crc32(t)
    first = local_header(b"pad", 0, 2, 0) + b"\3\0"
    loc = local_header(b"big.txt", crc, len(body), len(t)) + body
    x = struct.pack("<HH2s", 0x9999, 2, b"zz") + struct.pack("<HHQQQ", 1, 24, len(t), len(body), len(first))
    rec = struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\1\2", 45, 45, 0x0800, 8, 0, 0x0021, crc, 0xFFFFFFFF, 0xFFFFFFFF, 7, len(x), 0, 0, 0, 0,
                      0xFFFFFFFF) + b"big.txt" + x
    cdir = central_record(b"pad", 0, 2, 0, 0) + rec
    A["zip64_directory"] = first + loc + cdir + end_records(2, len(first) + len(loc), len(cdir))
    f = io.BytesIO()
    np.savez(f, a=np.arange(1000, dtype=np.int32), b=np.linspace(0, 1, 77), empty=np.zeros(0, np.uint8))
    A["npz"] = f.getvalue()
    f = io.BytesIO()
    np.savez_compressed(f, a=np.arange(20000, dtype=np.int64) % 97, b=np.zeros((3, 5)))
    A["npz_compressed"] = f.getvalue()
    A["empty"] = _zip([])
    return A


STORED_SIZES = (0, 1, 15, 16, 17, 32767, 32768, 32769, 3 * 32768 + 5)


def residue_archive(sizes=STORED_SIZES, method=zipfile.ZIP_STORED):
    """entries of every size at every data_off % 16: the name's length (1 to 16) places the data"""
    f = io.BytesIO()
    rng = np.random.default_rng(5)
    with zipfile.ZipFile(f, "w") as z:
        for n in sizes:
            for r in range(16):
                nlen = (r - f.tell() - 30) % 16 or 16
                name = ("%d_%d_" % (n, r) + "r" * 16)[:nlen]
                while name in z.namelist():
                    name = name[:-1] + chr(ord(name[-1]) + 1)
                z.writestr(name, rng.integers(0, 256, n, dtype=np.uint8).tobytes() if n % 2 else text(n, n + r), compress_type=method)
    return f.getvalue()


def many_empty(count=65536):
    """`count` empty stored entries: above 65535, zipfile writes the ZIP64 end record"""
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w") as z:
        for i in range(count):
            z.writestr("e%05d" % i, b"")
    return f.getvalue()


# ---- the damage catalogue: name -> (bytes, expected index status, {entry: expected status}) ----
def damage_catalogue():
    D, S = zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED
    t = text(3000, 7)
    good = _zip([("a.txt", t, dict(compress_type=D)), ("b.bin", t[:500], dict(compress_type=S)), ("c.txt", t[:900], dict(compress_type=D))])
    st, info, ents = walk(good)
    assert st == OK and all(e["status"] == 0 for e in ents)
    q = _eocd(good)
    cd = info["cd_off"]
    rec = [e["name_off"] - 46 for e in ents]

    def patch(at, fmt, *v):
        b = bytearray(good)
        struct.pack_into(fmt, b, at, *v)
        return bytes(b)

    C = {}
    C["no_end_record"] = (patch(q, "<I", 0x12345678), ERROR, {})
    C["below_22_bytes"] = (good[-21:], SRC_TOO_SMALL, {})
    C["count_too_large"] = (patch(q + 8, "<HH", 4, 4), ERROR, {})
    C["count_too_small"] = (patch(q + 8, "<HH", 2, 2), ERROR, {})
    C["chain_misses_the_end"] = (patch(rec[1] + 32, "<H", 1), ERROR, {})  # a comment length that is not there
    C["disk_number_1"] = (patch(q + 4, "<H", 1), ERROR, {})
    z64 = many_empty(65536)
    zq = _eocd(z64)
    b = bytearray(z64)
    struct.pack_into("<Q", b, zq - 20 + 8, len(z64) + 1000)
    C["zip64_locator_outside"] = (bytes(b), ERROR, {})
    C["bad_local_signature"] = (patch(ents[1]["local_off"], "<I", 0x04034B51), OK, {1: ERROR})
    C["data_past_directory"] = (patch(rec[2] + 20, "<I", ents[2]["csize"] + 1), OK, {2: SRC_TOO_SMALL})
    C["stored_sizes_differ"] = (patch(rec[1] + 24, "<I", 499), OK, {1: ERROR})
    bz = _zip([("a.txt", t, dict(compress_type=D)), ("z.bz2", t, dict(compress_type=zipfile.ZIP_BZIP2)), ("c.txt", t[:900], dict(compress_type=D))])
    C["method_12"] = (bz, OK, {1: UNSUPPORTED})
    C["flag_bit_0"] = (patch(rec[0] + 8, "<H", ents[0]["flags"] | 1), OK, {0: UNSUPPORTED})
    return C
