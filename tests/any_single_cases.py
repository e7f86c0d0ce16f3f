"""What tests/test_gpu_any_single_record.py runs: the single index-free calls (sfh_decompress_any*, sfh_recover_index*) on the
smallest shapes at which mapping one stream onto item 0 of a batch can go wrong, and the record the commit before that mapping
left of them (tests/golden/any_single_parent.json).  Every case is (name, context, entry point, stream, container, dst_n,
options); run_case returns what the call said (the record's fields) and, for a decode, the destination's bytes."""
import ctypes as C
import gzip
import hashlib
import json
import os
import struct
import zlib

import numpy as np
import torch

import unindexed_walk as W
from conftest import GOLDEN
from single_decode_cases import context_under
from starflate_amd import _capi
from test_gpu_any_batch import _data, _stream_of_length_0_mod_4, _stream_with_a_marker_at_2_mod_4

SEG = 32768
FILL, GUARD = 0xA5, 16
TRAILER = _capi.SIZE_FROM_TRAILER
KIND = {"raw": 0, "zlib": 1, "gzip": 2}
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
GOLDEN_JSON = os.path.join(GOLDEN, "any_single_parent.json")
SIZES = (0, 1, 32767, 32768, 32769, 65536, 65537, 7 * SEG - 5)
KINDS = ("text", "noise", "zeros", "noisehead")
CONTEXTS = {"default": {}, "serial": {"SFH_INFLATE_SERIAL": "1"}, "cap2": {"SFH_BATCH_CHUNKS": "2"}}


def parent_record():
    with open(GOLDEN_JSON) as f:
        return json.load(f)


def nseg_of(n):
    return max(1, -(-n // SEG))


def sha(b):
    return hashlib.sha256(b).hexdigest()


def contexts():
    return {name: context_under(**env) for name, env in CONTEXTS.items()}


def zlib_says(stream, n, container):
    """the first n bytes zlib decodes from the stream (fewer where the stream holds fewer), or None where zlib refuses it"""
    try:
        out = zlib.decompressobj(WBITS[container]).decompress(bytes(stream))
    except zlib.error:
        return None
    return out[:n]


def _gzip_around(body, data, flags=0, name=b"name.txt"):
    hdr = bytearray(b"\x1f\x8b\x08" + bytes([flags]) + b"\x00\x00\x00\x00\x00\xff")
    if flags & 0x04:
        hdr += struct.pack("<H", 6) + b"xtra!!"
    if flags & 0x08:
        hdr += name + b"\x00"
    if flags & 0x10:
        hdr += b"a comment\x00"
    if flags & 0x02:
        hdr += struct.pack("<H", zlib.crc32(bytes(hdr)) & 0xFFFF)
    stream = bytes(hdr) + bytes(body) + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)
    assert gzip.decompress(stream) == data
    return stream


def cases(enc):
    """[(name, context, entry, stream, container, dst_n, options)]; entry: decode / recover (device buffers), decode_host /
    recover_host.  options: caller (a caller's stream instead of NULL), depends (recover: False passes NULL), cap (decode_host)"""
    out = []

    def both(name, stream, container, n, ctx="default", **opt):
        out.append((name + "/decode", ctx, "decode", stream, container, n, opt))
        out.append((name + "/recover", ctx, "recover", stream, container, n, opt))

    # geometry: one segment takes no scan, two are the first that do; M nodes, H nodes, the label-2 edge (noisehead)
    datas = [(kind, n, _data(kind, n, 3 * j + 1)) for j, n in enumerate(SIZES) for kind in KINDS]
    geo = {}
    for cont in KIND:
        streams = enc.compress_batch([d for _, _, d in datas], container=cont)
        for (kind, n, d), s in zip(datas, streams):
            geo[kind, n, cont] = (s, d)
            assert zlib_says(s, n, cont) == d.tobytes()  # (what test_every_success_returns_its_input compares with)
            both(f"geometry/{kind}/{n}/{cont}", s, cont, n)
    for n in SIZES:  # the serial token kernel
        both(f"serial/text/{n}/zlib", geo["text", n, "zlib"][0], "zlib", n, ctx="serial")
    seven = 7 * SEG - 5
    for cont in KIND:  # a launch-batch cap below the item: it runs alone and whole
        both(f"cap2/text/{seven}/{cont}", geo["text", seven, cont][0], cont, seven, ctx="cap2")

    # the last scan wave of the item holds nothing, or one byte, in front of the sentinel
    d = _data("text", 2 * SEG + 100, 41)
    body = enc.compress(d)
    for rem in (0, 1):
        pad = (rem - (10 + 1 + len(body) + 8)) % 8192
        s = _gzip_around(body, d.tobytes(), 0x08, b"a" * pad)
        assert len(s) % 8192 == rem and nseg_of(d.size) >= 2
        both(f"lastwave/{rem}", s, "gzip", d.size)
        out.append((f"lastwave/{rem}/trailer", "default", "decode", s, "gzip", TRAILER, {}))

    # stored payloads full of flush markers and fake stored headers; streams whose markers fall badly for 4-byte scanning
    rng = np.random.default_rng(11)
    bad = rng.integers(0, 256, 3 * SEG + 77, dtype=np.uint8)
    for off in range(123, bad.size - 8, 300):
        bad[off:off + 4] = (0, 0, 0xFF, 0xFF)
    for off in range(250, bad.size - 8, 700):
        bad[off:off + 5] = (rng.integers(0, 2), 0, 0x80, 0xFF, 0x7F)
    both("adversarial/stored", enc.compress(bad, strategy="stored"), "raw", bad.size)
    both("adversarial/auto", enc.compress(bad), "raw", bad.size)
    d0, s0 = _stream_of_length_0_mod_4(enc, final_stream=False)
    both("marker/0mod4", s0, "raw", d0.size)
    d2, s2, front = _stream_with_a_marker_at_2_mod_4(enc)
    both("marker/2mod4/front", front, "raw", d2.size)
    both("marker/2mod4/tail", s2[len(front):], "raw", d2.size)

    # wrappers
    d = _data("text", 5 * SEG + 17, 9)
    body = W.zlib_flushed(d.tobytes(), 6, zlib.Z_FULL_FLUSH, -15, True)
    for flags in (0x08, 0x04 | 0x08 | 0x10, 0x02 | 0x10):
        s = _gzip_around(body, d.tobytes(), flags)
        out.append((f"wrapper/flags{flags:02x}/trailer", "default", "decode", s, "gzip", TRAILER, {}))
        both(f"wrapper/flags{flags:02x}/explicit", s, "gzip", d.size)
    gz = _gzip_around(body, d.tobytes())
    both("wrapper/below_isize", gz, "gzip", d.size - 1)
    both("wrapper/above_isize", gz, "gzip", d.size + 1)
    out.append(("wrapper/bad_crc/trailer", "default", "decode", gz[:-8] + struct.pack("<II", zlib.crc32(d.tobytes()) ^ 1, d.size),
                "gzip", TRAILER, {}))
    zs, zd = geo["text", 65537, "zlib"]
    both("wrapper/bad_adler", zs[:-1] + bytes([zs[-1] ^ 0x40]), "zlib", zd.size)
    both("wrapper/no_parse/gzip", b"\x1f\x8c" + gz[2:], "gzip", d.size)
    out.append(("wrapper/no_parse/gzip/trailer", "default", "decode", b"\x1f\x8c" + gz[2:], "gzip", TRAILER, {}))
    both("wrapper/no_parse/zlib", b"\x79" + zs[1:], "zlib", zd.size)
    both("wrapper/cut_trailer/gzip", gz[:-3], "gzip", d.size)  # (explicit sizes only: a cut trailer's ISIZE is any number)
    both("wrapper/cut_trailer/zlib", zs[:-2], "zlib", zd.size)

    # not indexable; damage
    d = _data("text", 2 * SEG + 5, 20)
    both("unflushed/zlib", zlib.compress(d.tobytes(), 6), "zlib", d.size)
    s = bytearray(enc.compress(d, container="zlib", block_bytes=SEG))
    ix = enc.last_index()
    s[(int(ix[1]) + int(ix[2])) // 2] ^= 0x5A
    both("damage/flip_seg1", bytes(s), "zlib", d.size)

    # depends: no dependent segment; dependent segments inside strips.  With the flags and without
    d = geo["text", seven, "raw"][1]
    for bb in (SEG, 4 * SEG):
        s = enc.compress(d, block_bytes=bb)
        out.append((f"depends/{bb}/given", "default", "recover", s, "raw", seven, {}))
        out.append((f"depends/{bb}/null", "default", "recover", s, "raw", seven, {"depends": False}))
        out.append((f"depends/{bb}/decode", "default", "decode", s, "raw", seven, {}))

    # a caller's stream (every other case passes NULL: the context's own)
    both("stream/caller", geo["text", seven, "zlib"][0], "zlib", seven, caller=True)
    both("stream/null", geo["text", seven, "zlib"][0], "zlib", seven)

    # host buffers
    for kind, n, cont, want in (("text", 65537, "zlib", 65537), ("noise", 32769, "raw", 32769), ("noisehead", seven, "gzip", TRAILER)):
        s = geo[kind, n, cont][0]
        out.append((f"host/{kind}/{n}/{cont}/decode", "default", "decode_host", s, cont, want, {}))
        out.append((f"host/{kind}/{n}/{cont}/small", "default", "decode_host", s, cont, want, {"cap": n - 1}))
        out.append((f"host/{kind}/{n}/{cont}/recover", "default", "recover_host", s, cont, n, {}))
        out.append((f"host/{kind}/{n}/{cont}/recover_null", "default", "recover_host", s, cont, n, {"depends": False}))
    return out


def _counts(c, r):
    r["scratch_bytes"] = c.last_decode_scratch_bytes()
    if r["rc"] == 0 and r.get("status", 0) == 0:  # (after a failed wrapper the counts are the call's before)
        st = c.last_recover_stats()
        r["nodes"], r["rows"] = int(st["nodes"]), int(st["rows"])
    if r["rc"] or r.get("status", 0):
        r["error"] = c.last_error()
    return r


def _size(stream, dst_n):
    return dst_n if dst_n != TRAILER else (int.from_bytes(stream[-4:], "little") if len(stream) >= 18 else 0)


def _up(stream):
    return torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda() if stream else torch.zeros(4, dtype=torch.uint8, device="cuda")


def run_case(c, entry, stream, container, dst_n, opt):
    """-> (the record's fields, the decoded bytes or None)"""
    lib, h, kind = c._lib, c._h, KIND[container]
    size = _size(stream, dst_n)
    hs = torch.cuda.Stream() if opt.get("caller") else None
    sp = C.c_void_p(hs.cuda_stream if hs else None)
    if entry == "decode":
        src = _up(stream)
        dst = torch.full((size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        st = C.c_uint32(0)
        torch.cuda.synchronize()
        rc = lib.sfh_decompress_any_device(h, src.data_ptr(), len(stream), kind, dst.data_ptr() if size else None, dst_n, C.byref(st), sp)
        got = dst.cpu().numpy()  # (the call has synchronised its stream)
        torch.cuda.synchronize()
        assert (got[size:] == FILL).all(), "a byte behind the destination was written"
        r = {"rc": rc, "status": st.value}
        if rc or st.value:
            r["dst_untouched"] = bool((got == FILL).all())
        else:
            r["out_sha256"] = sha(got[:size].tobytes())
        return _counts(c, r), got[:size].tobytes()
    if entry == "recover":
        src = _up(stream)
        nseg = nseg_of(size)
        index = torch.full((nseg + 1,), -1, dtype=torch.int64, device="cuda")
        dep = torch.full((nseg + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = lib.sfh_recover_index_device(h, src.data_ptr(), len(stream), kind, dst_n, index.data_ptr(), nseg,
                                          dep.data_ptr() if opt.get("depends", True) else None, sp)
        ix, dp = index.cpu().numpy(), dep.cpu().numpy()
        torch.cuda.synchronize()
        assert (dp[nseg:] == FILL).all(), "a byte behind the depends flags was written"
        r = {"rc": rc}
        if rc == 0:
            r["index_sha256"], r["depends_sha256"] = sha(ix.tobytes()), sha(dp[:nseg].tobytes())
        return _counts(c, r), None
    buf = np.frombuffer(stream, np.uint8)
    if entry == "decode_host":
        cap = opt.get("cap", size)
        dst = np.full(cap + GUARD, FILL, np.uint8)
        st, n_out = C.c_uint32(0), C.c_uint64(0)
        rc = lib.sfh_decompress_any(h, buf.ctypes.data, buf.size, kind, dst.ctypes.data, cap, dst_n, C.byref(n_out), C.byref(st))
        assert (dst[cap:] == FILL).all(), "a byte behind the destination was written"
        r = {"rc": rc, "status": st.value, "dst_n_out": n_out.value}
        if rc or st.value:
            r["dst_untouched"] = bool((dst == FILL).all())
        else:
            r["out_sha256"] = sha(dst[:size].tobytes())
        return _counts(c, r), dst[:size].tobytes()
    assert entry == "recover_host"
    nseg = nseg_of(size)
    index = np.full(nseg + 1, 77, np.uint64)
    dep = np.full(nseg + GUARD, FILL, np.uint8)
    rc = lib.sfh_recover_index(h, buf.ctypes.data, buf.size, kind, dst_n, index.ctypes.data, nseg,
                               dep.ctypes.data if opt.get("depends", True) else None)
    assert (dep[nseg:] == FILL).all(), "a byte behind the depends flags was written"
    r = {"rc": rc}
    if rc == 0:
        r["index_sha256"], r["depends_sha256"] = sha(index.tobytes()), sha(dep[:nseg].tobytes())
    return _counts(c, r), None
