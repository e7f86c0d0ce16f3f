"""Seekable gzip on the GPU (SFH_DICTZIP, sfh_dz_read_index*, sfh_decompress_dz*): the compressor writes an ordinary gzip file
whose header carries dictzip's table of chunk sizes, every gzip reader inflates it, every chunk inflates alone from its
table offset, and the library reads the file and byte ranges of it given nothing but its bytes -- its own files and those of a
dictzip writer in Python alike."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest
import torch

import dictzip_files as DZ
import starflate_amd
from range_cases import edge_ranges
from starflate_amd import Compressor, StarflateError, _capi, synth

pytestmark = pytest.mark.gpu

SEG = 32768
SIZES = (0, 1, 32768, 32769, 3 * 32768 + 5, 2 << 20)
KINDS = ("text", "random", "zeros")
DICTZIP = 3


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


def _content(kind, n):
    if kind == "text":
        return synth.gen_text(n, seed=n % 97 + 1) if n else np.zeros(0, np.uint8)
    if kind == "random":
        return np.random.default_rng(n + 3).integers(0, 256, n, dtype=np.uint8)
    return np.zeros(n, np.uint8)


def _compress_async(comp, data, container):
    src = torch.from_numpy(data.copy()).cuda() if data.size else torch.empty(0, dtype=torch.uint8, device="cuda")
    out = torch.zeros(_capi.lib().sfh_compress_bound_container(data.size, SEG, DICTZIP), dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int64, device="cuda")
    comp.compress_tensor_async(src, out, size, container=container, block_bytes=SEG)
    torch.cuda.synchronize()
    return out[: int(size.item())].cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def made(comp):
    """{(kind, n, path): (data bytes, file bytes, the compressor's own index)} -- every shape through sfh_compress ("host") and
    through sfh_compress_device_async ("async"), each compressed once for all tests"""
    out = {}
    for kind in KINDS:
        for n in SIZES:
            data = _content(kind, n)
            blob = comp.compress(data, container="dictzip")
            out[kind, n, "host"] = (data.tobytes(), blob, comp.last_index().copy())
            assert comp.last_block_bytes() == SEG
            blob = _compress_async(comp, data, "dictzip")
            out[kind, n, "async"] = (data.tobytes(), blob, comp.last_index().copy())
    return out


def _parse(blob):
    """the format of include/starflate_hip.h, read with struct -> (header bytes, sizes)"""
    assert blob[:10] == bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF])
    xlen, si, ln, ver, chlen, chcnt = struct.unpack("<H2sHHHH", blob[10:22])
    assert si == b"RA" and ver == 1 and chlen == SEG and xlen == 10 + 2 * chcnt and ln == 6 + 2 * chcnt
    return 22 + 2 * chcnt, struct.unpack(f"<{chcnt}H", blob[22: 22 + 2 * chcnt])


def test_writer(comp, made):
    assert len(made) == 36
    gz = {}
    for (kind, n, path), (data, blob, index) in made.items():
        key = (kind, n, path)
        assert zlib.decompress(blob, wbits=31) == data, key
        hdr, sizes = _parse(blob)
        nseg = max(1, -(-n // SEG))
        assert len(sizes) == nseg and hdr == 22 + 2 * nseg == _capi.lib().sfh_dz_header_bytes(n), key
        # sfh_copy_index equals the table's prefix sums; the last size reaches to the trailer
        assert [int(v) for v in index] == [hdr + sum(sizes[:k]) for k in range(nseg + 1)], key
        assert int(index[-1]) == len(blob) - 8, key
        if kind == "random" and n >= SEG:
            assert max(sizes) >= 32773, key  # stored segments: the largest sizes the table sees
        # every chunk inflated alone, by a fresh decoder, from its table offset: the dictzip contract
        for k in range(nseg) if n <= 4 * SEG else (0, 1, nseg // 2, nseg - 1):
            d = zlib.decompressobj(-15)
            assert d.decompress(blob[int(index[k]): int(index[k + 1])]) == data[k * SEG: (k + 1) * SEG], (key, k)
        # from the header's end on: the SFH_GZIP stream at block_bytes = 32768, from its byte 10 on
        if (kind, n) not in gz:
            gz[kind, n] = comp.compress(np.frombuffer(data, np.uint8), container="gzip", block_bytes=SEG)
        assert blob[hdr:] == gz[kind, n][10:], key
        assert blob[4:10] == gz[kind, n][4:10], key


def _device_index(comp, blob):
    """sfh_dz_read_index_device on the file in device memory -> (index, total_n)"""
    stream = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    index = torch.full((_capi.DZ_MAX_CHUNKS + 1,), -1, dtype=torch.int64, device="cuda")
    info = _capi.DzInfo()
    rc = _capi.lib().sfh_dz_read_index_device(comp._h, stream.data_ptr(), stream.numel(), C.byref(info), index.data_ptr(), index.numel(), None)
    assert rc == 0 and info.status == 0, (rc, info.status)
    got = index.cpu().numpy()
    assert (got[info.nseg + 1:] == -1).all()
    return [int(v) for v in got[: info.nseg + 1]], int(info.total_n)


def _device_decode(comp, blob, cap):
    """sfh_decompress_dz_device on the file in device memory -> (bytes, status)"""
    stream = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    out = torch.full((max(cap, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    got, st = C.c_uint64(0), C.c_uint32(9)
    rc = _capi.lib().sfh_decompress_dz_device(comp._h, stream.data_ptr(), stream.numel(), out.data_ptr(), cap, C.byref(got), C.byref(st), None)
    assert rc == 0, comp.last_error()
    return out[: got.value].cpu().numpy().tobytes(), int(st.value)


def test_reader_index(comp, made):
    for key, (data, blob, index) in made.items():
        host, total_n = starflate_amd.dictzip_index(blob)
        assert total_n == len(data) and [int(v) for v in host] == [int(v) for v in index], key
        assert _device_index(comp, blob) == ([int(v) for v in index], len(data)), key
    # files of a dictzip writer in Python: every variant of the header, the final block outside the table among them
    for name, (data, blob, want) in DZ.good_files(levels=(6,), sizes=(0, 1, 32768, 32769, 3 * 32768 + 5)).items():
        assert _device_index(comp, blob) == (want, len(data)), name
    name, (data, blob, want) = "level 0", DZ.good_files(levels=(0,), sizes=(3 * 32768 + 5,))["98309-outside-l0"]
    assert _device_index(comp, blob) == (want, len(data)), name


def test_reader_index_refusals_on_the_device(comp):
    lib = _capi.lib()
    data = DZ.text(70000, seed=4)
    blob, want = DZ.write(data, final="outside")
    stream = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    info = _capi.DzInfo(1, 2, 3, 4, 5)
    idx = torch.full((8,), 7, dtype=torch.int64, device="cuda")
    # index_cap one short: SFH_E_DST_TOO_SMALL, nothing written
    assert lib.sfh_dz_read_index_device(comp._h, stream.data_ptr(), stream.numel(), C.byref(info), idx.data_ptr(), 3, None) == -2
    assert (idx.cpu() == 7).all() and info.total_n == 1
    assert lib.sfh_dz_read_index_device(comp._h, stream.data_ptr(), stream.numel(), C.byref(info), idx.data_ptr(), 4, None) == 0
    assert idx.cpu().tolist() == want + [7] * 4 and (info.total_n, info.nseg, info.header_bytes, info.status, info.reserved) == (70000, 3, want[0], 0, 0)
    # a header that does not parse: the status, the index untouched -- the sizes reaching past the trailer (known only after
    # the sum), a bad magic, a stream of 17 bytes
    for bad, st in ((blob[:22] + b"\xff\xff" + blob[24:], 1), (b"\x1e" + blob[1:], 1), (blob[:17], 5)):
        s = torch.from_numpy(np.frombuffer(bad, np.uint8).copy()).cuda()
        idx.fill_(7)
        assert lib.sfh_dz_read_index_device(comp._h, s.data_ptr(), s.numel(), C.byref(info), idx.data_ptr(), 8, None) == 0
        assert (info.total_n, info.nseg, info.header_bytes, info.status) == (0, 0, 0, st) and (idx.cpu() == 7).all()


def test_reader_decode(comp, made):
    for key, (data, blob, _) in made.items():
        out, st = comp.decompress_dictzip(blob)
        assert st == 0 and out == data, key
        assert _device_decode(comp, blob, len(data)) == (data, 0), key
    assert starflate_amd.decompress_dictzip(made["text", 3 * 32768 + 5, "host"][1]) == made["text", 3 * 32768 + 5, "host"][0]
    # the files of the Python writer, the final block inside and outside the last chunk's size, stored and coded
    files = DZ.good_files(levels=(0, 6), sizes=(0, 1, 32768, 3 * 32768 + 5))
    for name in [k for k in files if k.split("-")[1] in ("inside", "outside", "all", "chcnt0")]:
        data, blob, _ = files[name]
        out, st = comp.decompress_dictzip(blob)
        assert st == 0 and out == data, name


def test_reader_detects_damage(comp, made):
    data, blob, index = made["text", 3 * 32768 + 5, "host"]
    at = (int(index[1]) + int(index[2])) // 2  # a byte in the middle of the second chunk
    bad = blob[:at] + bytes([blob[at] ^ 0x10]) + blob[at + 1:]
    out, st = comp.decompress_dictzip(bad)
    assert st != 0 and out == b""
    bad = blob[:-8] + bytes([blob[-8] ^ 1]) + blob[-7:]  # one CRC byte
    assert comp.decompress_dictzip(bad) == (b"", 1)
    dst = np.full(len(data), 0xA5, np.uint8)
    n64, st = C.c_uint64(9), C.c_uint32(9)
    src = np.frombuffer(bad, np.uint8)
    assert _capi.lib().sfh_decompress_dz(comp._h, src.ctypes.data, src.size, dst.ctypes.data, dst.size, C.byref(n64), C.byref(st)) == 0
    assert st.value == 1 and n64.value == 0 and (dst == 0xA5).all()  # dst is written only on status 0
    # ISIZE above the capacity: SFH_E_DST_TOO_SMALL
    src = np.frombuffer(blob, np.uint8)
    assert _capi.lib().sfh_decompress_dz(comp._h, src.ctypes.data, src.size, dst.ctypes.data, dst.size - 1, C.byref(n64), C.byref(st)) == -2


def _check_ranges(comp, data, blob, what):
    ranges = edge_ranges(len(data), SEG)
    offs, lens = [r[0] for r in ranges], [r[1] for r in ranges]
    outs, st = comp.read_ranges(blob, offs, lens)
    assert (st == 0).all(), what
    for (o, m), got in zip(ranges, outs):
        assert got == data[o: o + m], (what, o, m)
    # the C call itself, the destinations packed back to back in one pre-filled buffer
    k = len(ranges)
    pos = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.int64)
    buf = np.full(int(pos[-1]) + 5, 0xA5, np.uint8)
    src = np.frombuffer(blob, np.uint8)
    sts = np.full(k, 9, np.uint32)
    rc = _capi.lib().sfh_decompress_dz_ranges(comp._h, src.ctypes.data, src.size, k, (C.c_uint64 * k)(*offs), (C.c_uint64 * k)(*lens),
                                              (C.c_void_p * k)(*[buf.ctypes.data + int(p) for p in pos[:-1]]), sts.ctypes.data)
    assert rc == 0 and (sts == 0).all(), what
    want = np.concatenate([np.full(3, 0xA5, np.uint8)] + [np.frombuffer(data[o: o + m], np.uint8) for o, m in ranges] + [np.full(5, 0xA5, np.uint8)])
    assert np.array_equal(buf, want), what


def test_ranges(comp, made):
    for key in (("text", 3 * 32768 + 5, "host"), ("random", 32769, "async"), ("zeros", 32768, "host"), ("text", 1, "async")):
        data, blob, _ = made[key]
        _check_ranges(comp, data, blob, key)
    data, blob, _ = made["text", 0, "host"]
    outs, st = starflate_amd.read_ranges(blob, [0], [0])
    assert outs == [b""] and (st == 0).all()
    # a few ranges of the 2 MiB file: first and last byte, across a segment edge
    data, blob, _ = made["text", 2 << 20, "host"]
    offs, lens = [0, len(data) - 1, 17 * SEG - 3, 5], [1, 1, 7, 0]
    outs, st = starflate_amd.read_ranges(blob, offs, lens)
    assert (st == 0).all() and outs == [data[o: o + m] for o, m in zip(offs, lens)]
    # a host-made level-6 file, the final block outside the table as dictzip(1) leaves it
    data = DZ.text(3 * 32768 + 5, seed=11)
    blob, _ = DZ.write(data, level=6, final="outside", fname=b"words")
    _check_ranges(comp, data, blob, "python writer")


def test_ranges_of_a_damaged_file(comp, made):
    data, blob, index = made["text", 3 * 32768 + 5, "host"]
    at = (int(index[1]) + int(index[2])) // 2
    bad = blob[:at] + bytes([blob[at] ^ 0x10]) + blob[at + 1:]
    outs, st = comp.read_ranges(bad, [0, SEG + 5, 3 * SEG], [10, 10, 5])
    assert st[0] == 0 and st[2] == 0 and outs[0] == data[:10] and outs[2] == data[3 * SEG:]  # damage stays in its chunk
    assert outs[1] is None or outs[1] == data[SEG + 5: SEG + 15]  # (a flipped bit may also decode to the same bytes up to there)
    # a header that does not parse: every range gets its status
    outs, st = None, np.full(2, 9, np.uint32)
    src = np.frombuffer(blob[:22] + b"\xff\xff" + blob[24:], np.uint8)
    dst = np.full(8, 0xA5, np.uint8)
    rc = _capi.lib().sfh_decompress_dz_ranges(comp._h, src.ctypes.data, src.size, 2, (C.c_uint64 * 2)(0, 1), (C.c_uint64 * 2)(1, 1),
                                              (C.c_void_p * 2)(dst.ctypes.data, dst.ctypes.data + 4), st.ctypes.data)
    assert rc == 0 and st.tolist() == [1, 1] and (dst == 0xA5).all()


def test_refusals_on_the_device(comp):
    lib = _capi.lib()
    n = 3 * SEG + 5
    data = synth.gen_text(n, seed=5)
    bound = lib.sfh_compress_bound_container(n, 0, DICTZIP)
    assert bound == lib.sfh_compress_bound(n, 0) + 12 + 2 * 4
    dst = np.full(bound, 0xA5, np.uint8)
    out_n = C.c_size_t(7)
    src = torch.from_numpy(data.copy()).cuda()
    d_dst = torch.full((bound,), 0xA5, dtype=torch.uint8, device="cuda")
    d_n = torch.full((1,), 7, dtype=torch.int64, device="cuda")

    def calls(opt, cap):
        return (lib.sfh_compress(comp._h, data.ctypes.data, n, dst.ctypes.data, cap, C.byref(out_n), C.byref(opt)),
                lib.sfh_compress_device(comp._h, src.data_ptr(), n, d_dst.data_ptr(), cap, C.byref(out_n), C.byref(opt), None),
                lib.sfh_compress_device_async(comp._h, src.data_ptr(), n, d_dst.data_ptr(), cap, d_n.data_ptr(), C.byref(opt), None))

    assert calls(_capi.make_options(container="dictzip", block_bytes=65536), bound) == (-1, -1, -1)
    assert calls(_capi.make_options(container="dictzip", final_stream=False), bound) == (-1, -1, -1)
    assert calls(_capi.make_options(container="dictzip"), bound - 1) == (-2, -2, -2)
    # ... all of it before anything is enqueued: nothing was written
    torch.cuda.synchronize()
    assert (dst == 0xA5).all() and (d_dst.cpu() == 0xA5).all() and int(d_n.item()) == 7 and out_n.value == 7
    # block_bytes = 32768 given explicitly is the same file as 0
    assert comp.compress(data, container="dictzip", block_bytes=SEG) == comp.compress(data, container="dictzip")
    # the batched call refuses the container
    opt = _capi.make_options(container="dictzip")
    sp, dp = (C.c_void_p * 1)(data.ctypes.data), (C.c_void_p * 1)(dst.ctypes.data)
    one_n, one_cap, got = (C.c_uint64 * 1)(n), (C.c_uint64 * 1)(bound), (C.c_uint64 * 1)(7)
    assert lib.sfh_compress_batch(comp._h, 1, sp, one_n, dp, one_cap, got, C.byref(opt)) == -1
    dsp, ddp = (C.c_void_p * 1)(src.data_ptr()), (C.c_void_p * 1)(d_dst.data_ptr())
    assert lib.sfh_compress_batch_device_async(comp._h, 1, dsp, one_n, ddp, one_cap, d_n.data_ptr(), C.byref(opt), None) == -1
    ctxs = (C.c_void_p * 1)(comp._h)
    assert lib.sfh_compress_multi(ctxs, 1, data.ctypes.data, n, dst.ctypes.data, bound, C.byref(out_n), C.byref(opt)) == -1
    assert (dst == 0xA5).all() and got[0] == 7
    # ... and so do the decoders' container arguments: to them the file is an SFH_GZIP stream
    blob = np.frombuffer(comp.compress(data, container="dictzip"), np.uint8)
    back = np.zeros(n, np.uint8)
    st, n64 = (C.c_uint32 * 1)(9), (C.c_uint64 * 1)(0)
    bp, op, bn, on = (C.c_void_p * 1)(blob.ctypes.data), (C.c_void_p * 1)(back.ctypes.data), (C.c_uint64 * 1)(blob.size), (C.c_uint64 * 1)(n)
    assert lib.sfh_inflate_stream_batch(comp._h, 1, bp, bn, DICTZIP, op, on, n64, st) == -1
    assert lib.sfh_decompress_any_batch(comp._h, 1, bp, bn, DICTZIP, op, on, on, n64, st) == -1
    assert lib.sfh_decompress_any_batch(comp._h, 1, bp, bn, 2, op, on, on, n64, st) == 0 and st[0] == 0 and back.tobytes() == data.tobytes()


def test_dictzip_default_chunk_length_goes_to_the_stream_decoder(comp):
    data = DZ.text(150000, seed=8)
    blob, _ = DZ.write(data, chlen=58315, final="outside")
    assert zlib.decompress(blob, wbits=31) == data
    src = np.frombuffer(blob, np.uint8)
    dst = np.full(len(data), 0xA5, np.uint8)
    n64, st = C.c_uint64(9), C.c_uint32(9)
    assert _capi.lib().sfh_decompress_dz(comp._h, src.ctypes.data, src.size, dst.ctypes.data, dst.size, C.byref(n64), C.byref(st)) == -8
    assert (dst == 0xA5).all() and (n64.value, st.value) == (9, 9)
    stream = torch.from_numpy(src.copy()).cuda()
    d_dst = torch.full((len(data),), 0xA5, dtype=torch.uint8, device="cuda")
    assert _capi.lib().sfh_decompress_dz_device(comp._h, stream.data_ptr(), stream.numel(), d_dst.data_ptr(), d_dst.numel(),
                                                C.byref(n64), C.byref(st), None) == -8
    assert (d_dst.cpu() == 0xA5).all()
    sts = np.full(1, 9, np.uint32)
    assert _capi.lib().sfh_decompress_dz_ranges(comp._h, src.ctypes.data, src.size, 1, (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(4),
                                                (C.c_void_p * 1)(dst.ctypes.data), sts.ctypes.data) == -8
    assert (dst == 0xA5).all() and sts[0] == 9
    with pytest.raises(StarflateError) as e:
        comp.decompress_dictzip(blob)
    assert e.value.code == -8
    with pytest.raises(StarflateError) as e:
        starflate_amd.read_ranges(blob, [0], [4])
    assert e.value.code == -8
    assert starflate_amd.decompress_dictzip(blob) == data  # ... through decompress_stream(container="gzip")
