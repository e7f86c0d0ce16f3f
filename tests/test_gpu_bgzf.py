"""BGZF on the GPU (sfh_compress_bgzf*, sfh_bgzf_read_index_device, sfh_decompress_bgzf*).  The writer's file must be, slice
by slice of 32768 input bytes, the 18-byte BGZF header, then bytes [10:] of what compress_batch(slices, container="gzip") writes
for that slice alone with BSIZE to match, and the EOF member behind the last; gzip.decompress and a pure-Python BGZF walker
(tests/bgzf_files.py) must read it.  The reader must find the members of its own files and of Python-made ones exactly as
that walker does -- fake member headers inside stored data included -- decode them to what gzip.decompress gives, and end
every damaged file in a status."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import bgzf_files as BZ
import starflate_amd
from conftest import ROOT
from starflate_amd import Compressor, StarflateError, _capi, synth

pytestmark = pytest.mark.gpu

SEG = 32768
SIZES = (0, 1, 32767, 32768, 32769, 3 * 32768 + 5, 40 * 32768 + 7)
KINDS = ("text", "zeros", "random")
OPTIONS = {"default": {}, "chain": {"effort": "best"}, "fixed": {"strategy": "fixed"}}
NOT_INDEXABLE, DST_TOO_SMALL, INVALID_ARG = -8, -2, -1


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


def _cuda(data):
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda() if len(data) else torch.empty(0, dtype=torch.uint8, device="cuda")


def expected_file(comp, data, **options):
    """the defining property: header | compress_batch's member from byte 10 on, for every slice; then the EOF member"""
    data = data.tobytes()
    slices = [data[k: k + SEG] for k in range(0, len(data), SEG)]
    members = comp.compress_batch(slices, container="gzip", **options) if slices else []
    out = b""
    for m in members:
        out += BZ.EOF[:16] + struct.pack("<H", 18 + len(m) - 10 - 1) + m[10:]
    return out + BZ.EOF


@pytest.fixture(scope="module")
def made(comp):
    """{(kind, n, options): (data, file)}: every shape through sfh_compress_bgzf_device, each compressed once for all tests;
    the default options for every kind, a chain effort and forced fixed blocks on text"""
    out = {}
    for kind in KINDS:
        for n in SIZES:
            data = _content(kind, n)
            for name, options in OPTIONS.items():
                if name != "default" and kind != "text":
                    continue
                buf, size = comp.compress_bgzf_tensor(_cuda(data), **options)
                with pytest.raises(StarflateError):
                    comp.last_index()  # no block index after a BGZF call
                out[kind, n, name] = (data, buf[:size].cpu().numpy().tobytes())
    return out


def test_writer_is_the_gzip_members_with_bgzf_headers(comp, made):
    assert len(made) == 7 * 5
    for (kind, n, name), (data, blob) in made.items():
        key = (kind, n, name)
        assert blob == expected_file(comp, data, **OPTIONS[name]), key
        assert gzip.decompress(blob) == data.tobytes(), key
        moff, ooff, widest, eof = BZ.walk(blob)  # every BSIZE leads to the next member, the last one is the EOF member
        assert eof and len(moff) - 1 == -(-n // SEG) + 1 and ooff[-1] == n and widest == min(n, SEG), key
        assert len(blob) <= comp.bgzf_bound(n), key
        if kind == "random" and n >= SEG:
            assert moff[1] - moff[0] == SEG + 5 + 26, key  # a stored member
    assert made["text", 0, "default"][1] == BZ.EOF


def test_host_buffers_write_the_same_file(comp, made):
    for kind, n in (("text", 0), ("text", 1), ("random", 32769), ("text", 3 * 32768 + 5), ("zeros", 40 * 32768 + 7)):
        data, blob = made[kind, n, "default"]
        assert comp.compress_bgzf(data) == blob, (kind, n)
    assert starflate_amd.compress_bgzf(made["text", 32769, "chain"][0], effort="best") == made["text", 32769, "chain"][1]


def test_index_method_is_the_module_function(comp, made):
    """Compressor.bgzf_index: the host walk of starflate_amd.bgzf_index, on the smallest files"""
    for n in (0, 1, 32769):
        blob = made["text", n, "default"][1]
        (gm, go, ginfo), (wm, wo, winfo) = comp.bgzf_index(blob), starflate_amd.bgzf_index(blob)
        assert np.array_equal(gm, wm) and np.array_equal(go, wo) and ginfo == winfo, n
        moff, ooff, widest, eof = BZ.walk(blob)
        assert list(gm) == list(moff) and list(go) == list(ooff), n
        assert ginfo == {"total_n": n, "members": len(moff) - 1, "max_isize": widest, "has_eof": bool(eof)}, n


def test_async_call_on_a_callers_stream(comp, made):
    data, blob = made["text", 3 * 32768 + 5, "default"]
    stream = torch.cuda.Stream()
    src = _cuda(data)
    out = torch.zeros(comp.bgzf_bound(data.size), dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    comp.compress_bgzf_tensor_async(src, out, size, stream=stream.cuda_stream)
    stream.synchronize()
    assert out[: int(size.item())].cpu().numpy().tobytes() == blob


def test_carry_across_launch_batches(made):
    """SFH_BATCH_CHUNKS=2 in a fresh process: five members in three launch batches, the same file"""
    n = 4 * 32768 + 77
    code = ("import sys, numpy as np, torch\n"
            "from starflate_amd import Compressor, synth\n"
            f"data = synth.gen_text({n}, seed=11)\n"
            "c = Compressor(0)\n"
            "buf, size = c.compress_bgzf_tensor(torch.from_numpy(data).cuda())\n"
            "sys.stdout.buffer.write(buf[:size].cpu().numpy().tobytes())\n")
    env = dict(os.environ, SFH_BATCH_CHUNKS="2", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    c = Compressor(0)
    try:
        data = synth.gen_text(n, seed=11)
        want = expected_file(c, data)
        assert out.stdout == want and len(BZ.walk(want)[0]) - 1 == 6
        assert c.compress_bgzf(data) == want
    finally:
        c.close()


def test_writer_refusals(comp):
    src = _cuda(_content("text", 1000))
    L = _capi.lib()
    for options in ({"container": "gzip"}, {"container": "zlib"}, {"final_stream": False}, {"block_bytes": 65536}):
        with pytest.raises(StarflateError) as e:
            comp.compress_bgzf_tensor(src, **options)
        assert e.value.code == INVALID_ARG, options
    comp.compress_bgzf_tensor(src, block_bytes=SEG)  # 32768 is what 0 means
    short = torch.zeros(L.sfh_bgzf_bound(1000) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(StarflateError) as e:
        comp.compress_bgzf_tensor(src, out=short)
    assert e.value.code == DST_TOO_SMALL


# ---- the reader ----
def _device_index(comp, blob):
    moff, ooff, info = comp.bgzf_index_tensor(_cuda(blob))
    return [int(v) for v in moff.cpu()], [int(v) for v in ooff.cpu()], info


def _device_decode(comp, blob, cap=None, total=None):
    """sfh_decompress_bgzf_device -> (bytes written, status)"""
    total = len(gzip.decompress(blob)) if total is None else total
    cap = total if cap is None else cap
    out = torch.full((max(total, 16),), 0xA5, dtype=torch.uint8, device="cuda")
    got, st = C.c_uint64(0), C.c_uint32(9)
    src = _cuda(blob)
    rc = _capi.lib().sfh_decompress_bgzf_device(comp._h, src.data_ptr() if len(blob) else None, len(blob), out.data_ptr(), cap, C.byref(got),
                                                C.byref(st), None)
    if rc:
        raise StarflateError(rc, comp.last_error())
    return out[: got.value].cpu().numpy().tobytes(), int(st.value)


@pytest.fixture(scope="module")
def python_files():
    return BZ.good_files()


def _check_reads(comp, blob, data, key):
    wm, wo, widest, eof = BZ.walk(blob)
    hm, ho, hinfo = starflate_amd.bgzf_index(blob)
    assert ([int(v) for v in hm], [int(v) for v in ho]) == (wm, wo), key
    want_info = {"total_n": len(data), "members": len(wm) - 1, "max_isize": widest, "has_eof": eof}
    assert hinfo == want_info, key
    if len(blob):
        assert _device_index(comp, blob) == (wm, wo, want_info), key  # the device walk equals the host's
    assert _device_decode(comp, blob) == (data, 0), key
    assert comp.decompress_bgzf(blob) == (data, 0), key


def test_reader_on_the_writers_files(comp, made):
    for key, (data, blob) in made.items():
        _check_reads(comp, blob, data.tobytes(), key)
    assert starflate_amd.decompress_bgzf(made["text", 32769, "default"][1]) == made["text", 32769, "default"][0].tobytes()
    assert comp.decompress_bgzf(b"") == (b"", 0) and _device_decode(comp, b"", total=0) == (b"", 0)


def test_reader_on_python_made_files(comp, python_files):
    """members of odd ISIZE (outputs off every alignment), empty members, foreign subfields, stored members, no EOF member,
    and fake member headers inside stored data: nodes nobody reaches"""
    seen = 0
    for name, (data, blob, moff, ooff, eof) in python_files.items():
        if "65280" in name:
            continue
        _check_reads(comp, blob, data, name)
        seen += 1
    assert seen >= 9
    assert _device_index(comp, python_files["no EOF member"][1])[2]["has_eof"] is False


def test_members_of_65280_bytes(comp, python_files):
    data, blob = python_files["65280-byte members"][:2]
    assert _device_index(comp, blob)[2]["max_isize"] == 65280
    with pytest.raises(StarflateError) as e:
        _device_decode(comp, blob)
    assert e.value.code == NOT_INDEXABLE
    assert comp.decompress_bgzf(blob) == (data, 0)  # the host-buffer call reads every BGZF file
    assert starflate_amd.decompress_bgzf(blob) == data
    # ... and ends a damaged one in a status
    at = len(blob) - 28 - 8
    assert comp.decompress_bgzf(BZ.patched(blob, at, bytes([blob[at] ^ 0x40])))[1] == 1


def test_damaged_members(comp, made):
    data, blob = made["text", 3 * 32768 + 5, "default"]
    data = data.tobytes()
    moff, ooff, _, _ = BZ.walk(blob)
    crc_at = lambda k: moff[k + 1] - 8  # noqa: E731
    flip = lambda b, at: BZ.patched(b, at, bytes([b[at] ^ 0x40]))  # noqa: E731
    for k in (0, 1, 3):
        bad = flip(blob, crc_at(k))
        assert _device_decode(comp, bad, total=len(data)) == (b"", 1), k
        assert f"member {k}:" in comp.last_error(), k
        assert comp.decompress_bgzf(bad) == (b"", 1), k
    # a later damaged member does not mask the first: member 1's CRC and member 2's body
    bad = flip(flip(blob, crc_at(1)), moff[2] + 40)
    assert _device_decode(comp, bad, total=len(data))[1] == 1 and "member 1:" in comp.last_error()
    # ISIZE raised by one (the last data member, 5 bytes): exactly what the batch decoder says of that member alone, without
    # an index and with that ISIZE as its size
    k = 3
    bad = BZ.patched(blob, moff[k + 1] - 4, struct.pack("<I", 6))
    alone = comp.decompress_batch([bad[moff[k]: moff[k + 1]]], [6], container="gzip")[1][0]
    assert alone != 0
    assert _device_decode(comp, bad, total=len(data) + 1) == (b"", alone) and "member 3:" in comp.last_error()
    assert comp.decompress_bgzf(bad) == (b"", alone)
    # a flipped body byte in a coded member
    assert _device_decode(comp, flip(blob, moff[2] + 40), total=len(data))[1] != 0 and "member 2:" in comp.last_error()


def test_truncated_and_refused(comp, made, python_files):
    data, blob = made["text", 3 * 32768 + 5, "default"]
    moff = BZ.walk(blob)[0]
    for cut, want in ((moff[2] + 7, 5), (moff[2] + 500, 5), (len(blob) - 1, 5)):
        with pytest.raises(StarflateError) as e:
            _device_index(comp, blob[:cut])
        assert e.value.code == want, cut
        assert _device_decode(comp, blob[:cut], total=data.size) == (b"", want), cut
        assert comp.decompress_bgzf(blob[:cut]) == (b"", want), cut
    for name, bad, want in BZ.damaged():
        assert _device_decode(comp, bad, total=40000) == (b"", want), name
    # the EOF member missing: no error
    assert _device_decode(comp, blob[:-28]) == (data.tobytes(), 0)
    assert _device_index(comp, blob[:-28])[2]["has_eof"] is False
    # dst_cap one short
    with pytest.raises(StarflateError) as e:
        _device_decode(comp, blob, cap=data.size - 1)
    assert e.value.code == DST_TOO_SMALL
    # the index arrays one entry short: refused, nothing written, the info says how many
    src = _cuda(blob)
    m = len(moff) - 1
    arrays = torch.full((2, m + 1), -1, dtype=torch.int64, device="cuda")
    info = _capi.BgzfInfo()
    rc = _capi.lib().sfh_bgzf_read_index_device(comp._h, src.data_ptr(), src.numel(), C.byref(info), arrays[0].data_ptr(), arrays[1].data_ptr(),
                                                m, None)
    assert rc == DST_TOO_SMALL and info.members == m and bool((arrays == -1).all())
    rc = _capi.lib().sfh_bgzf_read_index_device(comp._h, src.data_ptr(), src.numel(), C.byref(info), arrays[0].data_ptr(), arrays[1].data_ptr(),
                                                m + 1, None)
    assert rc == 0 and [int(v) for v in arrays[0].cpu()] == moff
