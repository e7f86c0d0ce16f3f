"""BGZF members above 32 KiB on the device (sfh_decompress_bgzf_wide_device; sfh_decompress_bgzf for host buffers): bgzip's and
htslib's 65280 bytes per member, the format's 65536.  Such a member is one segment of the indexed decoder's WIDE rows (65536
output bytes, 65536 tokens).  Everything here is made with Python's zlib (tests/bgzf_files.py) or by hand
(tests/bgzf_wide_cases.py over tests/deflate_writer.py); the expected bytes are gzip.decompress's.  Every good file goes through the new device call and
through Compressor.decompress_bgzf, and both must give the data and status 0."""
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
import bgzf_wide_cases as K
from conftest import ROOT
from starflate_amd import Compressor, StarflateError, _capi

pytestmark = pytest.mark.gpu

WIDE = K.WIDE
NOT_INDEXABLE, DST_TOO_SMALL, INVALID_ARG = -8, -2, -1
INVALID_DISTANCE = 7


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


def _cuda(data):
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda() if len(data) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _wide(comp, blob, cap=None, total=None, stream=None, call="sfh_decompress_bgzf_wide_device"):
    """the device call -> (bytes written, status).  dst is filled with 0xA5 first: a refused call leaves all of it alone, and
    no call writes behind the file's total_n -- on success that is dst_n_out.  (A file with a failing member: the device
    call decodes straight into dst, as sfh_decompress_bgzf_device does, so the good members' bytes are there and dst_n_out
    is 0; it is the host-buffer call that leaves dst alone unless the status is 0.)"""
    total = len(gzip.decompress(blob)) if total is None else total
    cap = total if cap is None else cap
    out = torch.full((max(total, 16) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    got, st = C.c_uint64(0), C.c_uint32(9)
    src = _cuda(blob)
    torch.cuda.synchronize()
    rc = getattr(_capi.lib(), call)(comp._h, src.data_ptr() if len(blob) else None, len(blob), out.data_ptr(), cap, C.byref(got), C.byref(st),
                                    C.c_void_p(stream) if stream else None)
    if rc:
        assert bool((out == 0xA5).all()), "a refused call writes nothing"
        raise StarflateError(rc, comp.last_error())
    if stream:
        torch.cuda.synchronize()
    back = out.cpu().numpy()
    assert got.value == (total if st.value == 0 else 0)
    assert np.all(back[total:] == 0xA5), "dst behind the file's bytes is untouched"
    return back[: got.value].tobytes(), int(st.value)


def _both(comp, blob, data, key):
    assert gzip.decompress(blob) == data, key  # the file is what it is meant to be
    assert _wide(comp, blob) == (data, 0), key
    assert comp.decompress_bgzf(blob) == (data, 0), key
    out, n, st = comp.decompress_bgzf_wide_tensor(_cuda(blob), len(data))
    assert (out[:n].cpu().numpy().tobytes(), st) == (data, 0), key


def file_of(members):
    return b"".join(members) + BZ.EOF


# ---- member sizes ----
def test_member_sizes(comp):
    sizes = [32769, 0, 40001, 1, 65280, 32768, 65535, 65536]
    data = BZ.text(sum(sizes), seed=2)
    blob, moff, ooff = BZ.write(data, sizes)
    assert BZ.walk(blob)[2] == 65536 and any(o % 16 for o in ooff)  # outputs off every alignment: the byte stage with a write window
    _both(comp, blob, data, "sizes")
    big = BZ.good_files()["65280-byte members"]
    _both(comp, big[1], big[0], "65280-byte members")
    assert comp.decompress_bgzf(b"") == (b"", 0) and _wide(comp, b"", total=0) == (b"", 0)
    assert _wide(comp, BZ.EOF, total=0) == (b"", 0)


# ---- block shapes in a 65280-byte member ----
BLOCKS = {"one coded block": 1, "fixed": 1, "one stored block above the window": 1, "two stored blocks": 2,
          "a coded block, then a stored one": 2, "14 flushed blocks": 14, "nibbles, four blocks or more": None}


@pytest.fixture(scope="module")
def shapes():
    """name -> (payload, member, blocks with output)"""
    return {name: (payload, K.hand_member(body, payload), BLOCKS[name]) for name, (payload, body) in K.shape_cases().items()}


def test_block_shapes(comp, shapes):
    for name, (payload, member, _) in shapes.items():
        _both(comp, file_of([member]), payload, name)
    # all of them in one file: the wave's two halves on unlike members
    blob = file_of([m for _, m, _ in shapes.values()])
    data = b"".join(p for p, _, _ in shapes.values())
    _both(comp, blob, data, "all shapes")


def test_both_wide_token_kernels_ran(comp, shapes):
    """SFH_DBG_SEGINFO bit 1: the lane-serial kernel finished the row.  The speculative wave follows 8 blocks with output"""
    names = ["one coded block", "14 flushed blocks", "nibbles, four blocks or more", "one stored block above the window"]
    blob = file_of([shapes[n][1] for n in names])
    data = b"".join(shapes[n][0] for n in names)
    assert _wide(comp, blob) == (data, 0)
    info = comp.debug(_capi.DBG_SEGINFO, len(names) + 1)
    serial = [int(v) >> 1 & 1 for v in info[:, 2]]
    assert serial[0] == 0 and serial[1] == 1, serial
    assert serial[2] == 0, "four to eight blocks are the speculative wave's"
    assert int(info[3, 2]) & 1 and serial[3] == 0, "one stored block: the raw copy"
    assert [int(v) for v in info[:4, 3]] == [WIDE] * 4 and [int(v) for v in info[:, 0]] == [0] * 5


# ---- matches the narrow rows never see ----
@pytest.fixture(scope="module")
def far():
    return {name: (payload, K.hand_member(body, payload)) for name, (payload, body) in K.far_cases().items()}


def test_far_matches(comp, far):
    for name, (payload, member) in far.items():
        _both(comp, file_of([member]), payload, name)
    _both(comp, file_of([m for _, m in far.values()]), b"".join(p for p, _ in far.values()), "all")


def test_distance_before_the_member(comp, far):
    """a match at position 100 with distance 101 in a member of 40000 bytes: InvalidDistance, a status and no fault; the
    earlier, good member's position in the file does not lend it history"""
    body, claims = K.invalid_distance()
    bad = K.hand_member(body, b"\0" * claims)
    good = far["a match straddling 32768"][1]
    for blob, k in ((file_of([bad]), 0), (file_of([good, bad]), 1)):
        total = BZ.walk(blob)[1][-1]
        assert _wide(comp, blob, total=total) == (b"", INVALID_DISTANCE), k
        assert f"member {k}:" in comp.last_error()
        assert comp.decompress_bgzf(blob) == (b"", INVALID_DISTANCE), k


# ---- launch batches ----
def test_launch_batches_and_scratch():
    """SFH_BATCH_CHUNKS=4 in a fresh process: a wide launch batch holds 2 members, 9 members take five; the token scratch is
    2 members x 65536 tokens x 4 bytes"""
    code = ("import sys, gzip\n"
            f"sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
            "import numpy as np, torch\n"
            "import bgzf_files as BZ\n"
            "from starflate_amd import Compressor\n"
            "data = BZ.text(8 * 65280 + 33000, seed=12)\n"
            "blob = BZ.write(data, [65280] * 4 + [33000] + [65280] * 4)[0]\n"
            "c = Compressor(0)\n"
            "out, n, st = c.decompress_bgzf_wide_tensor(torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda(), len(data))\n"
            "assert st == 0 and out[:n].cpu().numpy().tobytes() == data == gzip.decompress(blob)\n"
            "print(c.last_decode_scratch_bytes())\n"
            "assert c.decompress_bgzf(blob) == (data, 0)\n")
    env = dict(os.environ, SFH_BATCH_CHUNKS="4", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert int(out.stdout.split()[-1]) == 2 * 65536 * 4


# ---- a caller's stream; one context, the narrow and the wide call in turn ----
def test_callers_stream_and_context_reuse(comp):
    big = BZ.good_files()["65280-byte members"]
    small = BZ.good_files()["sizes eof=True"]
    stream = torch.cuda.Stream()
    for _ in range(2):
        assert _wide(comp, small[1], stream=stream.cuda_stream, call="sfh_decompress_bgzf_device") == (small[0], 0)
        assert _wide(comp, big[1], stream=stream.cuda_stream) == (big[0], 0)
    assert _wide(comp, small[1], call="sfh_decompress_bgzf_device") == (small[0], 0)
    assert _wide(comp, small[1]) == (small[0], 0)  # a file of narrow members through the wide call


# ---- damage ----
@pytest.fixture(scope="module")
def three():
    data = BZ.text(3 * WIDE, seed=21)
    blob, moff, ooff = BZ.write(data, [WIDE] * 3)
    return data, blob, moff


def _alone(comp, blob, k):
    """what the stream decoder -- the host call's path for such members before the wide rows -- says of member k alone, by
    sfh_decompress_bgzf's rule: the item's status, or Error when it produced other than ISIZE bytes"""
    moff = BZ.walk(blob)[0]
    m = blob[moff[k]: moff[k + 1]]
    isize = struct.unpack("<I", m[-4:])[0]
    got, st = comp.decompress_stream(m, out_n=isize, container="gzip")
    return st if st else (0 if len(got) == isize else 1)


def test_damaged_members(comp, three):
    data, blob, moff = three
    flip = lambda b, at: BZ.patched(b, at, bytes([b[at] ^ 0x40]))  # noqa: E731
    body1 = moff[2] - moff[1] - 26
    cases = [(f"CRC of member {k}", flip(blob, moff[k + 1] - 8), k, len(data)) for k in range(3)]
    cases += [("body byte 40 of member 1", flip(blob, moff[1] + 18 + 40), 1, len(data)),
              ("the last quarter of member 1's body", flip(blob, moff[1] + 18 + body1 - body1 // 8), 1, len(data)),
              ("ISIZE of the last member + 1", BZ.patched(blob, moff[3] - 4, struct.pack("<I", WIDE + 1)), 2, len(data) + 1),
              # the earliest damaged member wins
              ("CRC of member 1, body of member 2", flip(flip(blob, moff[2] - 8), moff[2] + 18 + 40), 1, len(data)),
              ("body of member 0, CRC of member 2", flip(flip(blob, moff[0] + 18 + 40), moff[3] - 8), 0, len(data))]
    for name, bad, k, total in cases:
        want = _alone(comp, bad, k)
        got = _wide(comp, bad, total=total)
        print(name, "stream decoder:", want, "wide rows:", got[1])
        assert want != 0, name
        assert got == (b"", want), name
        assert f"member {k}:" in comp.last_error(), name
        assert comp.decompress_bgzf(bad) == (b"", want), name


def test_truncated_files(comp, three):
    """a cut inside member 1's header, body and trailer: the walk ends there in SrcTooSmall, as it does on the host, and
    nothing is decoded"""
    data, blob, moff = three
    for cut in (moff[1] + 7, moff[1] + 14, moff[1] + 500, moff[2] - 5, moff[2] - 1):
        with pytest.raises(BZ.WalkError) as e:
            BZ.walk(blob[:cut])
        assert e.value.status == 5
        assert _wide(comp, blob[:cut], total=len(data)) == (b"", 5), cut
        assert "BGZF members:" in comp.last_error()
        assert comp.decompress_bgzf(blob[:cut]) == (b"", 5), cut


# ---- refusals; the narrow call's contract ----
def test_refusals(comp, three):
    data, blob, moff = three
    over = BZ.patched(blob, moff[2] - 4, struct.pack("<I", 65537))  # ISIZE of member 1: not BGZF
    host_before = comp.decompress_bgzf(over)
    assert host_before[0] == b"" and host_before[1] != 0  # (the stream decoder's: the member holds 65280 bytes)
    with pytest.raises(StarflateError) as e:
        _wide(comp, over, total=len(data) + 257)
    assert e.value.code == NOT_INDEXABLE
    with pytest.raises(StarflateError) as e:
        _wide(comp, blob, cap=len(data) - 1)
    assert e.value.code == DST_TOO_SMALL
    L, h = _capi.lib(), comp._h
    src = _cuda(b"\0" + blob)
    out = torch.full((len(data) + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    got, st = C.c_uint64(0), C.c_uint32(0)
    f = L.sfh_decompress_bgzf_wide_device
    assert f(h, src.data_ptr() + 1, len(blob), out.data_ptr(), len(data), C.byref(got), C.byref(st), None) == INVALID_ARG  # src off 4
    src4 = _cuda(b"\0" * 4 + blob)
    assert f(h, src4.data_ptr() + 4, len(blob), out.data_ptr() + 8, len(data), C.byref(got), C.byref(st), None) == INVALID_ARG  # dst off 16
    assert f(h, None, len(blob), out.data_ptr(), len(data), C.byref(got), C.byref(st), None) == INVALID_ARG
    assert f(h, src4.data_ptr() + 4, len(blob), None, len(data), C.byref(got), C.byref(st), None) == INVALID_ARG
    assert f(h, src4.data_ptr() + 4, len(blob), out.data_ptr(), len(data), None, C.byref(st), None) == INVALID_ARG
    assert f(h, src4.data_ptr() + 4, len(blob), out.data_ptr(), len(data), C.byref(got), None, None) == INVALID_ARG
    assert f(None, src4.data_ptr() + 4, len(blob), out.data_ptr(), len(data), C.byref(got), C.byref(st), None) == INVALID_ARG
    assert bool((out == 0xA5).all())
    assert f(h, src4.data_ptr() + 4, len(blob), out.data_ptr(), len(data), C.byref(got), C.byref(st), None) == 0
    assert (got.value, st.value) == (len(data), 0) and out[: len(data)].cpu().numpy().tobytes() == data


def test_narrow_call_keeps_its_contract(comp):
    big = BZ.good_files()["65280-byte members"]
    with pytest.raises(StarflateError) as e:
        _wide(comp, big[1], call="sfh_decompress_bgzf_device")
    assert e.value.code == NOT_INDEXABLE
    with pytest.raises(StarflateError) as e:
        comp.decompress_bgzf_tensor(_cuda(big[1]), len(big[0]))
    assert e.value.code == NOT_INDEXABLE
