"""Container::GzipMembers on the host: the specification (include/starflate/container.hpp, decompress_members) against
gzip.decompress and its statuses, sf_members.h's header_end / hop / head_candidate against the specification's own walk --
under AddressSanitizer and UBSan on every prefix of a three-member file -- and the Python entry points that keep refusing
container="gzip_members".  No device."""
import gzip
import os
import subprocess
import tempfile

import numpy as np
import pytest

import deflate_writer as W
import members_cases as MC
import members_host as MH
import stream_cases as SC

GOOD = MC.good()
BAD = MC.bad()


def heads(blob, rows):
    """where each member's head stands: the file's first byte, then the first non-zero byte behind each trailer but the last"""
    at = [0]
    for r in rows[:-1]:
        p = int(r["src_end"])
        while blob[p] == 0:
            p += 1
        at.append(p)
    return at


@pytest.mark.parametrize("name", sorted(GOOD))
def test_specification_reads_what_gzip_reads(name):
    blob = GOOD[name]
    want = gzip.decompress(blob)
    st, got, rows = MH.spec(blob, len(want) + 100)  # (dst may be larger than the output)
    assert st == 0 and got == want
    assert int(rows[-1]["out_end"]) == len(want) and int(rows[-1]["src_end"]) <= len(blob)
    st, got, _ = MH.spec(blob, len(want))
    assert st == 0 and got == want


def test_member_rows_are_the_members():
    t = MC.text(9000, 1)
    parts = [t[:3000], t[3000:6000], t[6000:]]
    st, _, rows = MH.spec(GOOD["three"], MC.BIG)
    assert st == 0 and len(rows) == 3
    src = out = 0
    for r, p in zip(rows, parts):
        src += len(MC.member(p))
        out += len(p)
        assert (int(r["src_end"]), int(r["out_end"]), int(r["crc32"]), int(r["isize"])) == (src, out, gzip.zlib.crc32(p), len(p))
    st, _, rows = MH.spec(GOOD["empties"], MC.BIG)
    assert st == 0 and len(rows) == 5 and [int(r["isize"]) for r in rows] == [0, 3000, 0, 0, 0]


@pytest.mark.parametrize("name", sorted(BAD))
def test_statuses(name):
    blob, cap, want = BAD[name]
    st, _, _ = MH.spec(blob, cap)
    assert st == want


def test_a_full_capacity_decodes_what_one_byte_less_refuses():
    blob, cap, _ = BAD["capacity_one_short"]
    st, got, _ = MH.spec(blob, cap + 1)
    assert st == 0 and got == gzip.decompress(blob)


def test_the_reaching_match_is_legal_inside_one_member():
    """the distance-5 block behind five bytes of its own member decodes: the status is about the member boundary alone"""
    b = SC.Builder()
    b.dynamic(list(b"abcde"))
    b.dynamic([W.match(10, 5)] + list(b"xyz"), final=True)
    out = bytes(b.out)
    assert out == b"abcde" + b"abcdeabcde" + b"xyz"
    st, got, _ = MH.spec(MC.member(b"") + MC.member(out, body=b.bw.bytes().tobytes()), MC.BIG)
    assert st == 0 and got == out


@pytest.mark.parametrize("name", sorted(GOOD) + sorted(BAD))
def test_device_steps_agree_with_the_specification(name):
    blob, cap = (GOOD[name], MC.BIG) if name in GOOD else BAD[name][:2]
    assert MH.agree(blob, cap) == 0


@pytest.mark.parametrize("name", sorted(GOOD))
def test_head_candidate_holds_at_every_head(name):
    blob = GOOD[name]
    _, _, rows = MH.spec(blob, MC.BIG)
    hits = set(MH.head_candidates(blob))
    assert set(heads(blob, rows)) <= hits


def test_head_candidate_nowhere_else_in_random_bytes():
    payload = np.random.default_rng(11).integers(0, 256, 60000, dtype=np.uint8).tobytes()
    b = SC.Builder()
    b.stored(payload, final=True)
    first = MC.member(payload, body=b.bw.bytes().tobytes())
    blob = first + MC.join([MC.text(500, 3)])
    assert MH.head_candidates(blob) == [0, len(first)]


def test_sanitizers_on_every_prefix():
    exe = MH.sanitizer_program()
    t = MC.text(900, 4)
    blob = MC.member(t[:300], flg=12, extra=b"ab\x01\x00c", name=b"x") + bytes(3) + MC.member(t[300:600], flg=18, comment=b"c") + \
        MC.member(t[600:])
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "three.gz")
        with open(path, "wb") as f:
            f.write(blob)
        r = subprocess.run([exe, path, "2000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d prefixes agree" % (len(blob) + 1) in r.stdout


@pytest.mark.parametrize("call", ["decompress", "decompress_batch", "decompress_any_batch"])
def test_other_decoders_refuse_the_container_without_a_device(call):
    import starflate_amd as sf
    from starflate_amd import _capi

    assert _capi.STREAM_CONTAINER["gzip_members"] == 4 and "gzip_members" not in _capi.CONTAINER
    blob = GOOD["one"]
    args = {"decompress": (blob, 3000), "decompress_batch": ([blob], [3000]), "decompress_any_batch": ([blob], [3000])}[call]
    with pytest.raises(ValueError):
        getattr(sf, call)(*args, container="gzip_members")
