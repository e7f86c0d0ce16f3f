"""The stored-block start predicate of the stream decoder (stored_header_candidate, sf_inflate_core.h; DESIGN.md 3a "Stored
block starts"), compiled for the host and tried at every bit offset: it equals its closed form (one candidate per LEN byte B
with body[B - 1] < 32, at bit 8(B - 1) + bit_length(body[B - 1])), it holds on the LEN byte of every non-final stored block
of zlib streams (the true starts from the block walk of tests/deflate_writer.py) and at the exact start bit wherever the
block before ends on a byte boundary, its false hits on noise stay near 2 per MiB, and each of its four rules rejects."""
import zlib

import numpy as np
import pytest

import deflate_writer as W
import stream_host as H
import stream_stored_host as HS
from starflate_amd import synth


def _raw(data, level=6, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem)
    return c.compress(data) + c.flush()


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _stripes(n, stripe=100000):
    parts = [synth.gen_text(stripe, seed=k).tobytes() if k % 2 == 0 else _noise(stripe, 100 + k) for k in range(-(-n // stripe))]
    return b"".join(parts)[:n]


def _stored(stream):
    """[(start bit, LEN byte)] of the non-final stored blocks"""
    _, blocks = W.inflate(np.frombuffer(stream, np.uint8))
    assert blocks[-1]["type"] != 0 or len(blocks) > 1
    return [(b["start"], (b["start"] + 10) // 8) for b in blocks[:-1] if b["type"] == 0]


NOISE = _noise(1 << 20, 7)


def test_brute_force_equals_closed_form():
    level0 = _raw(synth.gen_text(1 << 20, seed=3).tobytes(), 0)
    assert H.scan(level0) == []  # (no dynamic-header hit in it: the stream the GPU test cuts at its stored blocks)
    crafted = [b"", b"\x00", bytes(4), bytes(5), bytes(6), b"\x00\x00\x00\xff\xff", b"\x1f\x00\x00\xff\xff", b"\x20\x00\x00\xff\xff",
               b"\x00\x01\x00\xfe\xff", b"\x00\x01\x00\xfe\xffx", bytes(64), b"\xff" * 64,
               b"".join(bytes([v, 2, 0, 0xFD, 0xFF, 7, 7]) for v in range(256)),
               b"".join(bytes([v, 0, 0, 0xFF, 0xFF]) for v in range(64)) + bytes(3)]
    for body in [NOISE, level0] + crafted:
        got, want = HS.scan(body), sorted(HS.closed_form(body))
        assert got == want, (len(body), got[:5], want[:5])
    assert len(HS.scan(level0)) >= 16 and len(HS.scan(crafted[-2])) == 32


@pytest.mark.parametrize("name", ["level0-text", "level0-noise", "level1-noise", "level6-noise-mem1", "level6-noise-mem8",
                                  "level6-noise-mem9"])
def test_true_starts_exact(name):
    data, level, mem = {"level0-text": (synth.gen_text(1 << 20, seed=3).tobytes(), 0, 8), "level0-noise": (NOISE, 0, 8),
                        "level1-noise": (NOISE, 1, 8), "level6-noise-mem1": (NOISE[:200000], 6, 1),
                        "level6-noise-mem8": (NOISE, 6, 8), "level6-noise-mem9": (NOISE, 6, 9)}[name]
    stream = _raw(data, level, mem)
    stored = _stored(stream)
    assert len(stored) >= 4, len(stored)
    hits = set(HS.scan(stream))
    assert all(any(8 * (B - 1) <= h < 8 * B for h in hits) for _, B in stored)
    assert all(p in hits for p, _ in stored), [p for p, _ in stored if p not in hits]


def test_true_starts_behind_huffman_blocks():
    """text / noise stripes at level 6: a stored block behind a Huffman block starts wherever that block's last code ends;
    its LEN byte always has a hit, and the hit is the start bit when the bit before the header is 1 or a byte ends there"""
    stream = _raw(_stripes(1000000), 6)
    stored = _stored(stream)
    hits = set(HS.scan(stream))
    assert len(stored) >= 20, len(stored)
    assert all(any(8 * (B - 1) <= h < 8 * B for h in hits) for _, B in stored)
    exact = sum(p in hits for p, _ in stored)
    print("non-final stored starts", len(stored), "exact", exact)
    assert 2 * exact >= len(stored), (exact, len(stored))


def test_false_hits_noise():
    hits = HS.scan(NOISE)
    print("stored-predicate hits on 1 MiB of noise:", len(hits))
    assert len(hits) <= 16, len(hits)  # expectation 2^20 * 2^-19 = 2; 16 or more: below 1e-9


def test_rejections():
    def stream(pad_bits=0, final=0, lead=None, ln=5, nlen=None, payload=None, lead_n=0):
        bw = W.BitWriter()
        if lead_n:
            bw.put(lead, lead_n)
        bw.put(final, 1)
        bw.put(0, 2)
        k = -bw.n % 8
        bw.put(pad_bits, k)
        bw.put(ln, 16)
        bw.put(ln ^ 0xFFFF if nlen is None else nlen, 16)
        bw.put(int.from_bytes(b"x" * ln if payload is None else payload, "little"), 8 * (ln if payload is None else len(payload)))
        return bw.bytes().tobytes()

    assert HS.scan(stream()) == [0]
    assert HS.scan(stream(lead=0b11, lead_n=2)) == [2]  # behind a code ending in 1
    assert HS.scan(stream(lead=0b11111, lead_n=5)) == [5]
    # BFINAL 1: no hit at the block's start (the zero bits behind it are a start of their own, a false one: by rule 2 a set bit
    # in front of a zero run is where a block may have ended)
    assert HS.scan(stream(final=1)) == [1] and HS.scan(stream(final=1), hi=1) == []
    assert HS.scan(stream(final=1, lead=0b111, lead_n=3)) == [4]
    assert HS.scan(stream(final=1, lead=0b11111, lead_n=5)) == []
    for bit in range(16):
        assert HS.scan(stream(nlen=(5 ^ 0xFFFF) ^ (1 << bit))) == []
    assert HS.scan(stream(payload=b"xxxx")) == []  # LEN reaches one byte past the body
    assert HS.scan(stream(payload=b"xxxxx")) == [0]
    for bit in range(5):  # a non-zero padding bit: never at the block's start; the zero bits above it stand for themselves
        assert HS.scan(stream(pad_bits=1 << bit)) == ([bit + 4] if bit < 2 else [])
    # a non-canonical p: a zero bit just before it inside the same byte; only the lowest zero bit of the run is the candidate
    s = stream(lead=0b001, lead_n=3)
    assert HS.scan(s) == [1]
    assert HS.scan(s, lo=2) == [] and HS.scan(s, lo=3, hi=4) == []
    # a header that straddles two bytes (bit 6 or 7): the candidate is the first bit of the byte in front of LEN
    assert HS.scan(stream(lead=0b111111, lead_n=6)) == [8]
    assert HS.scan(stream(lead=0b1111111, lead_n=7)) == [8]
    # B + 4 > body_n: the fields do not fit
    whole = stream(ln=0)
    assert HS.scan(whole) == [0]
    for cut in range(1, 5):
        assert HS.scan(whole[:-cut]) == []


def _run_members(blocks):
    """LEN bytes of the non-final stored blocks whose next block is a stored one too"""
    return [(b["start"] + 10) // 8 for b, nxt in zip(blocks, blocks[1:]) if b["type"] == 0 and nxt["type"] == 0]


@pytest.mark.parametrize("level,mem,n", [(0, 8, 1 << 20), (6, 8, 1 << 20), (6, 7, 1 << 20), (6, 6, 1 << 20), (6, 1, 300000)])
def test_finder_keeps_every_run_member(level, mem, n):
    """what k_stream_find asks besides the predicate, a stored header behind the payload (stored_run_follows), keeps every
    stored block of a run but its last, however short the blocks are: about 65535 bytes at level 0, 16 KiB, 8 KiB and 4 KiB at
    memLevel 8, 7 and 6, 127 bytes at memLevel 1.  Behind a stored block the start is exact"""
    stream = _raw(NOISE[:n], level, mem)
    _, blocks = W.inflate(np.frombuffer(stream, np.uint8))
    members = _run_members(blocks)
    assert len(members) >= len(blocks) - 2 >= (1 << 20) // 70000
    hits = set(HS.scan(stream, look=True))
    print(level, mem, "blocks", len(blocks), "run members", len(members), "taken", len(hits))
    assert all(8 * (B - 1) in hits for B in members)
    assert hits <= set(HS.scan(stream))


def test_finder_on_mixed_stream():
    """text / noise stripes: every stored block in front of a stored one is taken, the last of each run and no other"""
    stream = _raw(_stripes(1000000), 6)
    _, blocks = W.inflate(np.frombuffer(stream, np.uint8))
    members = _run_members(blocks)
    last = [(b["start"] + 10) // 8 for b, nxt in zip(blocks, blocks[1:]) if b["type"] == 0 and nxt["type"] != 0]
    hits = HS.scan(stream, look=True)
    assert len(members) >= 15 and len(last) >= 4
    assert all(any(8 * (B - 1) <= h < 8 * B for h in hits) for B in members)
    assert not any(8 * (B - 1) <= h < 8 * B for h in hits for B in last)


def test_look_ahead_on_noise():
    """a false hit that survives needs a second `LEN NLEN` pair and BTYPE 0 where its payload ends: 2^-18 of them"""
    noise = _noise(8 << 20, 11)
    plain, looked = HS.scan(noise), HS.scan(noise, look=True)
    print("false hits on 8 MiB of noise:", len(plain), "with the look-ahead:", len(looked))
    assert 4 <= len(plain) <= 64  # expectation 16
    assert looked == []  # expectation 16 * 2^-18


def test_look_ahead_rules():
    def body(follow):
        return b"\x00\x02\x00\xfd\xffab" + follow

    assert HS.scan(body(b"")) == [0] and HS.scan(body(b""), look=True) == []  # nothing follows
    for first in (0x02, 0x04, 0x05, 0x06, 0x07):  # fixed, dynamic, type 3
        assert HS.scan(body(bytes([first]) + b"\x00\x00\xff\xff"), look=True) == []
    assert HS.scan(body(b"\x00\x00\x00\xff\xff"), look=True)[0] == 0
    assert HS.scan(body(b"\x01\x00\x00\xff\xff"), look=True)[0] == 0  # a final stored block
    assert HS.scan(body(b"\x08\x01\x00\xfe\xffz"), look=True)[0] == 0  # non-zero padding bits are the format's right
    assert HS.scan(body(b"\x01\x00\x00\xff\xfe"), look=True) == []
    assert HS.scan(body(b"\x00\x00\x00\xff"), look=True) == []  # its LEN and NLEN do not fit
    assert HS.scan(body(b"\x00\x09\x00\xf6\xff"), look=True)[0] == 0  # (whether that block's payload fits is its lane's to find)
