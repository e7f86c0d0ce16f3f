"""The block-start predicate of the stream decoder (dynamic_header_candidate, sf_inflate_core.h), compiled for the host: it
holds at every non-final dynamic block start of zlib streams (levels, memLevels, strategies; the true starts from the
independent block walk of tests/deflate_writer.py), and its false hits on noise and on stored payloads that hold DEFLATE
streams are counted and bounded.  A false hit costs time only: the chain rule (tests/test_stream_chain.py) drops it."""
import zlib

import numpy as np
import pytest

import deflate_writer as W
import stream_host as H
from starflate_amd import synth

STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE}


def _raw(data, level=6, mem=8, strategy="default"):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, STRATEGIES[strategy])
    return c.compress(data) + c.flush()


def _true_starts(stream):
    _, blocks = W.inflate(np.frombuffer(stream, np.uint8))
    return blocks


@pytest.mark.parametrize("level,mem,strategy", [(1, 8, "default"), (6, 8, "default"), (9, 8, "default"), (6, 1, "default"),
                                                (6, 9, "default"), (9, 1, "default"), (6, 8, "filtered"), (6, 8, "huffman"),
                                                (6, 8, "rle"), (1, 1, "huffman")])
def test_finds_every_dynamic_start(level, mem, strategy):
    data = synth.gen_mixed(120000 if mem < 9 else 500000, seed=level + mem, stripe=30000).tobytes()
    stream = _raw(data, level, mem, strategy)
    blocks = _true_starts(stream)
    want = [b["start"] for b in blocks if b["type"] == 2 and b is not blocks[-1]]
    assert len(want) >= 1
    hits = set(H.scan(stream))
    missed = [p for p in want if p not in hits]
    assert not missed, missed
    # every hit that is not a true start is a false one; they must stay rare
    false = len(hits - set(b["start"] for b in blocks))
    assert false <= max(2, len(stream) * 8 // 100000), (false, len(stream))


def test_false_hits_noise():
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    hits = H.scan(noise)
    assert len(hits) < 40, len(hits)  # over 8 Mi bit positions


def test_false_hits_stored_deflate_payload():
    """a level-0 stream whose payload is a DEFLATE stream: every inner block start is a (false) candidate of the outer one"""
    inner = _raw(synth.gen_text(400000, seed=9).tobytes(), 6, 1)
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    outer = c.compress(inner) + c.flush()
    inner_hits = H.scan(inner)
    outer_hits = H.scan(outer)
    assert len(inner_hits) > 10
    assert len(outer_hits) >= len(inner_hits) - 2  # (a start cut by a stored header may be lost)
    assert len(outer_hits) <= len(inner_hits) + 40


def test_rejects_final_fixed_stored_and_incomplete():
    # BFINAL = 1, fixed and stored blocks never qualify; neither does a dynamic header with an incomplete code
    assert H.scan(_raw(b"x" * 1000, 6)) == []  # one final block
    assert H.scan(_raw(synth.gen_text(50000, seed=2).tobytes(), 6, 8, "default")[:0]) == []
    bw = W.BitWriter()
    toks = [ord("a")] * 50 + [W.match(10, 1)]
    ll = [9 if i in (ord("a"), 256, W.len_symbol(10)[0]) else 0 for i in range(286)]
    W.write_dynamic(bw, toks, ll, [1] + [0] * 29)
    W.write_stored(bw, b"", final=True)
    assert H.scan(bw.bytes().tobytes()) == []
