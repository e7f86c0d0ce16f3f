"""Length-limited Huffman codes at the caps of RFC 1951 on the GPU (the CPU side: tests/test_code_limits.py).

Compressor: the inputs of test_code_limits.deep_input drive k_plan past the caps -- an unconstrained literal/length tree
17 deep, a distance tree 16 deep, a code-length code deeper than 7 -- so finish_lengths' Kraft repair runs, canonical_codes
reverses 15-bit codes and k_emit writes a 15-bit length code with 5 extra bits (20 bits, the whole value field of its table
entry) and a 15-bit distance code with 13 (28 bits).  Histograms, lengths, plans and streams must equal the oracle's
chunk by chunk, and the GPU's lengths must be legal on their own.

Decoder: writer-made streams (tests/deflate_writer.py) with codes of every length 1..15, end-of-block on a 15-bit code,
7-bit code-length codes, one distance code of length 1, no distance code at all, several trees in one segment, and a
seeded set of random length-limited codes, through every decode path: index + sub-index (k_inflate_tokens_sub), index
only (speculative + lane-serial), SFH_INFLATE_SERIAL=1 (lane-serial) and the batch entry point."""
import zlib

import numpy as np
import pytest

import deflate_writer as W
import oracle_lib as O
from starflate_amd import _capi
from test_code_limits import (CHUNK, STRATEGIES, STRIPS, assert_edges_written, check_code, chunk_histograms, deep_input,
                              edge_segments, oracle_params, random_pages, stream_blocks, unconstrained)

pytestmark = pytest.mark.gpu


def _gpu_chunk_checks(compressor, data, deep, p, got, nch):
    hist = compressor.debug(_capi.DBG_HIST, nch)
    lens = compressor.debug(_capi.DBG_LENS, nch)
    plan = compressor.debug(_capi.DBG_PLAN, nch)
    ref = chunk_histograms(data, p)
    for c in range(nch):
        ll, dd = ref[c]
        assert np.array_equal(hist[c, :286], ll) and np.array_equal(hist[c, 288:318], dd), f"chunk {c}: hist"
        pl = O.plan_chunk(ll, dd, min(CHUNK, data.size - c * CHUNK), c + 1 == nch, p)
        assert plan[c, 0] == pl.btype and plan[c, 1] == pl.out_bytes, f"chunk {c}: plan"
        if pl.btype == 2:
            assert np.array_equal(lens[c, :288], np.frombuffer(pl.ll_lens, np.uint8)), f"chunk {c}: ll lens"
            assert np.array_equal(lens[c, 288:320], np.frombuffer(pl.d_lens, np.uint8)), f"chunk {c}: d lens"
    # the GPU's own numbers, without the oracle
    c = deep["ll"]
    assert unconstrained(hist[c, :286], hist[c, 288:318])[0] > 15
    check_code(lens[c, :286], 15, hist[c, :286])
    assert lens[c, 281] == 15 and hist[c, 281] == 1
    c = deep["d"]
    assert unconstrained(hist[c, :286], hist[c, 288:318])[1] > 15
    check_code(lens[c, 288:318], 15, hist[c, 288:318])
    assert lens[c, 288 + 29] == 15 and hist[c, 288 + 29] == 1
    index = compressor.last_index()
    blocks = stream_blocks(got, index, deep.values())
    hdr = blocks[deep["cl"]][0]["header"]
    assert max(W.huffman_depths(hdr["cl_freq"])) > 7
    check_code(hdr["cl_lens"], 7, hdr["cl_freq"])
    assert_edges_written(blocks, deep)
    return index


@pytest.mark.parametrize("strategy_name,strategy", STRATEGIES)
def test_compressor_past_the_caps(compressor, strategy_name, strategy):
    data, deep = deep_input()
    nch = (data.size + CHUNK - 1) // CHUNK
    for strip in STRIPS:
        p = oracle_params(strategy, strip)
        got = np.frombuffer(compressor.compress(data, strategy=strategy_name, stored_fast_path=False, block_bytes=strip,
                                                effort="best"), np.uint8)
        want = O.compress(data, p)
        assert got.size == want.size and np.array_equal(got, want), (strip, np.flatnonzero(got[: min(got.size, want.size)] != want[: min(got.size, want.size)])[:4])
        index = _gpu_chunk_checks(compressor, data, deep, p, got, nch)
        sub = compressor.last_subindex()
        assert zlib.decompress(got.tobytes(), -15) == data.tobytes()
        back, st = compressor.decompress(got, index, data.size, subindex=sub, block_bytes=strip)
        assert st == 0 and back == data.tobytes()
        back, st = compressor.decompress(got, index, data.size, block_bytes=strip)
        assert st == 0 and back == data.tobytes()


def test_compress_batch_past_the_caps(compressor):
    """k_plan's batch tables take n_raw and BFINAL from the chunk table: the same streams through compress_batch"""
    data, deep = deep_input()
    items = [data, data[CHUNK: 2 * CHUNK], data[: 2 * CHUNK]]
    outs = compressor.compress_batch(items, strategy="dynamic", stored_fast_path=False, block_bytes=65536, effort="best")
    for item, out in zip(items, outs):
        want = O.compress(item, oracle_params(3, 65536))
        assert np.array_equal(np.frombuffer(out, np.uint8), want)
        assert zlib.decompress(out, -15) == item.tobytes()
    _, index, _ = O.compress_indexed(data, oracle_params(3, 65536))
    assert_edges_written(stream_blocks(np.frombuffer(outs[0], np.uint8), index, deep.values()), deep)


@pytest.fixture(scope="module")
def serial():
    """a context made with SFH_INFLATE_SERIAL=1: the lane-serial kernel decodes every segment"""
    from starflate_amd import Compressor

    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SFH_INFLATE_SERIAL", "1")
        c = Compressor(0)
    yield c
    c.close()


def _every_path(compressor, serial, stream, idx, sub, data, bb, name):
    n = len(data)
    if sub is not None:
        back, st = compressor.decompress(stream, idx, n, subindex=sub, block_bytes=bb)
        assert st == 0 and back == data, (name, bb, "index + sub-index", st)
    back, st = compressor.decompress(stream, idx, n, block_bytes=bb)
    assert st == 0 and back == data, (name, bb, "index only", st)
    back, st = serial.decompress(stream, idx, n, block_bytes=bb)
    assert st == 0 and back == data, (name, bb, "lane-serial", st)
    outs, sts = compressor.decompress_batch([stream], [n], index=idx, subindex=sub, block_bytes=[bb])
    assert sts == [0] and outs[0] == data, (name, bb, "batch", sts)


def test_decoders_on_writer_streams(compressor, serial):
    seen = {"ll": set(), "d": set(), "cl": set(), "eob": set(), "len15x5": False, "dist15x13": False}
    for name, (segs, _) in edge_segments().items():
        one = all(len(b) == 1 for b in segs)
        stream, idx, sub, data, reps = W.write_stream(segs, subindex=one)
        assert zlib.decompress(stream.tobytes(), -15) == data
        for bb in (32768, 131072):
            _every_path(compressor, serial, stream, idx, sub, data, bb, name)
        for r in reps:
            seen["ll"] |= set(r["ll"])
            seen["d"] |= set(r["d"])
            seen["cl"] |= set(r["cl"])
            seen["eob"].add(r["eob"])
            seen["len15x5"] |= any(cl == 15 and ne == 5 and ev >= 16 for cl, ne, ev in r["len_items"])
            seen["dist15x13"] |= any(cl == 15 and ne == 13 and ev >= 4096 for cl, ne, ev in r["dist_items"])
        if one:  # the sub-indexed kernel's tokens are the writer's
            compressor.decompress(stream, idx, len(data), subindex=sub, block_bytes=32768)
            nseg = idx.size - 1
            info = compressor.debug(_capi.DBG_SEGINFO, nseg)  # status, tokens, raw | serial << 1, bytes, raw offset
            toks = compressor.debug(_capi.DBG_TOKENS, nseg)
            for c in range(nseg):
                want = segs[c][0][0]
                assert info[c, 0] == 0 and info[c, 1] == want.size and np.array_equal(toks[c, : want.size], want), (name, c)
    assert seen["ll"] >= set(range(1, 16)) and seen["d"] >= set(range(1, 16))
    assert 15 in seen["eob"] and 7 in seen["cl"] and seen["len15x5"] and seen["dist15x13"]


def test_decoders_on_random_length_limited_codes(compressor, serial):
    pages = random_pages(300)
    streams = [s for s, _, _ in pages]
    sizes = [len(d) for _, d, _ in pages]
    outs, sts = compressor.decompress_batch(streams, sizes)
    assert sts == [0] * len(pages)
    assert all(o == d for o, (_, d, _) in zip(outs, pages))
    assert any(15 in r["ll"] for _, _, r in pages) and any(15 in r["d"] for _, _, r in pages)
    # a few of them through the single-stream paths as well
    for s, d, _ in pages[:40]:
        idx = np.array([0, s.size], np.uint64)
        for c in (compressor, serial):
            back, st = c.decompress(s, idx, len(d), block_bytes=32768)
            assert st == 0 and back == d
