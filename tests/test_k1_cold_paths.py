"""k_lz77's cold paths: the code a strip of text never runs, or runs once (round 12).

The stored-fast-path block behind a chunk's first round (the chunk's other rounds taken in one go: stored by the probe, or
counted as literals with `kItemsSkipped`), the reload of the window behind such a chunk, the short probe of the chunk behind
it, the byte-by-byte branch of a strip's short last chunk, the strip's last bytes in `load4`, a round cut short, the chunk
end and the empty input all work from opaque copies of the thread index, so that their lane tests and addresses are made where
they are used and do not sit, spilled, in the round loop's registers.  The inputs below are the smallest that send a strip
through each of them; every case is compared with the specification: the stream bit for bit, the chunks' histograms
(DBG_HIST), token and item counts, the sub-index, and a zlib round trip -- at strips of 32 KiB and 64 KiB (and the strip that
holds the whole input where a case is about ONE strip), over the five table kernels, one exact-recency and one hash-chain
kernel (they share the kernel body).  Which chunks carry `kItemsSkipped` is asserted at the default effort only, whose
classes the CPU test pins down; the batch call, once, is held to the streams and the zlib round trip.

The first test needs no GPU: it holds every generator to its class on the oracle's tokens -- which chunks are stored by the
probe, which take the fast path and are not stored, which are coded."""
import functools
import zlib

import numpy as np
import pytest

import oracle_lib as O
from starflate_amd import _capi, synth
from test_gpu_parity import EFFORT_PARAMS

CHUNK = 32768    # kChunk
ROUND = 8192     # kRound = kSkipSpan: the probe span
SLACK = 128      # kSkipSlack
REGION = 512     # kRegion: the parse region the oracle counts tokens by
SKIPPED = 0x80000000  # kItemsSkipped

EFFORTS = ("default", "fast", "fastest", "thorough", "max", "recent", "best")
STORED, LITERALS, CODED = "stored", "literals", "coded"  # by the probe / fast path taken, not stored / matched and parsed


@functools.lru_cache(maxsize=1)
def cases():
    """name -> (bytes, strip sizes, the class of every chunk at every one of those strip sizes)"""
    rng = np.random.default_rng(1212)
    noise = rng.integers(0, 256, 3 * CHUNK, dtype=np.uint8)
    six = rng.integers(0, 64, CHUNK, dtype=np.uint8)
    text = synth.gen_text(3 * CHUNK, seed=12)
    cat = np.concatenate
    S, L, C = STORED, LITERALS, CODED
    out = {
        # one full chunk of noise: stored by the probe -- no tokens, no histogram
        "noise": (noise[:CHUNK], (CHUNK, 2 * CHUNK), [S]),
        # one full chunk of six-bit bytes: the fast path taken, not stored -- kItemsSkipped, the byte counts on the 32 copies
        "six_bit": (six, (CHUNK, 2 * CHUNK), [L]),
        # noise, text, noise, text in ONE strip: the reload, the short probe behind a skipped chunk, the epoch catching up
        "noise_text_noise_text": (cat([noise[:CHUNK], text[:CHUNK], noise[CHUNK: 2 * CHUNK], text[CHUNK: 2 * CHUNK]]),
                                  (CHUNK, 2 * CHUNK, 4 * CHUNK), [S, C, S, C]),
        # a run of zeros from the first byte behind a skipped chunk (round 6: the window's last byte is read there)
        "noise_zeros": (cat([noise[:CHUNK], np.zeros(20000, np.uint8)]), (CHUNK, 2 * CHUNK), [S, C]),
        # a strip's short last chunk takes the fast path with more than 8 KiB and less than 32 KiB of noise: byte by byte
        "text_short_noise": (cat([text[:CHUNK], noise[:20000]]), (CHUNK, 2 * CHUNK), [C, L]),
        # two strips, the first ends in a skipped chunk: a strip's first round behind it
        "skip_ends_strip": (cat([text[:CHUNK], noise[:CHUNK], text[CHUNK: CHUNK + 40000]]), (CHUNK, 2 * CHUNK), [C, S, C, C]),
        # six-bit bytes in front of text in one strip: the reload behind a chunk that was counted, not stored
        "six_text": (cat([six, text[:CHUNK + 777]]), (CHUNK, 2 * CHUNK, 4 * CHUNK), [L, C, C]),
        "empty": (np.zeros(0, np.uint8), (CHUNK, 2 * CHUNK), [C]),
    }
    # the strip's last bytes, a round cut short, load4's guard
    for n in (1, ROUND - 1, ROUND + 1, 2 * CHUNK + ROUND + 5):
        out[f"text{n}"] = (text[:n], (CHUNK, 2 * CHUNK), [C] * max(1, -(-n // CHUNK)))
    for data, _, _ in out.values():
        data.setflags(write=False)
    return out


def params(effort, bb):
    return O.default_params(strip_bytes=bb, **EFFORT_PARAMS[effort])


@functools.lru_cache(maxsize=None)
def want(name, effort, bb):
    """the specification's side of one case: stream, sub-index, per chunk (tokens, literal/length and distance counts)"""
    data = cases()[name][0]
    p = params(effort, bb)
    stream, _, sub = O.compress_indexed(data, p)
    chunks = [(flat, *O.histogram(tarr, nt, p.region_bytes)) for flat, nt, tarr in O.chunk_tokens(data, p)]
    stream.setflags(write=False)
    return stream, sub, chunks


def chunk_class(flat, size, probe_tokens):
    """probe_tokens: tokens of the chunk's first kSkipSpan positions when the fast path is off -- the rule's own figure (a
    chunk longer than the span whose span parses to kSkipSpan - kSkipSlack tokens or more takes the fast path)"""
    if flat.size == 0 and size:
        return STORED
    if size > ROUND and probe_tokens >= ROUND - SLACK:
        assert flat.size == size and not np.count_nonzero(flat & 0x80000000), "fast path taken: every byte a literal"
        return LITERALS
    return CODED


@pytest.mark.parametrize("name", sorted(cases()))
def test_generators_hit_their_classes(name):
    """on the CPU, from the oracle's tokens at the default effort: a chunk is stored by the probe (no tokens), or took the
    fast path and is not stored (its probe span is all but literals, and so every byte of it is a literal), or is coded; the
    classes do not depend on the strip size"""
    data, strips, classes = cases()[name]
    for bb in strips:
        chunks = want(name, "default", bb)[2]
        plain = O.chunk_tokens(data, O.default_params(strip_bytes=bb, fast_skip=0))
        assert len(chunks) == len(classes) == len(plain), (name, bb)
        for c, (flat, _, _) in enumerate(chunks):
            size = min(CHUNK, data.size - c * CHUNK)
            probe_tokens = int(plain[c][1][: ROUND // REGION].sum())
            assert chunk_class(flat, size, probe_tokens) == classes[c], (name, bb, c)
    sizes = {n: cases()[n][0].size for n in cases()}
    assert sizes["noise"] == sizes["six_bit"] == CHUNK and sizes["text_short_noise"] - CHUNK == 20000 and sizes["empty"] == 0
    assert {1, 8191, 8193, 65536 + 8192 + 5} <= set(sizes.values())


def check(compressor, name, effort, bb):
    data, _, classes = cases()[name]
    stream, sub, chunks = want(name, effort, bb)
    got = np.frombuffer(compressor.compress(data, effort=effort, block_bytes=bb), np.uint8)
    tag = (name, effort, bb)
    assert got.size == stream.size and np.array_equal(got, stream), tag
    assert np.array_equal(compressor.last_subindex(), sub), tag
    assert zlib.decompress(got.tobytes(), -15) == data.tobytes(), tag
    nch = len(chunks)
    ntok = compressor.debug(_capi.DBG_NTOK, nch)
    nitems = compressor.debug(_capi.DBG_NITEMS, nch)
    hist = compressor.debug(_capi.DBG_HIST, nch)
    for c, (flat, ll, dd) in enumerate(chunks):
        assert ntok[c] == flat.size, tag + (c, "tokens")
        assert (int(nitems[c]) & (SKIPPED - 1)) == flat.size + np.count_nonzero(flat & 0x80000000), tag + (c, "items")
        if effort == "default":  # (the classes are the default effort's: the CPU test above)
            assert bool(int(nitems[c]) & SKIPPED) == (classes[c] != CODED), tag + (c, "kItemsSkipped")
        if flat.size or not data.size:  # (a chunk stored by its probe has no histogram)
            assert np.array_equal(hist[c, :286], ll) and np.array_equal(hist[c, 288:318], dd), tag + (c, "histogram")


@pytest.mark.gpu
@pytest.mark.parametrize("effort", EFFORTS)
def test_cold_paths_vs_specification(compressor, effort):
    for name, (_, strips, _) in cases().items():
        for bb in strips:
            check(compressor, name, effort, bb)


@pytest.mark.gpu
def test_cold_paths_through_the_batch_call(compressor):
    """the batch kernel takes a strip's bytes, size and first chunk from the strip table: the same inputs, one item each"""
    names = [n for n in cases() if cases()[n][0].size]  # (an item of no bytes is not a batch item)
    items = [cases()[n][0] for n in names]
    for bb in (CHUNK, 2 * CHUNK):
        outs = compressor.compress_batch(items, block_bytes=bb)
        for name, item, out in zip(names, items, outs):
            assert np.array_equal(np.frombuffer(out, np.uint8), want(name, "default", bb)[0]), (name, bb)
            assert zlib.decompress(out, -15) == item.tobytes(), (name, bb)
