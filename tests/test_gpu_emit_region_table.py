"""k_emit takes the region starts from k_lz77's table (DBG_RITEM: the item index of every 1024-byte region's first token), not
from the items' kItemRegion flags.  On every case: the table names exactly the flagged items, region by region; the sub-index
is what the reference writer (deflate_writer.write_dynamic, region_starts) records for the chunk's tokens under the chunk's
code, and what the encoder specification gives; and the sub-indexed GPU decode returns the input."""
import numpy as np
import pytest

import deflate_writer as W
import oracle_lib as O
from starflate_amd import Compressor, _capi, synth

pytestmark = pytest.mark.gpu

CHUNK = 32768
REGIONS = 32
SKIPPED = 0x80000000  # kItemsSkipped
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


def _line61(n, seed=9):
    line = np.random.default_rng(seed).integers(32, 127, 61, dtype=np.uint8)
    return np.tile(line, n // 61 + 1)[:n]


def _six_bit(n, seed=21):
    return np.random.default_rng(seed).integers(0, 64, n, dtype=np.uint8)


def _chunks_of(data):
    return [data[k: k + CHUNK] for k in range(0, max(data.size, 1), CHUNK)]


def _writer_subindex(tokens, ll, dl, header_bits):
    """{bit offset from the chunk's first bit, tokens before} of every region, from the reference writer's marks: its own
    header's bits out, the chunk's header's in"""
    rep = W.write_dynamic(W.BitWriter(), tokens, ll, dl, region_starts=[r * W.REGION for r in range(REGIONS)])
    return np.array([[rep["marks"][r * W.REGION][0] - rep["header_bits"] + header_bits, rep["marks"][r * W.REGION][1]]
                     for r in range(REGIONS)], np.int64)


def _check_tables(comp, chunks, sub):
    """the debug arrays of the compress call just made against its sub-index `sub` [chunks, 32, 2]"""
    nch = len(chunks)
    ritem = comp.debug(_capi.DBG_RITEM, nch)
    items = comp.debug(_capi.DBG_ITEMS, nch)
    nitems = comp.debug(_capi.DBG_NITEMS, nch)
    ntoks = comp.debug(_capi.DBG_NTOK, nch)
    plan = comp.debug(_capi.DBG_PLAN, nch)
    lens = comp.debug(_capi.DBG_LENS, nch)
    seen = {"coded": 0, "skipped_coded": 0}
    for c, data in enumerate(chunks):
        btype, hbits, ntok = int(plan[c, 0]), int(plan[c, 2]), int(ntoks[c])
        nit, skipped = int(nitems[c]) & ~SKIPPED, bool(int(nitems[c]) & SKIPPED)
        # a region with data starts a token (every 1024th position does): its count of tokens before is below the chunk's
        live = np.array([r * W.REGION < data.size and ntok > 0 for r in range(REGIONS)])
        if btype != 0:
            assert np.array_equal(sub[c, :, 1] < ntok, live), c
        if btype == 0 and skipped:
            # stored, its items never written: the table is the fast path's (an item is a position), or all zero (no tokens)
            assert np.array_equal(ritem[c], np.minimum(np.arange(REGIONS) * W.REGION, nit)), c
            continue
        it = items[c, :nit].astype(np.uint32)
        for r in np.flatnonzero(live):
            e = int(it[ritem[c, r]])
            assert e & 0xC000 == 0xC000 and (e >> 9) & 31 == r, (c, r, hex(e))
        assert np.all(ritem[c, ~live] == nit), c
        assert int(np.count_nonzero((it & 0xC000) == 0xC000)) == int(live.sum()), c
        if btype == 0:
            assert not sub[c].any(), c
            continue
        seen["coded"] += 1
        if skipped:  # k_emit wrote the items itself: every position a literal
            seen["skipped_coded"] += 1
            tokens = data.astype(np.uint32)
            assert np.array_equal(it & 0xFF, tokens) and nit == ntok == data.size, c
        else:
            start = (it & 0x8000) != 0
            head = start & ((it & 0x0100) != 0)
            nxt = np.append(it[1:], np.uint32(0))
            tokens = np.where(head, np.uint32(W.MATCH) | ((it & 0xFF) << 16) | (nxt & 0x7FFF), it & 0xFF)[start].astype(np.uint32)
            assert tokens.size == ntok, c
        ll, dl = (FIXED_LL, FIXED_D) if btype == 1 else (lens[c, :286].tolist(), lens[c, 288:318].tolist())
        assert np.array_equal(sub[c].astype(np.int64), _writer_subindex(tokens, ll, dl, hbits)), c
    return seen


def _check_single(comp, data, strategy="auto"):
    got = comp.compress(data, strategy=strategy)
    idx, sub = comp.last_index(), comp.last_subindex()
    seen = _check_tables(comp, _chunks_of(data), sub)
    _, widx, wsub = O.compress_indexed(data, O.default_params(strategy=_capi.STRATEGY[strategy], fast_skip=1))
    assert np.array_equal(idx, widx) and np.array_equal(sub, wsub), strategy
    out, st = comp.decompress(got, idx, data.size, subindex=sub, block_bytes=comp.last_block_bytes())
    assert st == 0 and out == data.tobytes(), strategy
    return seen


def test_text_one_byte_last_chunk(comp):
    """64 KiB + 1 of text: three chunks, the last of one byte, all of whose regions but the first lie past the data"""
    seen = _check_single(comp, synth.gen_text(2 * CHUNK + 1, seed=7))
    assert seen["coded"] == 3


@pytest.mark.parametrize("kind", ["zeros", "line61"])
def test_many_starts_in_one_wave(comp, kind):
    """96 KiB of long matches: a chunk is a few hundred items, fewer than one batch, and one wave's 512 items hold many
    region starts"""
    data = np.zeros(3 * CHUNK, np.uint8) if kind == "zeros" else _line61(3 * CHUNK)
    seen = _check_single(comp, data)
    assert seen["coded"] == 3
    comp.compress(data)  # (the decode replaced the context's state)
    nit = comp.debug(_capi.DBG_NITEMS, 3)
    assert np.all(nit < 4096), nit


def test_items_written_by_emit(comp):
    """64 KiB of six-bit random bytes: the stored fast path is taken, the chunks are coded, k_emit writes the items"""
    seen = _check_single(comp, _six_bit(2 * CHUNK))
    assert seen["coded"] == 2 and seen["skipped_coded"] == 2


def test_batch_call(comp):
    """a batch of four items, 0, 700, 32768 and 70000 bytes: six chunks in one launch"""
    text = synth.gen_text(70000, seed=8)
    datas = [text[:0], text[:700], text[1000: 1000 + CHUNK], text]
    streams = comp.compress_batch(datas)
    idx, sub, bb = comp.last_batch_index()
    chunks = [ch for d in datas for ch in _chunks_of(d)]
    assert len(chunks) == 6
    sub = np.asarray(sub).reshape(len(chunks), REGIONS, 2)
    seen = _check_tables(comp, chunks, sub)
    assert seen["coded"] >= 5
    wsub = [O.compress_indexed(d, O.default_params(fast_skip=1))[2].ravel() for d in datas]
    assert np.array_equal(sub.ravel(), np.concatenate(wsub))
    outs, sts = comp.decompress_batch(streams, [d.size for d in datas], idx, sub.ravel(), bb)
    assert sts == [0] * 4 and all(o == d.tobytes() for o, d in zip(outs, datas))


@pytest.mark.parametrize("strategy", ["fixed", "dynamic"])
def test_forced_strategy_stage(comp, strategy):
    """the 64 KiB + 1 of text with the strategy forced: k_emit's 9392-word stage"""
    seen = _check_single(comp, synth.gen_text(2 * CHUNK + 1, seed=7), strategy)
    assert seen["coded"] == 3
