"""k_emit's paths: the small stage (strategy auto) at its bound, the big stage (forced fixed / dynamic) on the single and the
batch calls, chunks whose items k_emit writes itself (the stored fast path, chunk not stored), partial last batches of items,
and the sub-index on data with many long matches.  Every stream is bit-exact against the encoder specification (the oracle)
and decodes with zlib, the oracle's decoder and the GPU decoder (with the sub-index)."""
import zlib

import numpy as np
import pytest

import oracle_lib as O
from starflate_amd import Compressor, _capi, synth

pytestmark = pytest.mark.gpu

CHUNK = 32768


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


def _params(strategy="auto", stored_fast_path=True):
    return O.default_params(strategy=_capi.STRATEGY[strategy], fast_skip=int(stored_fast_path))


def _near_stored(n, seed=11):
    """bytes whose dynamic literal block is a few dozen bytes under the stored block (7.99 bits per byte, no repeats)"""
    pw = np.ones(256)
    pw[:64] = 0.5
    return np.random.default_rng(seed).choice(256, size=n, p=pw / pw.sum()).astype(np.uint8)


def _noise_with_repeats(n, seed=12):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, n, dtype=np.uint8)
    for k in range(0, n - 200, 4096):  # a short repeat every 4 KiB
        d[k + 100: k + 140] = d[k: k + 40]
    return d


def _runs(n, seed=9):
    """half zeros, half one 61-byte line repeated (bench.py's runs workload)"""
    line = np.random.default_rng(seed).integers(32, 127, 61, dtype=np.uint8)
    d = np.zeros(n, np.uint8)
    d[n // 2:] = np.tile(line, (n - n // 2) // 61 + 1)[: n - n // 2]
    return d


def _check_single(comp, data, strategy="auto", stored_fast_path=True):
    """stream, index and sub-index == the specification's; the stream decodes with zlib, the oracle and the GPU decoder"""
    got = comp.compress(data, strategy=strategy, stored_fast_path=stored_fast_path)
    want, widx, wsub = O.compress_indexed(data, _params(strategy, stored_fast_path))
    assert np.array_equal(np.frombuffer(got, np.uint8), want), (data.size, strategy)
    idx, sub = comp.last_index(), comp.last_subindex()
    assert np.array_equal(idx, widx) and np.array_equal(sub, wsub), (data.size, strategy)
    assert zlib.decompress(got, -15) == data.tobytes()
    st, w, back = O.decompress(np.frombuffer(got, np.uint8), data.size)
    assert st == 0 and w == data.size and np.array_equal(back, data)
    out, st = comp.decompress(got, idx, data.size, subindex=sub, block_bytes=comp.last_block_bytes())
    assert st == 0 and out == data.tobytes()
    return np.frombuffer(got, np.uint8), idx


def _chunks(stream, idx):
    """(block type, bytes) of every chunk of a single-call stream"""
    return [((int(stream[int(a)]) >> 1) & 3, int(b) - int(a)) for a, b in zip(idx[:-1], idx[1:])]


def test_auto_largest_coded_chunk(comp):
    """strategy auto: dynamic blocks just under their stored size fill the small stage to within a few dozen bytes"""
    for data in (_near_stored(4 * CHUNK + 5000), _noise_with_repeats(3 * CHUNK + 77)):
        for fast in (True, False):
            stream, idx = _check_single(comp, data, "auto", fast)
    blocks = _chunks(*_check_single(comp, _near_stored(4 * CHUNK), "auto"))
    assert all(bt == 2 and CHUNK - 64 < n < CHUNK + 5 for bt, n in blocks), blocks


@pytest.mark.parametrize("strategy", ["fixed", "dynamic"])
def test_forced_strategies_single(comp, strategy):
    """forced fixed / dynamic (the big stage): noise codes to more than its stored size"""
    noise = synth.gen_random(3 * CHUNK + 999, seed=3)
    text = synth.gen_text(5 * CHUNK + 4321, seed=6)
    for data in (noise, text):
        for fast in (True, False):
            stream, idx = _check_single(comp, data, strategy, fast)
    blocks = _chunks(*_check_single(comp, noise[: 3 * CHUNK], strategy))
    assert all(bt == (1 if strategy == "fixed" else 2) and n > CHUNK + 5 for bt, n in blocks), blocks


def _check_batch(comp, items, container="raw", **opt):
    streams = comp.compress_batch(items, container=container, **opt)
    hdr, tr = {"raw": (0, 0), "zlib": (2, 4), "gzip": (10, 8)}[container]
    wbits = {"raw": -15, "zlib": 15, "gzip": 31}[container]
    idx, sub, bb = comp.last_batch_index()
    wsubs = []
    for i, (data, got) in enumerate(zip(items, streams)):
        assert got == comp.compress(data, container=container, **opt), i
        want, _, wsub = O.compress_indexed(data, _params(opt.get("strategy", "auto"), opt.get("stored_fast_path", True)))
        assert np.array_equal(np.frombuffer(got[hdr: len(got) - tr], np.uint8), want), i
        assert zlib.decompress(got, wbits) == data.tobytes(), i
        wsubs.append(wsub.ravel())
    assert np.array_equal(sub, np.concatenate(wsubs))
    outs, sts = comp.decompress_batch(streams, [d.size for d in items], idx, sub, bb, container=container)
    assert sts == [0] * len(items) and all(o == d.tobytes() for o, d in zip(outs, items))


@pytest.mark.parametrize("strategy", ["fixed", "dynamic"])
def test_forced_strategies_batch(comp, strategy):
    items = [synth.gen_random(2 * CHUNK + 5, seed=1), synth.gen_text(3 * CHUNK + 100, seed=2), np.zeros(777, np.uint8),
             _near_stored(CHUNK + 17)]
    _check_batch(comp, items, strategy=strategy)


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
def test_batch_containers(comp, container):
    items = [synth.gen_text(5 * CHUNK + 321, seed=4), _near_stored(2 * CHUNK), _runs(3 * CHUNK + 1000), np.zeros(0, np.uint8),
             synth.gen_mixed(1 << 20, seed=3, stripe=1 << 16)[: 300_001]]
    _check_batch(comp, items, container=container)


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]
FIXED_LENS = np.array([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8 + [5] * 32, np.uint32)


def _host_subindex(comp, nch):
    """every coded chunk's sub-index bit offsets, recomputed by walking its tokens with its code lengths: a flagged region's
    entry is the bit offset of its first token from the chunk's first byte, a region past the data the end-of-block code's"""
    toks, flags = comp.debug_tokens(nch)
    plan = comp.debug(_capi.DBG_PLAN, nch)
    lens = comp.debug(_capi.DBG_LENS, nch).astype(np.uint32)
    want = np.zeros((nch, 32), np.uint32)
    for c in range(nch):
        btype, hbits = int(plan[c, 0]), int(plan[c, 2])
        if btype == 0:
            continue
        ln = FIXED_LENS if btype == 1 else lens[c]
        cost = np.empty(toks[c].size, np.int64)
        for k, t in enumerate(toks[c].tolist()):
            if t & 0x80000000:
                L, D = ((t >> 16) & 0xFF) + 3, (t & 0x7FFF) + 1
                ls, ds = np.searchsorted(LBASE, L, "right") - 1, np.searchsorted(DBASE, D, "right") - 1
                cost[k] = ln[257 + ls] + LEXT[ls] + ln[288 + ds] + DEXT[ds]
            else:
                cost[k] = ln[t]
        before = hbits + np.concatenate([[0], np.cumsum(cost)])
        want[c, :] = before[-1]
        for k, r in flags[c]:
            want[c, r] = before[k]
    return want


def test_region_starts_on_long_matches(comp):
    """zero pages and long runs, four 258-byte matches or more per 1024-byte region: every region's sub-index entry against
    the specification and against the offsets recomputed on the host from the tokens.  No lane's eight items hold two region
    starts: every 1024th position starts a token of at most 258 bytes and two items, so flagged items are 8 or more apart and
    k_emit's item walk (a lane with two starts) is not reached"""
    for data in (np.zeros(4 * CHUNK + 123, np.uint8), _runs(6 * CHUNK + 4000),
                 np.tile(np.frombuffer(b"0123456789abcdef" * 20 + b"x", np.uint8), 900), synth.gen_text(3 * CHUNK + 99, seed=5)):
        nch = (data.size + CHUNK - 1) // CHUNK
        for strategy in ("auto", "fixed", "dynamic"):
            _check_single(comp, data, strategy, stored_fast_path=False)
            comp.compress(data, strategy=strategy, stored_fast_path=False)  # (the GPU decode above replaced the context's index)
            sub = comp.last_subindex()
            plan = comp.debug(_capi.DBG_PLAN, nch)
            coded = plan[:, 0] != 0
            assert coded.any()
            assert np.array_equal(sub[coded, :, 0], _host_subindex(comp, nch)[coded]), strategy
            items = comp.debug(_capi.DBG_ITEMS, nch)
            nit = comp.debug(_capi.DBG_NITEMS, nch)
            for c in range(nch):
                it = items[c, : nit[c]]
                at = np.flatnonzero((it & 0xC000) == 0xC000)
                assert at.size == min(32, (min(CHUNK, data.size - c * CHUNK) + 1023) // 1024), (c, at.size)
                assert np.all(np.diff(at // 8) > 0), (strategy, c)  # at most one region start per eight aligned items


def test_items_written_by_emit(comp):
    """the stored fast path taken and the chunk NOT stored: k_emit writes the chunk's items itself (kItemsSkipped)"""
    for data in (_near_stored(3 * CHUNK + 5), synth.gen_random(2 * CHUNK + 3000, seed=8)):
        for strategy in ("auto", "fixed", "dynamic"):
            _check_single(comp, data, strategy, stored_fast_path=True)


def test_partial_last_batches(comp):
    """chunks whose item count is not a multiple of 4096 (a partial last batch), down to a single item"""
    text = synth.gen_text(CHUNK * 4, seed=13)
    for n in (1, 2, 7, 4095, 4097, 8191, 12289, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 4095):
        for strategy in ("auto", "dynamic"):
            _check_single(comp, text[:n], strategy)
