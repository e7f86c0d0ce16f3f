"""k_plan's symbol sort and canonical codes at the shapes where they can go wrong (round 11).

The sort of the literal/length alphabet has two paths -- up to 64 used symbols are compacted to one per lane, more are ranked
group by group with the empty groups left out -- and canonical_codes counts a code's lengths in 8-bit fields per 16-lane
row.  The cases below sit on those seams: 1, 2, 63, 64, 65, 128, 129 and 285 used literal/length symbols, symbols in groups
0 and 4 only, per-length counts of 255 and 256 (past a field, across rows), lengths clamped at 15 with Kraft repair, a
distance alphabet of 0, 1, 2 and 30 symbols, a code-length code of all 19 symbols and one of 2.  (285, not 286: the
specification's shortest match is 4 bytes, so no token has length symbol 257; 285 is every symbol a chunk's tokens can
use.  256 literals of equal count and the end-of-block symbol give 255 codes of 8 bits, a full field; `one_length_256` is
the case that passes it.)

Every case is one to four chunks (at most 128 KiB) compressed in 32 KiB blocks, so every chunk stands alone.  For every
chunk: lengths and plan against the oracle's plan of the chunk's own DBG_HIST, the stream against the oracle's bit for bit,
a zlib round trip; under all four strategies (forced fixed runs the 288- and 32-symbol canonical codes on the fixed
lengths), and once through the batch call.  Each case asserts FROM THE GPU'S HISTOGRAM that it hit its class; the first
test, which needs no GPU, asserts the same from the oracle's tokens, which is how the generators were chosen."""
import functools
import zlib

import numpy as np
import pytest

import deflate_writer as W
import oracle_lib as O
from starflate_amd import _capi
from test_code_limits import CHUNK, chunk_histograms, cl_items, deep_input, oracle_params, unconstrained

STRATEGIES = (("auto", 0), ("stored", 1), ("fixed", 2), ("dynamic", 3))
BLOCK = 32768


# ---- generators: bytes whose tokens (one chunk each, no carried window) land in a class ----

def once_each(values, seed):
    """every value once, shuffled: no byte repeats, so no match -- len(values) literals and the end-of-block symbol"""
    a = np.array(sorted(values), np.uint8)
    np.random.default_rng(seed).shuffle(a)
    return a


def spread(k, seed):
    """k byte values over all four literal groups"""
    return np.random.default_rng(seed).permutation(256)[:k].tolist()


def with_copies(prefix, copies, seed, pad_below=256):
    """prefix, then for every (offset, length) a copy of prefix[offset: offset + length]; every copy lies at the start of a
    512-byte parse region of its own, behind random bytes below pad_below, so that none is cut"""
    rng = np.random.default_rng(seed)
    out = list(prefix)
    for off, length in copies:
        while len(out) % 512 != 8:
            out.append(int(rng.integers(0, pad_below)))
        out += list(prefix[off: off + length])
    return np.array(out, np.uint8)


def every_symbol(seed=7):
    """all 256 literals, all 29 length symbols: 286 used literal/length symbols"""
    rng = np.random.default_rng(seed)
    out = rng.permutation(256).tolist()
    for k, length in enumerate(W.LEN_BASE):  # a run of length + 1 equal bytes: a literal and a match of `length` at distance 1
        while len(out) % 512 != 8:
            out.append(int(rng.integers(0, 256)))
        v = (out[-1] + 1 + k) % 256
        out += [v] * (length + 1) + [(v + 101) % 256]
    return np.array(out, np.uint8)


def one_length_past_a_field():
    """'a' at every other place, 255 other values once each: 'a' gets 1 bit and 255 literals and the end-of-block symbol 9
    bits -- 256 codes of one length"""
    a = np.full(510, 97, np.uint8)
    a[1::2] = [v for v in range(256) if v != 97]
    return a


def equal_literals(seed=3):
    """256 literals of equal count and the end-of-block symbol: 255 codes of 8 bits, lanes of every row"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.permutation(256), rng.permutation(256)]).astype(np.uint8)


def planted_distances(counts, seed, long_copy=0):
    """random bytes with 5-byte copies planted counts[c] times at a distance of code c, each from a place whose bytes occur
    nowhere else so far (no nearer and no longer match than the planted one) and inside one 512-byte parse region;
    long_copy: one more copy of that many bytes"""
    rng = np.random.default_rng(seed)
    plan = np.array([c for c, k in enumerate(counts) for _ in range(k)])
    rng.shuffle(plan)
    plan = sorted(plan.tolist(), key=lambda c: W.DIST_BASE[c] >= 2048)  # the far ones last, when their sources exist
    out, seen = [], {}

    def push(b):
        out.append(int(b))
        if len(out) >= 4:
            g = bytes(out[-4:])
            seen[g] = seen.get(g, 0) + 1

    for _ in range(1100):
        push(rng.integers(0, 256))
    for c in plan:
        while True:
            push(rng.integers(0, 256))
            pos = len(out)
            if pos % 512 > 500 or pos < W.DIST_BASE[c] + 8:
                continue
            d = W.DIST_BASE[c] + int(rng.integers(0, min(1 << W.DIST_EXTRA[c], pos - W.DIST_BASE[c] - 4)))
            q = pos - d
            if d < 5 or seen[bytes(out[q: q + 4])] != 1 or seen[bytes(out[q + 1: q + 5])] != 1:
                continue
            for k in range(5):
                push(out[q + k])
            push((out[q + 5] + 1 + int(rng.integers(0, 255))) % 256)  # (the copy ends here)
            break
    if long_copy:
        while len(out) % 512 != 8:
            push(rng.integers(0, 256))
        for k in range(long_copy):
            push(out[40 + k])
    assert len(out) <= CHUNK
    return np.array(out, np.uint8)


def all_distance_codes(seed=5):
    """a 5-byte copy at a distance of every one of the 26 distance codes from 5 bytes on, and runs / periods of 1 to 4 bytes
    for the four nearest"""
    a = planted_distances([0] * 4 + [2] * 26, seed).tolist()
    rng = np.random.default_rng(seed)
    for d in (1, 2, 3, 4):
        while len(a) % 512 != 8:
            a.append(int(rng.integers(0, 256)))
        unit = [(a[-1] + 1 + 7 * k) % 256 for k in range(d)]
        a += (unit * 12)[:d + 9]
    assert len(a) <= CHUNK
    return np.array(a, np.uint8)


def every_code_length_symbol(seed=1):
    """distance codes 4..18 at Fibonacci counts 1, 2, 3 .. 987 and one far copy: the distance code has every length 1..15 (15
    twice).  The
    literal/length code sends runs of equal lengths (16), the lone unused symbol 257 (a single 0), the unused distance codes
    0..3 (17), and, with one long copy, eleven or more unused length symbols in a row (18)"""
    fib = [1, 1]
    while len(fib) < 16:
        fib.append(fib[-1] + fib[-2])
    return planted_distances([0] * 4 + fib[1:] + [0] * 11, seed, long_copy=100)


def two_symbol_code_length_code():
    """127 literals once each at values whose gaps are one or two unused values (runs of at most three used ones): all 128
    codes are 7 bits, the unused values are sent as single zeros, there is no distance code: the code-length code has the
    two symbols 0 and 7"""
    return once_each(list(range(0, 252, 2)) + [253], 1)


NAMES = ("m1_empty", "m2", "m63", "m64", "m65", "m128", "m129", "m285_every_symbol", "groups_0_4_small", "groups_0_4_large", "equal_literals",
         "one_length_256", "d1", "d2", "d30", "cl_2", "deep", "cl_19")


@functools.lru_cache(maxsize=1)
def cases():
    """-> {name: (bytes, class predicate on (ll, d) histograms of chunk 0 .. [, chunk])}"""
    def m_is(m, md=0):
        return lambda ll, d: np.count_nonzero(ll) == m and np.count_nonzero(d) == md

    def cl_used(ll, d):
        p = oracle_params(3, BLOCK)
        pl = O.plan_chunk(ll, d, CHUNK, True, p)
        return {s for s, _ in cl_items(np.frombuffer(pl.ll_lens, np.uint8)[:286], np.frombuffer(pl.d_lens, np.uint8)[:30])}

    def lens_of(ll, d):
        pl = O.plan_chunk(ll, d, CHUNK, True, oracle_params(3, BLOCK))
        return np.frombuffer(pl.ll_lens, np.uint8)[:286].astype(np.int64)

    out = {
        "m1_empty": (np.zeros(0, np.uint8), m_is(1)),
        "m2": (np.array([65], np.uint8), m_is(2)),
        "m63": (once_each(spread(62, 63), 0), m_is(63)),
        "m64": (once_each(spread(63, 64), 0), m_is(64)),
        "m65": (once_each(spread(64, 65), 0), m_is(65)),
        "m128": (once_each(spread(127, 128), 0), m_is(128)),
        "m129": (once_each(spread(128, 129), 0), m_is(129)),
        "m285_every_symbol": (every_symbol(), lambda ll, d: np.count_nonzero(ll) == 285 and ll[257] == 0),
        # groups 0 and 4 with empty groups between: compacted (m <= 64), and ranked group by group (m > 64)
        "groups_0_4_small": (once_each(range(5, 45), 2), lambda ll, d: np.count_nonzero(ll) == 41 and not ll[64:256].any()),
        "groups_0_4_large": (with_copies(once_each(range(64), 4), [(3, 4), (8, 5), (14, 6), (21, 20)], 4, pad_below=64),
                             lambda ll, d: np.count_nonzero(ll) > 64 and not ll[64:256].any() and ll[:64].all()),
        "equal_literals": (equal_literals(), lambda ll, d: (ll[:256] == ll[0]).all() and ll[0] > 0 and ll[256] == 1 and not ll[257:].any()
                           and np.bincount(lens_of(ll, d), minlength=16)[8] == 255),
        "one_length_256": (one_length_past_a_field(), lambda ll, d: np.bincount(lens_of(ll, d), minlength=16)[9] == 256),
        "d1": (with_copies(once_each(range(100, 140), 6), [(0, 8)], 6), lambda ll, d: np.count_nonzero(d) == 1),
        "d2": (with_copies(once_each(range(100, 140), 6), [(0, 8), (20, 8)], 6), lambda ll, d: np.count_nonzero(d) == 2),
        "d30": (all_distance_codes(), lambda ll, d: np.count_nonzero(d) == 30),
        "cl_2": (two_symbol_code_length_code(), lambda ll, d: cl_used(ll, d) == {0, 7}),
    }
    data, deep = deep_input()  # [0] distance tree 16 deep, [1] literal/length tree 17 deep, [3] code-length code deeper than 7
    out["deep"] = (data, lambda ll, d: unconstrained(ll, d)[0] > 15, deep["ll"])
    out["cl_19"] = (every_code_length_symbol(), lambda ll, d: cl_used(ll, d) == set(range(19)))
    assert tuple(out) == NAMES
    return out


def nchunks(data):
    return max(1, (data.size + CHUNK - 1) // CHUNK)


def assert_class(name, hists):
    entry = cases()[name]
    ll, d = hists[entry[2] if len(entry) > 2 else 0]
    assert entry[1](np.asarray(ll[:286], np.int64), np.asarray(d[:30], np.int64)), f"{name}: the input no longer hits its class"


@pytest.mark.parametrize("name", NAMES)
def test_generators_hit_their_classes(name):
    """on the CPU, from the oracle's tokens: every generator lands in the class it is named for"""
    data = cases()[name][0]
    assert 1 <= nchunks(data) <= 4 and data.size <= 131072
    assert_class(name, chunk_histograms(data, oracle_params(3, BLOCK)))


def check_chunks(compressor, name, data, strategy):
    p = oracle_params(strategy, BLOCK)
    nch = nchunks(data)
    hist = compressor.debug(_capi.DBG_HIST, nch)
    lens = compressor.debug(_capi.DBG_LENS, nch)
    plan = compressor.debug(_capi.DBG_PLAN, nch)
    assert_class(name, [(hist[c, :286], hist[c, 288:318]) for c in range(nch)])
    for c in range(nch):
        ll, dd = hist[c, :286], hist[c, 288:318]
        pl = O.plan_chunk(ll, dd, min(CHUNK, data.size - c * CHUNK), c + 1 == nch, p)
        assert plan[c, 0] == pl.btype and plan[c, 1] == pl.out_bytes, (name, c, "plan")
        assert np.array_equal(lens[c, :288], np.frombuffer(pl.ll_lens, np.uint8)), (name, c, "ll lens")
        assert np.array_equal(lens[c, 288:320], np.frombuffer(pl.d_lens, np.uint8)), (name, c, "d lens")


@pytest.mark.gpu
@pytest.mark.parametrize("strategy_name,strategy", STRATEGIES)
def test_plan_codes_at_the_seams(compressor, strategy_name, strategy):
    for name, entry in cases().items():
        data = entry[0]
        got = np.frombuffer(compressor.compress(data, strategy=strategy_name, stored_fast_path=False, block_bytes=BLOCK, effort="best"), np.uint8)
        check_chunks(compressor, name, data, strategy)
        want = O.compress(data, oracle_params(strategy, BLOCK))
        assert got.size == want.size and np.array_equal(got, want), (name, strategy_name)
        assert zlib.decompress(got.tobytes(), -15) == data.tobytes(), (name, strategy_name)


@pytest.mark.gpu
def test_plan_codes_through_the_batch_call(compressor):
    """k_plan takes a chunk's bytes and BFINAL from the chunk table: the same cases, one item each, in one call"""
    names = [n for n in NAMES if cases()[n][0].size]  # (an item of no bytes is not a batch item)
    items = [cases()[n][0] for n in names]
    outs = compressor.compress_batch(items, strategy="dynamic", stored_fast_path=False, block_bytes=BLOCK, effort="best")
    for name, item, out in zip(names, items, outs):
        want = O.compress(item, oracle_params(3, BLOCK))
        assert np.array_equal(np.frombuffer(out, np.uint8), want), name
        assert zlib.decompress(out, -15) == item.tobytes(), name
