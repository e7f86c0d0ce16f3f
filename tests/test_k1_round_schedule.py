"""k_lz77's round schedule.  What a round does is fixed by the specification; WHEN the kernel does it is not: the window's
shift, the store of the next round's bytes and the table's ageing run in the round before, behind its parse; a variant in which
half of the workgroup starts a round's parse while the other half still finishes its last match step was measured and left out
(profiles/r09_notes.md), and the cases that would catch it stay.  Whatever the order, the
stream is the specification's, bit for bit.  The inputs put something observable at every place such a reordering can break:

far    a text of 3 * 8192 + 5 bytes three times over, so every match of the later copies lies 24,581 bytes back -- three
       rounds and five bytes: a window shifted twice, not at all, or under a wave that is still extending finds other bytes
       there.  The first 24 bytes of every round but the first are noise of the upper half of the byte range, which the text
       never has: the round's first token is a literal, coded from the very bytes that the look-ahead's shift overwrites.
mix    far's first chunk, a chunk of noise, then far again: the stored fast path, the window loaded again behind it, the
       short probe of the next chunk, and a strip whose last round is 15 bytes.
short  far cut to one round and two rounds plus the look-ahead (give or take a byte), and to three rounds plus 1..7 steps of
       1024 and seven bytes: last rounds of every step count, odd and even (the last one all eight steps of a round that is
       seventeen bytes short), where a head start of the parse must fall back or cope.

The specification's side is checked alone first, on the CPU: every stream round-trips through the oracle's decoder and `far`
has the tokens this docstring says it has, so a GPU failure here can only be the kernel's."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from starflate_amd import synth
from test_gpu_parity import EFFORT_PARAMS, _params

CHUNK = 32768   # kChunk: a DEFLATE block, four rounds
ROUND = 8192    # kRound
REGION = 512    # a wave's parse region
BACK = 3 * ROUND + 5  # how far back far's copies lie

EFFORTS = ("default", "fast", "fastest", "thorough", "max", "recent", "recent_all", "best", "ultra", "extreme")
ORACLE_CHECKED = ("default", "fast", "fastest", "thorough", "max", "recent", "best")
SHORT = (ROUND + 32, 2 * ROUND + 31, 2 * ROUND + 33) + tuple(3 * ROUND + 1024 * k + 7 for k in range(1, 8))
BATCH_BB = 8 * CHUNK


@functools.lru_cache(maxsize=None)
def _far_and_noise():
    base = synth.gen_text(4 * 65536, seed=47)[:BACK]
    far = np.tile(base, 3)[: 9 * ROUND + 40].copy()
    rng = np.random.default_rng(5)
    for r in range(1, -(-far.size // ROUND)):
        far[r * ROUND: r * ROUND + 24] = rng.integers(128, 256, 24, dtype=np.uint8)[: far.size - r * ROUND]
    noise = rng.integers(0, 256, CHUNK, dtype=np.uint8)
    far.setflags(write=False)
    return far, noise


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (bytes, block_bytes): one strip each."""
    far, noise = _far_and_noise()
    cases = {"far": (far, 4 * CHUNK),
             "mix": (np.concatenate([far[:CHUNK], noise, far[CHUNK: CHUNK + 2 * CHUNK + ROUND + 13]]), 8 * CHUNK)}  # (to far's end)
    for n in SHORT:
        cases[f"short{n}"] = (far[:n], -(-n // CHUNK) * CHUNK)
    return cases


def _oracle_params(effort, bb):
    p = _params(block_bytes=bb)
    for k, v in EFFORT_PARAMS[effort].items():
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def _want(name, effort, bb=None):
    """The specification's stream for a case (computed once, shared by the tests, never written to)."""
    data, own = _cases()[name]
    want = O.compress(data, _oracle_params(effort, bb or own))
    want.setflags(write=False)
    return want


def test_cases_are_what_the_docstring_says():
    assert sorted(EFFORTS) == sorted(EFFORT_PARAMS) and set(ORACLE_CHECKED) <= set(EFFORTS)
    far, bb = _cases()["far"]
    assert far.size == 3 * BACK and far.size // ROUND == 9 and bb == 4 * CHUNK and far.size <= bb  # (the cut is past three copies)
    assert np.array_equal(far[BACK + 24: 4 * ROUND], far[24: ROUND - 5])  # a copy lies BACK behind (between the noise blocks)
    mix, bbm = _cases()["mix"]
    assert mix.size == 106511 and mix.size % ROUND == 15 and bbm == 8 * CHUNK
    assert len(SHORT) == 10 and sorted({-(-(n % ROUND) // 1024) for n in SHORT}) == [1, 2, 3, 4, 5, 6, 7, 8]  # steps of 1024 in the last round
    for data, b in _cases().values():
        assert data.dtype == np.uint8 and b % CHUNK == 0 and data.size <= b


@pytest.mark.parametrize("effort", ORACLE_CHECKED)
def test_far_has_a_literal_first_and_far_matches_in_every_round(effort):
    """In every full round from the fourth on: the first token is a literal, and the round's first region has two matches
    of more than 32 bytes from more than 24,576 bytes back."""
    far, bb = _cases()["far"]
    toks, nt = O.strip_tokens(far, _oracle_params(effort, bb))
    for r in range(3, far.size // ROUND):
        g = r * ROUND // REGION
        t = toks[g * REGION: g * REGION + nt[g]]
        assert nt[g] and not (t[0] & 0x80000000), (effort, r)
        m = t[(t & 0x80000000) != 0]
        long_far = (((m >> 16) & 0xFF) + 3 > 32) & ((m & 0x7FFF) + 1 > 24576)
        assert np.count_nonzero(long_far) >= 2 and np.all((m[long_far] & 0x7FFF) + 1 == BACK), (effort, r)


@pytest.mark.parametrize("effort", EFFORTS)
def test_oracle_streams_round_trip(effort):
    for name, (data, _) in _cases().items():
        st, w, back = O.decompress(_want(name, effort), data.size)
        assert st == 0 and w == data.size and np.array_equal(back, data), (name, effort)


@pytest.mark.gpu
@pytest.mark.parametrize("effort", EFFORTS)
def test_round_schedule_bit_exact_vs_oracle(compressor, effort):
    for name, (data, bb) in _cases().items():
        got = np.frombuffer(compressor.compress(data, effort=effort, block_bytes=bb), np.uint8)
        want = _want(name, effort)
        assert got.size == want.size, f"{name}/{effort}: size {got.size} != {want.size}"
        assert np.array_equal(got, want), f"{name}/{effort}: first diff at {np.flatnonzero(got != want)[:4]}"


@pytest.mark.gpu
@pytest.mark.parametrize("effort", EFFORTS)
def test_batch_equals_single_calls(compressor, effort):
    """far, mix and two short strips in one batch call (the batch kernels are instantiations of their own)."""
    names = ("far", "mix", f"short{SHORT[1]}", f"short{SHORT[6]}")
    items = [_cases()[k][0] for k in names]
    streams = compressor.compress_batch(items, effort=effort, block_bytes=BATCH_BB)
    for name, data, s in zip(names, items, streams):
        got = np.frombuffer(s, np.uint8)
        single = np.frombuffer(compressor.compress(data, effort=effort, block_bytes=BATCH_BB), np.uint8)
        assert np.array_equal(got, single), f"{name}/{effort}: batch differs from the single call"
        assert np.array_equal(got, _want(name, effort, BATCH_BB)), f"{name}/{effort}: batch differs from the oracle"
