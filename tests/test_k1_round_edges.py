"""k_lz77 at the ends of a strip.  A round's bytes are prefetched a round ahead, eight per thread, by two `load4`: one
dword load each where the word lies inside the strip (pos + 4 <= n), byte by byte with zeros beyond the end where it does
not.  A strip's last round is short, so the match loop runs fewer steps there (nsteps = ceil(qn / step), odd or even), and the
loop takes a wave's intervals in PAIRS: the half of the workgroup that starts an interval late, the pair that ends at
nsteps and the pair that does not must all pass the same barriers.  Strip lengths around one round, two rounds and a chunk,
each plus the look-ahead, give or take up to nine bytes, put the strip's end on every side of a thread's two words and
of a step's first position; each must give the specification's stream bit for bit, for every kernel class (step tables
at stride 2 with two levels and with one, every position, the two tables of `max`, whose match loop alone still takes
its intervals one at a time, exact recency at stride 2 and at every position, hash chains of depth 8, 16 and 32).

(History: a variant that fetched the prefetch with one unguarded 8-byte load behind a uniform test
rb + 2 * kRound + kLook <= n was measured and left out, profiles/r08_notes.md; the lengths bracket that bound too.)

The specification's side is checked alone first, on the CPU: every input round-trips through the oracle's decoder, so a
GPU failure here can only be the kernel's."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from starflate_amd import synth
from test_gpu_parity import EFFORT_PARAMS, _params

CHUNK = 32768   # kChunk: a DEFLATE block, four rounds
ROUND = 8192    # kRound: positions per round, eight per thread
LOOK = 32       # kLook: the bytes behind a round that its matches may read

EFFORTS = ("default", "fast", "fastest", "thorough", "max", "recent", "recent_all", "best", "ultra", "extreme")
DELTAS = (-9, -8, -5, -4, -1, 0, 1, 3, 4, 7, 8)
LENGTHS = sorted({base + d for base in (ROUND + LOOK, 2 * ROUND + LOOK, CHUNK + LOOK) for d in DELTAS}
                 | {ROUND - 1, ROUND, ROUND + 1, LOOK + 8 * 1024 - 4})


@functools.lru_cache(maxsize=None)
def _text():
    return synth.gen_text(4 * 65536, seed=31)


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (bytes, block_bytes).  One strip per input (block_bytes >= n, a multiple of 32 KiB) except where said."""
    text = _text()
    cases = {f"n{n}": (text[:n], max(CHUNK, -(-n // CHUNK) * CHUNK)) for n in LENGTHS}
    # several strips of 64 KiB, the last one 32 KiB + 5 bytes: after two full strips, and after three
    cases["strips3"] = (text[: 2 * 65536 + CHUNK + 5], 65536)
    cases["strips4"] = (text[: 3 * 65536 + CHUNK + 5], 65536)
    # a chunk of noise, then text, in one strip: the chunk takes the stored fast path, so the window is loaded again and the
    # next chunk's probe is short right where the strip ends 13 bytes into a round
    noise = np.random.default_rng(83).integers(0, 256, CHUNK, dtype=np.uint8)
    cases["noise_text"] = (np.concatenate([noise, text[: 2 * CHUNK + 13]]), 4 * CHUNK)
    return cases


@functools.lru_cache(maxsize=None)
def _want(name, effort):
    """The specification's stream for a case (computed once, shared by the tests, never written to)."""
    data, bb = _cases()[name]
    p = _params(block_bytes=bb)
    for k, v in EFFORT_PARAMS[effort].items():
        setattr(p, k, v)
    want = O.compress(data, p)
    want.setflags(write=False)
    return want


def test_lengths_cover_every_prefetch_boundary():
    """The cases are the ones the module's docstring names: a thread's two prefetched words (8t and 8t + 4 behind a round's
    look-ahead) lie inside the strip up to n - 4 and n - 8, so the deltas put n on both sides of both for the last thread
    and of a word's middle; the last round is one step of a few positions behind one, two and four full rounds, or all
    eight steps with the last one a position short (kRound - 1)."""
    assert sorted(EFFORTS) == sorted(EFFORT_PARAMS) and len(set(EFFORTS)) == len(EFFORTS)
    assert ROUND + LOOK in LENGTHS and 2 * ROUND + LOOK in LENGTHS and CHUNK + LOOK in LENGTHS
    assert len(LENGTHS) == 3 * len(DELTAS) + 3  # (kLook + 8 * 1024 - 4 is kRound + kLook - 4 again)
    for data, bb in _cases().values():
        assert bb % CHUNK == 0 and data.dtype == np.uint8
    for name in ("strips3", "strips4"):
        data, bb = _cases()[name]
        assert data.size % bb == CHUNK + 5 and data.size // bb + 1 == int(name[-1])
    assert _cases()["noise_text"][0].size == 96 * 1024 + 13


@pytest.mark.parametrize("effort", EFFORTS)
def test_oracle_streams_round_trip(effort):
    for name, (data, _) in _cases().items():
        st, w, back = O.decompress(_want(name, effort), data.size)
        assert st == 0 and w == data.size and np.array_equal(back, data), (name, effort)


@pytest.mark.gpu
@pytest.mark.parametrize("effort", EFFORTS)
def test_strip_ends_bit_exact_vs_oracle(compressor, effort):
    for name, (data, bb) in _cases().items():
        got = np.frombuffer(compressor.compress(data, effort=effort, block_bytes=bb), np.uint8)
        want = _want(name, effort)
        assert got.size == want.size, f"{name}/{effort}: size {got.size} != {want.size}"
        assert np.array_equal(got, want), f"{name}/{effort}: first diff at {np.flatnonzero(got != want)[:4]}"
