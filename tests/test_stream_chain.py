"""The chain rule of the stream decoder: the library's own step C (sf::stream_chain_round, sf_stream_chain.h, compiled for the
host) driven by tests/stream_chain.py's model of the decode passes: over true, injected false and deleted candidates it always
yields exactly the serial decoder's block sequence; a clean candidate set needs no repair round, and a run of false candidates
(stored blocks full of DEFLATE data) is mended in one round, not one round per link."""
import numpy as np
import pytest

import stream_chain as SC


def _stream(rng, nblocks):
    sizes = rng.integers(20, 3000, nblocks)
    return SC.Stream([int(x) for x in np.cumsum(sizes)], rng)


@pytest.mark.parametrize("seed", range(60))
def test_chain_is_the_serial_sequence(seed):
    rng = np.random.default_rng(seed)
    st = _stream(rng, int(rng.integers(1, 80)))
    true = st.starts
    keep = [s for s in true[1:] if rng.random() > (seed % 4) * 0.25]  # deleted candidates
    false = [int(x) for x in rng.integers(1, st.ends[-1], int(rng.integers(0, 60)))]  # injected ones
    cands = sorted(set([0] + keep + false))
    blocks, last, rounds = SC.chain(st, cands)
    assert blocks == list(range(len(st.ends)))
    assert last["final"] and last["status"] == 0


def test_true_candidates_need_no_repair():
    rng = np.random.default_rng(1)
    st = _stream(rng, 50)
    blocks, _, rounds = SC.chain(st, list(st.starts))
    assert blocks == list(range(50)) and rounds == 0


def test_no_candidates_one_chunk():
    rng = np.random.default_rng(2)
    st = _stream(rng, 20)
    blocks, _, rounds = SC.chain(st, [0])
    assert blocks == list(range(20)) and rounds == 0



def test_false_run_is_one_round():
    """every candidate but chunk 0 false (a stored stream whose payload is DEFLATE data): one repair round, not one per link"""
    rng = np.random.default_rng(4)
    st = SC.Stream([int(x) for x in np.cumsum(np.full(200, 5000))], rng, garbage_error=0.0)
    cands = [0] + [int(s) + 1000 for s in st.starts[1:]]
    blocks, last, rounds = SC.chain(st, cands)
    assert blocks == list(range(200)) and last["final"]
    assert rounds <= 2, rounds
