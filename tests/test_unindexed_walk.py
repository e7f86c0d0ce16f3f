"""The walk rule (tests/unindexed_walk.py) on the CPU: streams of the oracle encoder and of zlib recover the
index the writer knows; an unflushed stream is not indexable."""
import os
import zlib

import numpy as np
import pytest

import oracle_lib as O
import unindexed_walk as W
from starflate_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _mixed(n, seed):
    rng = np.random.default_rng(seed)
    text = synth.gen_text(n, seed=seed)
    noise = rng.integers(0, 256, n, dtype=np.uint8)
    mask = (np.arange(n) // 40000) % 2 == 1
    return np.where(mask, noise, text).astype(np.uint8)


@pytest.mark.parametrize("name", ["starfleet.html.dynamic.flushed", "starfleet.html.fixed.flushed"])
def test_golden_index(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        stream = f.read()
    want = np.fromfile(os.path.join(GOLDEN, name + ".index"), dtype="<u8").tolist()
    n = os.path.getsize(os.path.join(GOLDEN, "starfleet.html"))
    assert W.recover_index(stream, n) == want


@pytest.mark.parametrize("kind", ["text", "noise", "mixed", "zeros"])
@pytest.mark.parametrize("strip", [32768, 4 * 32768])
@pytest.mark.parametrize("n", [0, 1, 32767, 32768, 32769, 5 * 32768 + 7])
def test_oracle_streams(kind, strip, n):
    data = {"text": lambda: synth.gen_text(n, seed=n + 1),
            "noise": lambda: np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8),
            "mixed": lambda: _mixed(n, n + 3),
            "zeros": lambda: np.zeros(n, np.uint8)}[kind]()
    stream, index, _ = O.compress_indexed(data, O.default_params(strip_bytes=strip))
    assert W.recover_index(stream.tobytes(), n) == index.tolist()


@pytest.mark.parametrize("container,wbits", [("raw", -15), ("zlib", 15), ("gzip", 31)])
@pytest.mark.parametrize("flush", [zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH])
@pytest.mark.parametrize("finish_block", [True, False])
def test_zlib_streams(container, wbits, flush, finish_block):
    data = _mixed(6 * 32768 + 100, 5).tobytes()
    stream = W.zlib_flushed(data, 6, flush, wbits, finish_block)
    ix = W.recover_index(stream, len(data), container)
    # every segment inflates, on its own with the bytes before it as history, to its 32 KiB
    d = zlib.decompressobj(-15)
    out = b"".join(d.decompress(stream[ix[k]:ix[k + 1]]) for k in range(len(ix) - 1))
    assert out == data


def test_stored_payload_markers():
    # noise the encoder stores, full of flush markers and fake stored headers: the walk jumps over the payloads
    rng = np.random.default_rng(9)
    data = rng.integers(0, 256, 8 * 32768, dtype=np.uint8)
    for off in range(100, data.size - 8, 300):
        data[off:off + 4] = (0, 0, 0xFF, 0xFF)
    for off in range(250, data.size - 8, 1000):
        data[off:off + 5] = (0, 0, 0x80, 0xFF, 0x7F)
    stream, index, _ = O.compress_indexed(data, O.default_params(strip_bytes=32768))
    assert W.recover_index(stream.tobytes(), data.size) == index.tolist()


def test_unflushed_not_indexable():
    data = synth.gen_text(4 * 32768, seed=3).tobytes()
    with pytest.raises(W.NotIndexable):
        W.recover_index(zlib.compress(data, 6)[2:-4], len(data))
