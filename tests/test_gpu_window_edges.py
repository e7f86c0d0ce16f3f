"""Where a match may reach, on the GPU (the CPU side and the inputs: tests/test_window_edges.py).

Compressor: periodic inputs put k_lz77's candidates exactly on the window's edge at every position of every strip (a period
of 32768: every match is at distance 32768; 32767: at 32767; 32769: none) through the step codes' ageing, the window checks
and the 4-byte cut (kFar4), for every effort, strip size, fast-path setting and, on a subset, lazy level.  Streams must be
bit-exact with the oracle and round-trip; walked by the writer's reader, they must obey the window rules on their own and
reach the edge as often as the oracle's do.

Decoders: the compressor's own period-32768 streams (a distance-32768 copy across a segment boundary in every token, and
into stored segments with the fast path on) and writer-made strips (stored segments at every raw_off & 3, copies at 32768,
32767 and 32768 - 257 into them, overlapping copies across the 3968-byte steps and the 36 KiB ring's wrap, dist == out_pos
in a strip's first segment and one byte more) through every decode path, with the strip size, twice it and half of it."""
import zlib

import numpy as np
import pytest

import deflate_writer as W
import oracle_lib as O
from test_gpu_parity import EFFORT_PARAMS
from test_window_edges import (CHUNK, EDGE_FLOOR, EFFORTS, PERIODS, WINDOW, check_four_byte_sites, check_window_rules,
                               edge_coverage, first_of_strip, four_byte_input, params, periodic, raw_strips, step_edge_strip,
                               walk)

pytestmark = pytest.mark.gpu

INVALID_DISTANCE = 7


@pytest.fixture(scope="module")
def serial():
    """a context made with SFH_INFLATE_SERIAL=1: the lane-serial kernel decodes every segment"""
    from starflate_amd import Compressor

    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SFH_INFLATE_SERIAL", "1")
        c = Compressor(0)
    yield c
    c.close()


def _paths(compressor, serial, stream, idx, sub, n, bb):
    """-> {path: (bytes, status)} for index + sub-index (when there is one), index only, lane-serial and the batch"""
    out = {}
    if sub is not None:
        out["sub"] = compressor.decompress(stream, idx, n, subindex=sub, block_bytes=bb)
    out["index"] = compressor.decompress(stream, idx, n, block_bytes=bb)
    out["serial"] = serial.decompress(stream, idx, n, block_bytes=bb)
    outs, sts = compressor.decompress_batch([stream], [n], index=idx, subindex=sub, block_bytes=[bb])
    out["batch"] = (outs[0], sts[0])
    return out


def _decodes(compressor, serial, stream, idx, sub, data, bb, what):
    for path, (back, st) in _paths(compressor, serial, stream, idx, sub, len(data), bb).items():
        assert st == 0 and back == data, (what, bb, path, st)


def _invalid(compressor, serial, stream, idx, sub, n, bb, what):
    for path, (_, st) in _paths(compressor, serial, stream, idx, sub, n, bb).items():
        assert st == INVALID_DISTANCE, (what, bb, path, st)


def _strip_sizes(compressor, serial, stream, idx, sub, data, bb, what):
    """the strip size and twice it decode; half of it (when that is a strip at all and splits the data) is InvalidDistance"""
    _decodes(compressor, serial, stream, idx, sub, data, bb, what)
    _decodes(compressor, serial, stream, idx, sub, data, 2 * bb, what)
    if bb >= 2 * CHUNK and len(data) > bb // 2:
        _invalid(compressor, serial, stream, idx, sub, len(data), bb // 2, what)


def test_efforts_are_the_parity_suites():
    assert EFFORTS == EFFORT_PARAMS


@pytest.mark.parametrize("effort", sorted(EFFORTS))
def test_compressor_at_the_window_edge(compressor, serial, effort):
    for period in PERIODS:
        for six in (False, True):
            data = periodic(period, 4 * CHUNK + 777, six)  # a ragged tail
            for bb in (32768, 65536, 1 << 20):
                for fast in (False, True):
                    got = np.frombuffer(compressor.compress(data, stored_fast_path=fast, block_bytes=bb, effort=effort), np.uint8)
                    assert compressor.last_block_bytes() == bb
                    want = O.compress(data, params(effort, bb, fast))
                    what = (effort, period, six, bb, fast)
                    assert got.size == want.size and np.array_equal(got, want), what
                    assert zlib.decompress(got.tobytes(), -15) == data.tobytes()
                    if period == WINDOW or (bb == 65536 and not six):
                        out, m = walk(got)
                        assert out == data.tobytes()
                        check_window_rules(m, compressor.last_block_bytes())
                        if period == WINDOW and not fast and bb > CHUNK:
                            assert edge_coverage(m, data.size, bb) >= EDGE_FLOOR[effort], what
                    if period == WINDOW and bb > CHUNK:
                        idx, sub = compressor.last_index(), compressor.last_subindex()
                        _strip_sizes(compressor, serial, got, idx, sub, data.tobytes(), bb, what)
    # lazy 0 (and 3 above) where every match is on the edge
    data = periodic(WINDOW, 3 * CHUNK + 99, True)
    for lazy in (0, 1):
        got = np.frombuffer(compressor.compress(data, stored_fast_path=False, block_bytes=65536, effort=effort, lazy=lazy), np.uint8)
        assert np.array_equal(got, O.compress(data, params(effort, 65536, False, lazy=lazy))), (effort, lazy)


@pytest.mark.parametrize("effort", ["default", "best", "recent_all"])
def test_long_strip_at_the_window_edge(compressor, serial, effort):
    """one strip of 4 MiB: the step codes are aged hundreds of times with the candidate on the edge the whole way"""
    bb = 4 << 20
    data = periodic(WINDOW, bb + 4321, True)
    got = np.frombuffer(compressor.compress(data, stored_fast_path=False, block_bytes=bb, effort=effort), np.uint8)
    want = O.compress(data, params(effort, bb, False))
    assert got.size == want.size and np.array_equal(got, want), effort
    assert zlib.decompress(got.tobytes(), -15) == data.tobytes()
    assert got.size < data.size // 8  # the edge is found strip-long, not only at its start
    idx, sub = compressor.last_index(), compressor.last_subindex()
    back, st = compressor.decompress(got, idx, data.size, subindex=sub, block_bytes=bb)
    assert st == 0 and back == data.tobytes()
    back, st = serial.decompress(got, idx, data.size, block_bytes=bb)
    assert st == 0 and back == data.tobytes()


def test_compress_batch_at_the_window_edge(compressor):
    items = [periodic(p, 3 * CHUNK + 5 * p // 1024, six) for p in PERIODS for six in (False, True)]
    for fast in (False, True):
        outs = compressor.compress_batch(items, stored_fast_path=fast, block_bytes=65536)
        for item, out in zip(items, outs):
            assert np.array_equal(np.frombuffer(out, np.uint8), O.compress(item, params("default", 65536, fast)))
            assert zlib.decompress(out, -15) == item.tobytes()


@pytest.mark.parametrize("effort", sorted(EFFORTS))
def test_four_byte_cut(compressor, effort):
    data, sites = four_byte_input()
    n4096 = n5 = 0
    for bb in (32768, 131072):
        got = np.frombuffer(compressor.compress(data, strategy="dynamic", stored_fast_path=False, block_bytes=bb, effort=effort), np.uint8)
        want = O.compress(data, params(effort, bb, False, strategy=3))
        assert got.size == want.size and np.array_equal(got, want), (effort, bb)
        out, m = walk(got)
        assert out == data.tobytes()
        check_window_rules(m, bb)
        a, b = check_four_byte_sites(m, sites)
        n4096 += a
        n5 += b
    # at 223 sites, a quarter of each kind, over both strip sizes the oracle takes 63 (fast, fastest) to 104 (the chains)
    # 4-byte matches at 4096 and 74 to 104 five-byte ones at 4097
    assert n4096 >= 50 and n5 >= 50, (effort, n4096, n5)


def test_decoders_on_raw_strips(compressor, serial):
    segs, k, raws = raw_strips()
    stream, idx, _, data, reps = W.write_stream(segs, strip_segments=k)
    assert zlib.decompress(stream.tobytes(), -15) == data
    assert sorted(r["data_byte"] % 4 for r in reps if r.get("type") == 0 and r["len"]) == [0, 1, 2, 3]
    _strip_sizes(compressor, serial, stream, idx, None, data, k * CHUNK, "raw strips")


@pytest.mark.parametrize("clip", [False, True])
def test_decoders_across_steps_and_the_ring(compressor, serial, clip):
    segs, k = step_edge_strip(clip)
    stream, idx, sub, data, _ = W.write_stream(segs, strip_segments=k, subindex=clip)
    assert zlib.decompress(stream.tobytes(), -15) == data
    _strip_sizes(compressor, serial, stream, idx, sub, data, k * CHUNK, ("steps", clip))


def test_first_segment_of_a_strip(compressor, serial):
    good = W.write_stream(first_of_strip(0)[0], strip_segments=2, subindex=True)
    bad = W.write_stream(first_of_strip(1)[0], strip_segments=2, subindex=True)
    for stream, idx, sub, data, _ in (good, bad):
        assert zlib.decompress(stream.tobytes(), -15) == data
        st, w, back = O.decompress(stream, len(data))
        assert st == 0 and back.tobytes() == data
    # segment 3: a strip's first with 98304-byte strips, its second with 65536
    _decodes(compressor, serial, good[0], good[1], good[2], good[3], 3 * CHUNK, "dist == out_pos")
    _decodes(compressor, serial, good[0], good[1], good[2], good[3], 2 * CHUNK, "dist == out_pos")
    _invalid(compressor, serial, bad[0], bad[1], bad[2], len(bad[3]), 3 * CHUNK, "dist == out_pos + 1")
    _decodes(compressor, serial, bad[0], bad[1], bad[2], bad[3], 2 * CHUNK, "dist == out_pos + 1, second of its strip")
    # the batch, block_bytes per item
    items = (good, bad, bad)
    for sub in (False, True):
        outs, sts = compressor.decompress_batch([s for s, *_ in items], [len(d) for _, _, _, d, _ in items],
                                                index=np.concatenate([i for _, i, *_ in items]),
                                                subindex=np.concatenate([x for _, _, x, _, _ in items]) if sub else None,
                                                block_bytes=[3 * CHUNK, 3 * CHUNK, 2 * CHUNK])
        assert sts == [0, INVALID_DISTANCE, 0] and outs[0] == good[3] and outs[2] == bad[3], (sub, sts)
