"""What tests/test_gpu_single_decode_record.py and tests/test_gpu_batch_inflate.py share: the record of the single decode made by
the commit before it became a batch of one (tests/golden/single_decode_parent.json), the items of the two batch tests whose
single-call statuses that record holds, and a context created under environment variables."""
import json
import os

from conftest import GOLDEN
from starflate_amd import synth

CHUNK = 32768
GOLDEN_JSON = os.path.join(GOLDEN, "single_decode_parent.json")


def parent_record():
    with open(GOLDEN_JSON) as f:
        return json.load(f)


def nseg_of(n):
    return max(1, -(-n // CHUNK))


def _split(idx, sub, sizes):
    """the flattened batch index -> per item (index, subindex), views"""
    out, e, g = [], 0, 0
    for n in sizes:
        k = nseg_of(n)
        out.append((idx[e: e + k + 1], sub[g * 64: (g + k) * 64]))
        e += k + 1
        g += k
    return out


def damaged_batch(comp):
    """test_raw_items_equal_the_single_call_damaged_ones_included's items: (sizes, items, streams, idx, sub, bb, per)"""
    sizes = (70000, 200000, 100000, 50000, 300000, 1000)
    items = [synth.gen_text(n, seed=30 + i) for i, n in enumerate(sizes)]
    streams = [bytearray(s) for s in comp.compress_batch(items, block_bytes=262144)]
    idx, sub, bb = comp.last_batch_index()
    idx, sub, bb = idx.copy(), sub.copy(), bb.copy()
    per = _split(idx, sub, sizes)
    streams[1][len(streams[1]) // 2] ^= 0x5A          # a flipped body byte
    per[2][0][1] += 3                                  # a wrong index entry
    per[3][1][2 * 5] += 7                              # a wrong sub-index word
    bb[4] = 32768                                      # too small a block_bytes: InvalidDistance
    return sizes, items, [bytes(s) for s in streams], idx, sub, bb, per


def first_entry_batch(comp):
    """test_raw_items_with_a_first_entry_past_0's items: gzip streams read as raw bodies through their index"""
    sizes = (5000, 70000, 40000)
    items = [synth.gen_text(n, seed=50 + i) for i, n in enumerate(sizes)]
    streams = comp.compress_batch(items, container="gzip")
    idx, sub, bb = comp.last_batch_index()
    idx = idx.copy()
    per = _split(idx, sub, sizes)
    assert all(int(p[0][0]) == 10 for p in per)
    per[2][0][0] += 1  # a damaged entry 0
    return sizes, items, streams, idx, sub, bb, per


def context_under(**env):
    """a Compressor whose context was created with these environment variables set (SFH_BATCH_CHUNKS, SFH_INFLATE_SERIAL)"""
    from starflate_amd import Compressor

    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Compressor(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
