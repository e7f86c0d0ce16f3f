"""Look-alikes of block starts inside stored payloads, for the stream decoders' tests (tests/test_gpu_stream_stored.py,
tests/stream_malformed_cases.py): bytes that the candidate filter of k_stream_find takes for a block start and that are none.
A record started on one is off the chain and has to be repaired.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import deflate_writer as W


def look(v, ln):
    """`v LEN NLEN`: with v < 32 a stored block's header byte and its length fields"""
    return bytes([v]) + ln.to_bytes(2, "little") + (ln ^ 0xFFFF).to_bytes(2, "little")


def stored_look_alikes(seed, nblocks=12, size=1500):
    """stored blocks of `size` bytes whose payloads hold look-alikes, most of them with another look-alike where their payload
    would end, so that the finder takes them: LEN inside the payload, LEN past the next true header (past the body in the last
    two blocks), a chain of three in which each lands exactly on the next, and one with random bytes behind it"""
    rng = np.random.default_rng(seed)
    bw, out = W.BitWriter(), bytearray()
    for b in range(nblocks):
        p = bytearray(rng.integers(32, 256, size, dtype=np.uint8).tobytes())
        p[40:45] = look(0, 155)                     # inside the payload: 45 + 155 = 200
        p[200:205] = look(0, 60 + b)                # (random bytes behind it)
        p[340:345] = look(int(rng.integers(0, 32)), 2 * (size + 5) + 200 - 345)  # byte 200 of the block after the next
        p[640:645] = look(0, 300)                   # a chain of three: 645 + 300 = 945, 950 + 300 = 1250,
        p[945:950] = look(0, 300)
        p[1250:1255] = look(0, size + 5 + 200 - 1255)  # and from there to byte 200 of the next block
        W.write_stored(bw, bytes(p))
        out += p
    W.write_stored(bw, b"", final=True)
    return bw.bytes().tobytes(), bytes(out)


def stored_payload(seed, size=300):
    """a stored payload that starts with a stored look-alike the finder takes: `0 LEN NLEN` whose payload ends on a second one"""
    p = bytearray(np.random.default_rng(seed).integers(32, 256, size, dtype=np.uint8).tobytes())
    p[0:5] = look(0, 150)
    p[155:160] = look(0, 40)
    return bytes(p)


def dynamic_payload(seed, size=300):
    """a stored payload that starts with a dynamic-header look-alike: the bytes of a whole, good, non-final dynamic block (so
    the strict predicate holds at its first bit), then noise"""
    rng = np.random.default_rng(seed)
    toks = [int(x) for x in rng.integers(97, 105, 120)] + [W.match(30, 7), W.match(9, 1)]
    bw = W.BitWriter()
    t, ll, dl, _ = W.huffman_block(toks)
    W.write_dynamic(bw, t, ll, dl)
    head = bw.bytes().tobytes()
    assert len(head) < size
    return head + rng.integers(32, 256, size - len(head), dtype=np.uint8).tobytes()
