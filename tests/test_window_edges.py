"""Where a match may reach: the window and strip edges, on the CPU (the GPU side: tests/test_gpu_window_edges.py).

Inputs that put the encoder's candidates exactly on its edges -- random bytes repeating with a period of 16384, 32767,
32768 or 32769 (the window is 32768 bytes: a period of 32768 is matchable at every position, one of 32769 at none), and
isolated repeats of four bytes at distances 4095, 4096 and 4097 (a 4-byte match farther than 4096 is dropped) -- and
writer-made strips (tests/deflate_writer.py) whose matches reach into stored segments at every stream alignment, straddle
the GPU decoder's 3968-byte steps and its 36 KiB ring, and reach back exactly to the start of a strip.

Here: the writer's strips and stored blocks decode with zlib and with the oracle's restatement of the reference decoder to
the writer's own bytes; its match walk (W.inflate(matches=...)) reports exactly the tokens that were written; and the
oracle's streams for the periodic inputs obey the window rules and reach the edge as often as the GPU tests expect."""
import zlib

import numpy as np
import pytest

import deflate_writer as W
import oracle_lib as O

CHUNK = 32768
WINDOW = 32768
PARSE_REGION = 512  # a match never crosses one (sf_device.h kRegion; the oracle's region_bytes)
PERIODS = (16384, 32767, 32768, 32769)
FAR4 = 4096
KB_SPAN, KB_RING = 3968, 36864  # the GPU decoder's step and ring (sf_inflate.hip)
RING_EDGE = (-100, -1, 0, 1)  # where overlapping copies start around the ring's w-th wrap: RING_EDGE[w % 4]

# The oracle's own effort parameters (test_gpu_parity.EFFORT_PARAMS), repeated so the CPU suite does not import a GPU module.
EFFORTS = {"default": {}, "fast": {"depth": 1}, "fastest": {"depth": 1, "use_near": 0}, "thorough": {"stride2": 0, "step": 512},
           "max": {"stride2": 0, "step": 512, "hash_bits": 12, "long_hash_bytes": 7},
           "best": {"chain_depth": 8}, "ultra": {"chain_depth": 16}, "extreme": {"chain_depth": 32},
           "recent": {"recent": 1, "near_depth": 1, "link_steps": 1},
           "recent_all": {"recent": 1, "near_depth": 1, "link_steps": 1, "stride2": 0, "step": 512}}

# Fraction of the bytes past each strip's first chunk that distance-32768 matches cover, period 32768, stored fast path off.
# Measured with the oracle (random and six-bit bytes alike, strips of 64 KiB and 1 MiB):
#   default 0.936 / 0.922, fast and fastest 0.632 / 0.645, thorough 0.963 / 0.961, max 0.529 / 0.583,
#   best 0.9998 / 0.9997, ultra and extreme 1.0, recent 0.936 / 0.921, recent_all 0.961 / 0.958.
EDGE_FLOOR = {"default": 0.90, "fast": 0.60, "fastest": 0.60, "thorough": 0.94, "max": 0.50, "best": 0.99, "ultra": 0.99,
              "extreme": 0.99, "recent": 0.90, "recent_all": 0.94}


def periodic(period, n, six=False, seed=0):
    """n bytes repeating one random block of `period` bytes; six: bytes < 64, so a chunk of literals is still coded"""
    rng = np.random.default_rng(seed * 100003 + period + (1 << 20) * six)
    return np.tile(rng.integers(0, 64 if six else 256, period, dtype=np.uint8), n // period + 1)[:n]


def four_byte_input(n=5 * CHUNK + 321, seed=0):
    """random filler with isolated repeats -- (length, distance) in turn (4, 4095), (4, 4096), (4, 4097), (5, 4097) --
    every 700 bytes from 8192 on: the longest match at a repeat's position and distance is exactly its length.
    -> (data, [(position, length, distance)])"""
    rng = np.random.default_rng(seed + 41)
    d = rng.integers(0, 256, n, dtype=np.uint8)
    kinds = ((4, 4095), (4, 4096), (4, 4097), (5, 4097))
    sites = []
    for k, q in enumerate(range(8192, n - 16, 700)):
        ln, dist = kinds[k % 4]
        d[q:q + ln] = d[q - dist:q - dist + ln]
        if d[q + ln] == d[q - dist + ln]:
            d[q + ln] ^= 0x5A
        if d[q - 1] == d[q - dist - 1]:
            d[q - 1] ^= 0xA5
        sites.append((q, ln, dist))
    for q, ln, dist in sites:
        assert bytes(d[q:q + ln]) == bytes(d[q - dist:q - dist + ln]) and d[q + ln] != d[q - dist + ln] and d[q - 1] != d[q - dist - 1]
    return d, sites


def params(effort, bb, fast=True, lazy=3, strategy=0):
    return O.default_params(strip_bytes=bb, fast_skip=int(fast), lazy=lazy, strategy=strategy, **EFFORTS[effort])


def walk(stream):
    """-> (decoded bytes, [(output position, distance, length)]) by the writer's own reader"""
    m = []
    out, _ = W.inflate(stream, matches=m)
    return out, m


def check_window_rules(matches, bb):
    """what every stream of the encoder obeys, whatever the effort: a match reaches back at most 32768 bytes and never
    before its strip, does not cross a parse region (so neither a sub-index region nor a chunk), and a 4-byte one is
    never farther than 4096"""
    for pos, dist, ln in matches:
        assert 3 <= ln <= 258 and 1 <= dist <= WINDOW, (pos, dist, ln)
        assert pos - dist >= pos // bb * bb, ("before the strip", pos, dist, bb)
        assert pos // PARSE_REGION == (pos + ln - 1) // PARSE_REGION, ("crosses a region", pos, ln)
        assert not (ln == 4 and dist > FAR4), ("a far 4-byte match", pos, dist)


def edge_coverage(matches, n, bb, dist=WINDOW):
    """bytes covered by matches at `dist`, over the bytes past each strip's first chunk (None: there are none)"""
    past = sum(max(0, min(s + bb, n) - (s + CHUNK)) for s in range(0, n, bb))
    return sum(ln for _, d, ln in matches if d == dist) / past if past else None


def check_four_byte_sites(matches, sites):
    """no 4-byte match farther than 4096; -> (4-byte matches at exactly 4096, 5-byte ones at 4097) at the planted sites"""
    at = {p: (d, ln) for p, d, ln in matches}
    assert not any(ln == 4 and d > FAR4 for _, d, ln in matches)
    n4096 = sum(1 for q, ln, dist in sites if dist == 4096 and at.get(q) == (4096, 4))
    n5 = sum(1 for q, ln, dist in sites if ln == 5 and at.get(q) == (4097, 5))
    return n4096, n5


# ---- writer-made strips ----

def edge_tokens(rng, n, hist, dists, at=(), clip_region=False, lit_p=0.3):
    """tokens for n bytes of a segment with `hist` bytes of strip history: literals and matches at the distances `dists`
    (those that fit), lengths mostly 258; at: {position: (length, distance)} matches placed exactly there.
    clip_region: no match crosses a 1024-byte region (the sub-index's condition)."""
    toks, pos, at = [], 0, dict(at)
    while pos < n:
        if pos in at:
            ln, dist = at.pop(pos)  # (the writer checks its distance against the strip)
            assert pos + ln <= n
            toks.append(W.match(ln, dist))
            pos += ln
            continue
        room = n - pos
        nxt = min([p for p in at if p > pos] + [n])
        room = min(room, nxt - pos)
        if clip_region:
            room = min(room, W.REGION - pos % W.REGION)
        ok = [d for d in dists if d <= hist + pos]
        if room < 3 or not ok or rng.random() < lit_p:
            toks.append(int(rng.integers(0, 256)))
            pos += 1
            continue
        ln = min(room, 258 if rng.random() < 0.6 else int(rng.integers(3, 259)))
        toks.append(W.match(ln, int(ok[rng.integers(len(ok))])))
        pos += ln
    return np.array(toks, np.uint32)


def raw_strips(seed=0):
    """Four strips of four segments (block_bytes 131072).  Strip k holds a stored segment whose data sits at stream
    offset k (mod 4) -- segment 1 of strips 0 and 2, segment 0 of strips 1 and 3 -- and the segment behind it copies
    from it at distances 32768, 32767 and 32768 - 257 (lengths up to 258, from its first byte on); the other segments
    copy from anything within the window.  -> (segments, strip_segments, raw segment numbers)"""
    rng = np.random.default_rng(seed + 5)
    segs, raws = [], []
    far = (WINDOW, WINDOW - 1, WINDOW - 257)
    for k in range(4):
        r = 1 if k % 2 == 0 else 0
        for s in range(4):
            hist = s * CHUNK
            if s == r:
                segs.append(W.RawSegment(rng.integers(0, 256, CHUNK, dtype=np.uint8).tobytes(), raw_mod=k))
                raws.append(len(segs) - 1)
            elif s == r + 1:
                segs.append([W.huffman_block(edge_tokens(rng, CHUNK, hist, far, at={0: (258, WINDOW)}, lit_p=0.1))])
            else:
                segs.append([W.huffman_block(edge_tokens(rng, CHUNK, hist, (1, 2, 3, 4096, 32768 - 1000, WINDOW)))])
    return segs, 4, raws


def step_edge_strip(clip_region=False, seed=0):
    """One strip of eight segments (block_bytes 262144): overlapping copies (distance 1..3, length 258, or up to the
    region's end with clip_region) starting where p % 3968 is 3967, 0 or 1 (all three in every segment), and where the strip position
    is a multiple of 36864 (the ring's size) plus RING_EDGE; copies at distance 100..3000
    of bytes the same step made; distance-32768 copies across the segment boundary in between."""
    rng = np.random.default_rng(seed + 9)
    segs = []
    for s in range(8):
        hist = s * CHUNK
        want = []  # in order of priority: the ring's wrap, the step edges, the same step's bytes
        for w in range(1, 8):
            want.append((w * KB_RING + RING_EDGE[w % 4] - hist, 258, 1 + w % 3))
        for j in range(9):  # one edge per step: 258-byte copies a byte apart would overlap
            e = (-1, 0, 1)[(j + s) % 3]
            want.append((j * KB_SPAN + e, 258, 1 + (j + e) % 3))
        for j in range(8):
            want.append((j * KB_SPAN + 1500, 200, 100 + 300 * j))
        keep = {}
        for p, ln, d in want:
            if clip_region:
                ln = min(ln, W.REGION - p % W.REGION)
            if not (0 <= p < CHUNK - 300 and ln >= 3 and d <= hist + p):
                continue
            if all(p + ln <= q or q + lq <= p for q, (lq, _) in keep.items()):
                keep[p] = (ln, d)
        segs.append([W.huffman_block(edge_tokens(rng, CHUNK, hist, (1, 2, 3, 100, WINDOW), at=keep, clip_region=clip_region))])
    return segs, 8


def first_of_strip(dist_extra, seed=0):
    """Four segments; segment 3 copies from its own first byte (dist == out_pos) at several positions -- or, dist_extra 1,
    one byte farther, into segment 2.  Segment 3 is a strip's first with block_bytes 32768 or 98304 and a strip's second
    with 65536.  No match crosses a 1024-byte region (the sub-index applies)."""
    rng = np.random.default_rng(seed + 13)
    segs = []
    for s in range(4):
        hist = (s % 2) * CHUNK  # strips of two segments: what the writer may assume for the bad variant as well
        at = {}
        if s == 3:
            at = {1: (3, 1 + dist_extra), 700: (258, 700 + dist_extra), 5000: (100, 5000 + dist_extra),
                  CHUNK - 600: (258, CHUNK - 600 + dist_extra)}  # (1 + dist_extra: the random tokens' distances are others)
            at = {p: (min(ln, W.REGION - p % W.REGION), d) for p, (ln, d) in at.items()}
        segs.append([W.huffman_block(edge_tokens(rng, CHUNK if s < 3 else CHUNK - 77, 0 if s == 3 else hist, (1, 3, 64, 1000),
                                                 at=at, clip_region=True))])
    return segs, 2


def _decodes(stream, data):
    assert zlib.decompress(stream.tobytes(), -15) == data
    st, w, back = O.decompress(stream, len(data))
    assert st == 0 and w == len(data) and back.tobytes() == data


def test_stored_blocks_and_raw_segments():
    stream, _, _, data, _ = W.write_stream([[b"", b"abc", b"", b"de"]])
    assert data == b"abcde" and zlib.decompress(stream.tobytes(), -15) == data
    for mod in range(4):
        stream, _, _, data, reps = W.write_stream([W.RawSegment(b"xyz", raw_mod=mod)])
        assert zlib.decompress(stream.tobytes(), -15) == b"xyz" and reps[-1]["data_byte"] % 4 == mod
    segs, k, raws = raw_strips()
    stream, idx, _, data, reps = W.write_stream(segs, strip_segments=k)
    _decodes(stream, data)
    stored = [r for r in reps if r.get("type") == 0 and r["len"]]
    assert [r["data_byte"] % 4 for r in stored] == [0, 1, 2, 3] and all(r["len"] == CHUNK for r in stored)
    for r, s in zip(stored, raws):  # the data is where the segment's bytes are, in a segment of its own
        assert idx[s] <= r["data_byte"] < idx[s + 1]
        assert stream[r["data_byte"]: r["data_byte"] + CHUNK].tobytes() == data[s * CHUNK: (s + 1) * CHUNK]
    out, m = walk(stream)
    assert out == data
    for s in raws:  # the segment behind the stored one reaches into it from its first byte on, at all three distances
        lo = (s + 1) * CHUNK
        far = {d for p, d, _ in m if lo <= p < lo + CHUNK and p - d >= s * CHUNK and p - d < lo}
        assert far == {WINDOW, WINDOW - 1, WINDOW - 257} and (lo, WINDOW, 258) in m


def test_strip_history_is_the_writers_rule():
    rng = np.random.default_rng(1)
    lits = [W.huffman_block(rng.integers(0, 256, CHUNK).astype(np.uint32))]
    reach = [W.huffman_block(edge_tokens(rng, 1000, CHUNK, (WINDOW,), at={0: (258, WINDOW)}))]
    stream, _, _, data, _ = W.write_stream([lits, reach], strip_segments=2)
    _decodes(stream, data)
    assert data[CHUNK:CHUNK + 258] == data[:258]
    with pytest.raises(AssertionError):
        W.write_stream([lits, reach], strip_segments=1)  # the second segment is a strip of its own: no history


@pytest.mark.parametrize("clip", [False, True])
def test_step_edge_strip(clip):
    segs, k = step_edge_strip(clip)
    stream, idx, sub, data, _ = W.write_stream(segs, strip_segments=k, subindex=clip)
    _decodes(stream, data)
    out, m = walk(stream)
    assert out == data
    want = []
    pos = 0
    for blocks in segs:
        for t in blocks[0][0].tolist():
            if t & W.MATCH:
                want.append((pos, (t & 0x7FFF) + 1, ((t >> 16) & 0xFF) + 3))
                pos += want[-1][2]
            else:
                pos += 1
    assert m == want  # the walk reports exactly the tokens written
    for s in range(8):
        assert {p % CHUNK % KB_SPAN for p, d, _ in m if d <= 3 and p // CHUNK == s} >= {KB_SPAN - 1, 0, 1}, s
    starts = {p for p, d, _ in m if d <= 3}
    assert all(w * KB_RING + RING_EDGE[w % 4] in starts for w in range(1, 8) if not (clip and RING_EDGE[w % 4] == -1))


def test_first_segment_of_a_strip():
    for extra in (0, 1):
        segs, k = first_of_strip(extra)
        stream, idx, sub, data, _ = W.write_stream(segs, strip_segments=k, subindex=True)
        _decodes(stream, data)
        _, m = walk(stream)
        lo = 3 * CHUNK
        mine = [(p - lo, d) for p, d, _ in m if p >= lo and d > 64 and d != 1000]
        assert len(mine) == 3 and all(d == p + extra for p, d in mine)
        assert (lo + 1, 1 + extra) in {(p, d) for p, d, _ in m}
    with pytest.raises(AssertionError):
        W.write_stream(first_of_strip(1)[0], strip_segments=1, subindex=True)


@pytest.mark.parametrize("period", PERIODS)
def test_oracle_at_the_window_edge(period):
    """the specification's own streams for the periodic inputs: the window rules hold, a period of 32768 is matched at
    distance 32768 (at least EDGE_FLOOR of the bytes, fast path off), one of 32767 at 32767, one of 32769 not at all"""
    for six in (False, True):
        data = periodic(period, 3 * CHUNK + 1111, six)
        for effort in ("default", "best", "recent_all", "max"):
            for bb, fast in ((65536, False), (131072, True)):
                s = O.compress(data, params(effort, bb, fast))
                out, m = walk(s)
                assert out == data.tobytes()
                check_window_rules(m, bb)
                if period == 32769:
                    assert (six or not m) and all(ln < 16 for _, _, ln in m)  # six-bit bytes: a few chance matches
                elif period in (32767, 32768):
                    assert {d for _, d, _ in m if d > 4096} <= {period}
                    if not fast:
                        assert edge_coverage(m, data.size, bb, period) >= EDGE_FLOOR[effort], (effort, six, bb)


def test_oracle_four_byte_cut():
    data, sites = four_byte_input()
    total = [0, 0]
    for effort in EFFORTS:
        s = O.compress(data, params(effort, 131072, fast=False, strategy=3))
        out, m = walk(s)
        assert out == data.tobytes()
        check_window_rules(m, 131072)
        n4096, n5 = check_four_byte_sites(m, sites)
        total[0] += n4096
        total[1] += n5
    assert total[0] > 0 and total[1] > 0
