"""A plain RFC 1951 writer and reader for tests: dynamic blocks from a token list and code lengths chosen freely by
the caller, so that tests can reach the edges of the format that the compressor's own inputs never reach (15-bit
literal/length and distance codes, 7-bit code-length codes, repeats at their maximum, runs across the HLIT/HDIST
boundary, HLIT = 257 / 286, HDIST = 1 / 30, trimmed HCLEN), and strips whose matches reach back across segments and
into stored segments at any stream alignment.

TEST INFRASTRUCTURE ONLY.  Pure Python and numpy.  Tokens are the oracle's format (uint32: bit 31 match, bits 16..23
length - 3, bits 0..14 distance - 1; else a literal byte).  Every writer returns a report of the code lengths it
actually wrote, so a test can assert that it touched the edge it was built for."""
import heapq

import numpy as np

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
MATCH = 0x80000000
REGION = 1024  # sub-index regions (include/starflate_hip.h: 32 regions of 1024 bytes per segment)
SEGMENT = 32768


def match(length, dist):
    assert 3 <= length <= 258 and 1 <= dist <= 32768
    return MATCH | ((length - 3) << 16) | (dist - 1)


def len_symbol(length):
    """-> (symbol 257..285, extra bits, extra value)"""
    if length == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def dist_symbol(dist):
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return k, DIST_EXTRA[k], dist - DIST_BASE[k]


def token_symbols(tokens):
    """-> (literal/length symbol counts [286] with one end-of-block, distance symbol counts [30])"""
    ll, d = np.zeros(286, np.int64), np.zeros(30, np.int64)
    for t in np.asarray(tokens, np.uint32).tolist():
        if t & MATCH:
            ll[len_symbol(((t >> 16) & 0xFF) + 3)[0]] += 1
            d[dist_symbol((t & 0x7FFF) + 1)[0]] += 1
        else:
            ll[t] += 1
    ll[256] += 1
    return ll, d


def expand(tokens, history=b""):
    """the bytes tokens stand for after `history` (the bytes a match may reach back into)"""
    out = bytearray(history)
    for t in np.asarray(tokens, np.uint32).tolist():
        if t & MATCH:
            length, dist = ((t >> 16) & 0xFF) + 3, (t & 0x7FFF) + 1
            assert dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out[len(history):])


# ---- code lengths ----

def kraft(lens, maxbits=15):
    """Kraft sum of the non-zero lengths in units of 2^-maxbits (complete code: 1 << maxbits)"""
    return sum(1 << (maxbits - int(l)) for l in lens if l)


def huffman_depths(freq):
    """Unconstrained Huffman code lengths (heapq; ties broken arbitrarily, which leaves the maximum depth of a
    Fibonacci-like chain alone).  One used symbol: length 1."""
    used = [(int(f), s) for s, f in enumerate(freq) if f]
    out = np.zeros(len(freq), np.int64)
    if len(used) == 1:
        out[used[0][1]] = 1
    if len(used) < 2:
        return out
    heap = [(f, k, [s]) for k, (f, s) in enumerate(used)]
    heapq.heapify(heap)
    k = len(heap)
    while len(heap) > 1:
        fa, _, a = heapq.heappop(heap)
        fb, _, b = heapq.heappop(heap)
        for s in a + b:
            out[s] += 1
        heapq.heappush(heap, (fa + fb, k, a + b))
        k += 1
    return out


def package_merge(freq, maxbits):
    """Optimal length-limited code lengths (boundary-free package-merge, Larmore & Hirschberg): an independent way to
    get legal codes with lengths up to maxbits.  Needs 2 ** maxbits >= used symbols."""
    used = sorted((int(f), s) for s, f in enumerate(freq) if f)
    out = np.zeros(len(freq), np.int64)
    if len(used) == 1:
        out[used[0][1]] = 1
    if len(used) < 2:
        return out
    assert len(used) <= 1 << maxbits
    leaves = [(f, (s,)) for f, s in used]
    cur = list(leaves)
    for _ in range(maxbits - 1):
        pk = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pk, key=lambda x: x[0])
    for _, syms in cur[: 2 * len(used) - 2]:
        for s in syms:
            out[s] += 1
    return out


def skewed_lengths(freq, maxbits):
    """A complete code as deep as the limit lets it be: package-merge over weights 2^-rank of the symbols by descending
    frequency.  With more than maxbits used symbols, maxbits-bit codes are certain."""
    used = sorted((s for s, f in enumerate(freq) if f), key=lambda s: -freq[s])
    w = [0] * len(freq)
    for i, s in enumerate(used):
        w[s] = 1 << (len(used) - i)
    return package_merge(w, maxbits)


def canonical(lens):
    """RFC 1951 3.2.2: code values (MSB-first) of the non-zero lengths"""
    lens = [int(l) for l in lens]
    bl = [0] * 16
    for l in lens:
        if l:
            bl[l] += 1
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1 if b > 1 else 0
        nxt[b] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = nxt[l]
            nxt[l] += 1
    return out


# ---- bits ----

class BitWriter:
    """LSB-first bit packer.  Whole bytes leave the accumulator as they fill, so a put costs the same at any stream size."""

    def __init__(self):
        self.buf, self.acc, self.nacc = bytearray(), 0, 0

    @property
    def n(self):  # bits written
        return 8 * len(self.buf) + self.nacc

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.nacc
        self.nacc += n
        if self.nacc >= 64:
            k = self.nacc >> 3
            self.buf += (self.acc & ((1 << 8 * k) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.nacc -= 8 * k

    def put_code(self, code, length):  # Huffman codes go MSB first
        self.put(int(f"{code:0{length}b}"[::-1], 2), length)

    def align(self):
        self.nacc += -self.nacc % 8  # (buf holds whole bytes)

    def bytes(self):
        return np.frombuffer(bytes(self.buf) + self.acc.to_bytes((self.nacc + 7) // 8, "little"), np.uint8).copy()


class BitReader:
    def __init__(self, data, bit=0):
        self.b = bytes(np.asarray(data, np.uint8)) + bytes(8)
        self.nbits = 8 * (len(self.b) - 8)
        self.pos = bit

    def get(self, n):
        assert self.pos + n <= self.nbits, "read past the end"
        k = self.pos >> 3
        r = (int.from_bytes(self.b[k:k + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)  # n <= 16
        self.pos += n
        return r


# ---- the code-length RLE ----

def rle(seq, max_repeats=True, avoid=False):
    """Code-length items [(symbol, extra value)] of one sequence.  max_repeats: 16/17/18 take their longest repeats
    (6 / 10 / 138) first; else they take the shortest legal pieces (3 / 3 / 11).  avoid: no 16/17/18 at all."""
    seq = [int(x) for x in seq]
    items, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if avoid:
            items += [(v, 0)] * r
            continue
        if v == 0:
            while r >= 11:
                c = min(r, 138) if max_repeats else (r if r <= 21 else 11)
                if 0 < r - c < 3 and c > 11:  # leave a legal tail
                    c = r - 3 if r - 3 >= 11 else c
                items.append((18, c - 11))
                r -= c
            while r >= 3:
                c = min(r, 10) if max_repeats else (r if r <= 5 else 3)
                items.append((17, c - 3))
                r -= c
            items += [(0, 0)] * r
        else:
            items.append((v, 0))
            r -= 1
            while r >= 3:
                c = min(r, 6) if max_repeats else (r if r <= 5 else 3)
                items.append((16, c - 3))
                r -= c
            items += [(v, 0)] * r
    return items


def _expand_items(items):
    out = []
    for s, e in items:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + e)
        elif s == 17:
            out += [0] * (3 + e)
        else:
            out += [0] * (11 + e)
    return out


# ---- blocks ----

def write_stored_empty(bw, final=False):
    """An empty stored block: byte alignment, as Z_FULL_FLUSH / Z_SYNC_FLUSH leave"""
    bw.put(int(final), 1)
    bw.put(0, 2)
    bw.align()
    bw.put(0, 16)
    bw.put(0xFFFF, 16)


def write_stored(bw, data, final=False):
    """A stored block that carries data (at most 65535 bytes).  -> the stream byte offset of its first data byte"""
    data = bytes(data)
    assert len(data) <= 0xFFFF
    bw.put(int(final), 1)
    bw.put(0, 2)
    bw.align()
    bw.put(len(data), 16)
    bw.put(len(data) ^ 0xFFFF, 16)
    at = bw.n // 8
    if data:
        bw.put(int.from_bytes(data, "little"), 8 * len(data))
    return at


class RawSegment:
    """A segment of one stored block that carries all its bytes, behind as many empty stored blocks as it takes to put
    the first data byte at a stream offset of raw_mod (mod 4); raw_mod None: no empty block in front."""

    def __init__(self, data, raw_mod=None):
        self.data, self.raw_mod = bytes(data), raw_mod


def huffman_block(tokens, **opt):
    """(tokens, ll lengths, d lengths, options): a dynamic block whose codes are package-merge's at 15 bits"""
    tokens = np.asarray(tokens, np.uint32)
    ll, d = token_symbols(tokens)
    return tokens, package_merge(ll, 15), package_merge(d, 15), opt


def write_dynamic(bw, tokens, ll_lens, d_lens, final=False, hlit=None, hdist=None, max_repeats=True, avoid_repeats=False,
                  cross=False, trim_hclen=True, cl_lens=None, region_starts=None):
    """One dynamic block.  ll_lens (286 or 288) / d_lens (30 or 32): the caller's code lengths (each a legal prefix code;
    256 must have a code).  hlit / hdist: how many lengths the header sends (default: trimmed to the last used, at
    least 257 / 1).  cross: one RLE over both sequences, so a run may reach over the HLIT/HDIST boundary (RFC 1951
    3.2.7 allows it).  cl_lens: the code-length code's lengths (default: package-merge at 7 bits of the item counts).
    region_starts: output offsets at which to record (bit position, tokens before) of the first token starting there
    (block-relative bit positions, from bw.n before the call).
    -> report dict: ll / d / cl = sorted code lengths of every symbol written, and what the tests look for."""
    ll = [int(x) for x in ll_lens][:286] + [0] * max(0, 286 - len(ll_lens))
    dl = [int(x) for x in d_lens][:30] + [0] * max(0, 30 - len(d_lens))
    assert ll[256], "end-of-block needs a code"
    assert kraft(ll) <= 1 << 15 and kraft(dl) <= 1 << 15
    if hlit is None:
        hlit = max([257] + [s + 1 for s in range(286) if ll[s]])
    if hdist is None:
        hdist = max([1] + [s + 1 for s in range(30) if dl[s]])
    assert 257 <= hlit <= 286 and 1 <= hdist <= 30
    assert not any(ll[hlit:]) and not any(dl[hdist:])
    seq_l, seq_d = ll[:hlit], dl[:hdist]
    if cross:
        items = rle(seq_l + seq_d, max_repeats, avoid_repeats)
    else:
        items = rle(seq_l, max_repeats, avoid_repeats) + rle(seq_d, max_repeats, avoid_repeats)
    assert _expand_items(items) == seq_l + seq_d
    clf = [0] * 19
    for s, _ in items:
        clf[s] += 1
    if cl_lens is None:
        cl_lens = package_merge(clf, 7)
    elif isinstance(cl_lens, str):
        assert cl_lens == "skewed"
        cl_lens = skewed_lengths(clf, 7)
    cl = [int(x) for x in cl_lens]
    assert all(cl[s] for s in range(19) if clf[s]) and kraft(cl, 7) <= 128 and max(cl) <= 7
    hclen = 19
    if trim_hclen:
        while hclen > 4 and cl[CL_ORDER[hclen - 1]] == 0:
            hclen -= 1
    assert not any(cl[CL_ORDER[k]] for k in range(hclen, 19))
    start = bw.n
    bw.put(int(final), 1)
    bw.put(2, 2)
    bw.put(hlit - 257, 5)
    bw.put(hdist - 1, 5)
    bw.put(hclen - 4, 4)
    for k in range(hclen):
        bw.put(cl[CL_ORDER[k]], 3)
    clc = canonical(cl)
    for s, e in items:
        bw.put_code(clc[s], cl[s])
        if s >= 16:
            bw.put(e, (2, 3, 7)[s - 16])
    llc, dc = canonical(ll), canonical(dl)
    rep = {"ll": set(), "d": set(), "cl": sorted({cl[s] for s, _ in items}), "eob": ll[256], "hlit": hlit, "hdist": hdist,
           "hclen": hclen, "cl_items": items, "len_items": set(), "dist_items": set(), "header_bits": bw.n - start}
    marks, pos, want = {}, 0, sorted(region_starts or [])
    for k, t in enumerate(np.asarray(tokens, np.uint32).tolist()):
        while want and want[0] <= pos:
            marks[want.pop(0)] = (bw.n - start, k)
        if t & MATCH:
            length, dist = ((t >> 16) & 0xFF) + 3, (t & 0x7FFF) + 1
            s, ne, ev = len_symbol(length)
            assert ll[s], f"length symbol {s} has no code"
            bw.put_code(llc[s], ll[s])
            bw.put(ev, ne)
            ds, de, dv = dist_symbol(dist)
            assert dl[ds], f"distance symbol {ds} has no code"
            bw.put_code(dc[ds], dl[ds])
            bw.put(dv, de)
            rep["ll"].add(ll[s])
            rep["d"].add(dl[ds])
            rep["len_items"].add((ll[s], ne, ev))
            rep["dist_items"].add((dl[ds], de, dv))
            pos += length
        else:
            assert ll[t], f"literal {t} has no code"
            bw.put_code(llc[t], ll[t])
            rep["ll"].add(ll[t])
            pos += 1
    while want:
        marks[want.pop(0)] = (bw.n - start, len(tokens))
    bw.put_code(llc[256], ll[256])
    rep["ll"].add(ll[256])
    rep["ll"], rep["d"] = sorted(rep["ll"]), sorted(rep["d"])
    rep["marks"] = marks
    return rep


def segment_tokens_ok(tokens, sub, hist=0):
    """no match crosses a 1024-byte region (the sub-index's condition) and none reaches before the segment's `hist`
    bytes of history (the earlier segments of its strip)"""
    pos = 0
    for t in np.asarray(tokens, np.uint32).tolist():
        n = ((t >> 16) & 0xFF) + 3 if t & MATCH else 1
        if t & MATCH and (t & 0x7FFF) + 1 > pos + hist:
            return False
        if sub and pos // REGION != (pos + n - 1) // REGION:
            return False
        pos += n
    return True


def write_stream(segments, final=True, subindex=False, strip_segments=1):
    """A block-indexed stream: each segment (at most 32768 bytes of output) is a list of blocks, each (tokens, ll_lens,
    d_lens, options dict for write_dynamic) or a bytes-like object (a stored block that carries it; empty: an empty stored
    block), or the segment is a RawSegment; every segment but the last (or every one, final=False) ends with an empty
    stored block, so that the next one starts on a byte.  strip_segments: segments per strip (block_bytes / 32768): a
    segment's matches may reach back into the earlier segments of its strip, never before the strip.  subindex: one
    dynamic block per segment, no match across a 1024-byte region: also the 32 x {bit offset, tokens before} entries per
    segment.  -> (stream uint8, index uint64[nseg + 1], subindex uint32[nseg, 32, 2] or None, output bytes, reports per
    block: write_dynamic's, or {"type": 0, "data_byte": stream offset of its first byte, "len": bytes} for a stored one)"""
    bw = BitWriter()
    idx, subs, reps, out = [0], [], [], bytearray()
    strip = b""
    for si, blocks in enumerate(segments):
        seg_start = bw.n
        assert seg_start % 8 == 0
        if si % strip_segments == 0:
            strip = b""
        seg_out = b""
        last_seg = final and si == len(segments) - 1
        if isinstance(blocks, RawSegment):
            j = 0 if blocks.raw_mod is None else (blocks.raw_mod - (seg_start // 8 + 5)) % 4  # an empty stored block is 5 bytes
            blocks = [b""] * j + [blocks.data]
        for bi, blk in enumerate(blocks):
            fin = last_seg and bi == len(blocks) - 1
            if isinstance(blk, (bytes, bytearray)):
                assert not subindex
                reps.append({"type": 0, "data_byte": write_stored(bw, blk, final=fin), "len": len(blk)})
                seg_out += bytes(blk)
                continue
            tokens, ll, dl, opt = blk
            opt = dict(opt or {})
            if subindex:
                assert len(blocks) == 1 and segment_tokens_ok(tokens, True, len(strip))
                opt["region_starts"] = [r * REGION for r in range(32)]
            reps.append(write_dynamic(bw, tokens, ll, dl, final=fin, **opt))
            seg_out += expand(tokens, strip + seg_out)
        assert len(seg_out) == SEGMENT or (len(seg_out) <= SEGMENT and si == len(segments) - 1), "only the last segment may be short"
        if subindex:  # the one block starts at the segment's first bit: its bit offsets are the segment's
            subs.append(np.array([reps[-1]["marks"][r * REGION] for r in range(32)], np.uint32))
        if not last_seg:
            write_stored_empty(bw)
        bw.align()
        idx.append(bw.n // 8)
        out += seg_out
        strip += seg_out
    stream = bw.bytes()
    return (stream, np.array(idx, np.uint64), np.stack(subs) if subindex else None, bytes(out), reps)


# ---- reading ----

def read_header(br):
    """A dynamic block's header from br (just past BFINAL / BTYPE).  -> dict: hlit, hdist, hclen, cl_lens[19],
    cl_freq[19] (item counts recounted), ll_lens[286], d_lens[30], items"""
    hlit, hdist, hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = br.get(3)
    dec = _decoder(cl, 7)
    seq, items, clf = [], [], [0] * 19
    while len(seq) < hlit + hdist:
        s = _decode(br, dec)
        clf[s] += 1
        if s < 16:
            seq.append(s)
            items.append((s, 0))
        else:
            e = br.get((2, 3, 7)[s - 16])
            items.append((s, e))
            seq += [seq[-1]] * (3 + e) if s == 16 else [0] * ((3 if s == 17 else 11) + e)
    assert len(seq) == hlit + hdist, "a run past the last length"
    ll = seq[:hlit] + [0] * (286 - hlit)
    dl = seq[hlit:] + [0] * (30 - hdist)
    return {"hlit": hlit, "hdist": hdist, "hclen": hclen, "cl_lens": cl, "cl_freq": clf, "ll_lens": ll, "d_lens": dl, "items": items}


def _decoder(lens, maxbits):
    codes = canonical(lens)
    return {(int(l), c): s for s, (l, c) in enumerate(zip(lens, codes)) if l}, maxbits


def _decode(br, dec):
    table, maxbits = dec
    code = 0
    for l in range(1, maxbits + 1):
        code = (code << 1) | br.get(1)
        s = table.get((l, code))
        if s is not None:
            return s
    raise ValueError("no code matches")


def inflate(data, bit=0, stop_at_segment_end=False, matches=None):
    """A plain decoder of raw DEFLATE from `bit` on, for what the tests need to see: -> (bytes, blocks), each block a
    dict with its type, start bit ("start") and output offset ("out"), header (dynamic) and the (code length, extra bits,
    extra value) of every length and distance item and the code length of every literal / end-of-block.  Stops after
    BFINAL (or, stop_at_segment_end, after the first empty stored block).  matches: a list that gets (output position, distance, length) of every match.
    Slow (a Python call per bit of a code): meant for streams of a MiB or so."""
    br = BitReader(data, bit)
    out, blocks = bytearray(), []
    while True:
        fin, typ = br.get(1), br.get(2)
        blk = {"type": typ, "ll": set(), "len_items": set(), "dist_items": set(), "start": br.pos - 3, "out": len(out)}
        blocks.append(blk)
        if typ == 0:
            br.pos += -br.pos % 8
            n, nn = br.get(16), br.get(16)
            assert n ^ nn == 0xFFFF
            for _ in range(n):
                out.append(br.get(8))
            if fin or (stop_at_segment_end and n == 0):
                break
            continue
        assert typ in (1, 2)
        if typ == 2:
            h = read_header(br)
            blk["header"] = h
            ll, dl = h["ll_lens"], h["d_lens"]
        else:
            ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8  # all 288: 286 and 287 move the 9-bit codes
            dl = [5] * 32
        dl_ = _decoder(dl, 15)
        lld = _decoder(ll, 15)
        while True:
            s = _decode(br, lld)
            blk["ll"].add(ll[s])
            if s < 256:
                out.append(s)
            elif s == 256:
                blk["eob"] = ll[s]
                break
            else:
                k = s - 257
                length = LEN_BASE[k] + br.get(LEN_EXTRA[k])
                blk["len_items"].add((ll[s], LEN_EXTRA[k], length - LEN_BASE[k]))
                ds = _decode(br, dl_)
                dist = DIST_BASE[ds] + br.get(DIST_EXTRA[ds])
                blk["dist_items"].add((dl[ds], DIST_EXTRA[ds], dist - DIST_BASE[ds]))
                assert dist <= len(out), "distance too far back"
                if matches is not None:
                    matches.append((len(out), dist, length))
                for _ in range(length):
                    out.append(out[-dist])
        if fin:
            break
    blk["end"] = br.pos
    return bytes(out), blocks
