"""Writer-made streams without flush points for the stream decoders' window tests (tests/test_stream_window.py on the CPU,
tests/test_gpu_stream_window.py on the GPU): far distances (32768, 32767, 32768 - 257) through many chunks and groups,
chunks with prescribed output sizes around 32768, a match with dist == out_pos or out_pos + 1 inside the first 32 KiB, and
the same with a second fault in front of or behind it.  Seeded, built on tests/deflate_writer.py, nothing on disk.  Every
builder returns a Case: the raw stream, the bytes the writer itself expanded, and where each block starts (stream bit, output
offset), from which predict() states the chunk partition a context with nominal chunks of S bytes must arrive at.

TEST INFRASTRUCTURE ONLY."""
import zlib

import numpy as np

import deflate_writer as W
import stream_host as H

WIN = 32768
FAR = (32768, 32767, 32768 - 257)
OK, ERROR, INVALID_BLOCK_HEADER, LEN_MISMATCH, DST_TOO_SMALL, SRC_TOO_SMALL, INVALID_LIT_OR_LEN, INVALID_DISTANCE = range(8)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
SIZE_CLASSES = (32767, 32768, 32769, 3 * 32768 + 5, 5 * 32768)  # and "a few hundred bytes": below 1000


def write_fixed(bw, toks, final=False):
    """One fixed-Huffman block of the tokens"""
    bw.put(int(final), 1)
    bw.put(1, 2)
    llc, dc = W.canonical(FIXED_LL), W.canonical([5] * 32)
    for t in toks:
        if t & W.MATCH:
            ln, d = ((t >> 16) & 0xFF) + 3, (t & 0x7FFF) + 1
            s, eb, ev = W.len_symbol(ln)
            bw.put_code(llc[s], FIXED_LL[s])
            bw.put(ev, eb)
            ds, deb, dev = W.dist_symbol(d)
            bw.put_code(dc[ds], 5)
            bw.put(dev, deb)
        else:
            bw.put_code(llc[t], FIXED_LL[t])
    bw.put_code(llc[256], FIXED_LL[256])


class Case:
    """raw: the raw DEFLATE stream; data: the writer's bytes (a failing stream: the bytes in front of its first fault);
    blocks: [(stream bit, output offset)] of every block start; status: what the serial decoder must answer with room
    enough; fault_out: the output position of the first fault in stream order (a clean stream: len(data))."""

    def __init__(self, name, raw, data, blocks, status=OK, **more):
        self.name, self.raw, self.data, self.blocks, self.status = name, bytes(raw), bytes(data), list(blocks), status
        self.fault_out = len(self.data)
        self.__dict__.update(more)

    @property
    def n(self):
        return len(self.data)

    def wrapped(self, container, isize=None, adler=None):
        """the stream in its container, made on the host (isize / adler: a trailer field to write instead of the true one)"""
        if container == "raw":
            return self.raw
        if container == "zlib":
            a = zlib.adler32(self.data) if adler is None else adler
            return b"\x78\x9c" + self.raw + a.to_bytes(4, "big")
        n = len(self.data) if isize is None else isize
        return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + self.raw + zlib.crc32(self.data).to_bytes(4, "little") + \
            (n & 0xFFFFFFFF).to_bytes(4, "little")

    def expected(self, cap):
        """the raw stream's serial status with a dst of cap bytes: every byte in front of the first fault has to fit"""
        return DST_TOO_SMALL if cap < self.fault_out else self.status


class Builder:
    """blocks appended to one bit stream; the output they stand for is expanded as they are written"""

    def __init__(self):
        self.bw, self.out, self.blocks = W.BitWriter(), bytearray(), []

    def _expand(self, toks):
        out = self.out
        for t in toks:
            if t & W.MATCH:
                ln, d = ((t >> 16) & 0xFF) + 3, (t & 0x7FFF) + 1
                assert d <= len(out)
                if d >= ln:
                    at = len(out) - d
                    out += out[at: at + ln]
                else:
                    for _ in range(ln):
                        out.append(out[-d])
            else:
                out.append(t)

    def dynamic(self, toks, final=False, expand=True):
        """a dynamic block with package-merge's (complete) codes; without a match it still sends a complete distance code
        of two 1-bit codes nobody uses, so that every block start satisfies the strict block-start predicate"""
        self.blocks.append((self.bw.n, len(self.out)))
        ll_f, d_f = W.token_symbols(toks)
        ll = [int(x) for x in W.package_merge(ll_f, 15)]
        dl = [int(x) for x in W.package_merge(d_f, 15)] if d_f.any() else [1, 1] + [0] * 28
        W.write_dynamic(self.bw, toks, ll, dl, final=final)
        if expand:
            self._expand(toks)

    def fixed(self, toks, final=False):
        self.blocks.append((self.bw.n, len(self.out)))
        write_fixed(self.bw, toks, final)
        self._expand(toks)

    def stored(self, data, final=False):
        self.blocks.append((self.bw.n, len(self.out)))
        W.write_stored(self.bw, data, final)
        self.out += bytes(data)

    def case(self, name, **more):
        return Case(name, self.bw.bytes().tobytes(), self.out, self.blocks, **more)


def generations(G, seed, runs=40, run=1, last=20001, mixed=True):
    """32 KiB of random literals (four blocks), then G generations of 32 KiB (the last one: `last` bytes), each a copy of the
    bytes one window back through matches of up to 258 bytes at distances from FAR, except `runs` runs of `run` fresh
    random literals at places that change with every generation.  A generation is cut into 1 to 4 blocks in front of
    matches, and the match a block starts with is at distance 32768.  mixed: some blocks are fixed ones, and now and then
    a stored block of fresh bytes follows a generation (so the generations do not stay aligned to the window either)."""
    rng = np.random.default_rng(seed)
    b = Builder()
    first = rng.integers(0, 256, WIN, dtype=np.uint8)
    for q in range(4):
        b.dynamic([int(x) for x in first[q * 8192: (q + 1) * 8192]])
    for g in range(1, G + 1):
        n = last if g == G else WIN
        base = len(b.out)
        mask = np.zeros(n + 1, bool)
        mask[n] = True
        for s in rng.integers(0, n, runs):
            mask[s: min(s + run, n)] = True
        nxt = np.minimum.accumulate(np.where(mask, np.arange(n + 1), n)[::-1])[::-1]  # the next fresh position from p on
        fresh = rng.integers(0, 256, n, dtype=np.uint8)
        toks, p, at_match = [], 0, []
        while p < n:
            room = int(nxt[p]) - p
            if room == 0:
                toks.append(int(fresh[p]))
                p += 1
            elif room < 3:
                toks.append(b.out[base + p - WIN])  # (too short for a match: the same byte as a literal)
                p += 1
            else:
                ln = min(room, 258 if rng.integers(0, 4) else int(rng.integers(3, 259)))
                if 0 < room - ln < 3 and room <= 258:
                    ln = room
                at_match.append(len(toks))
                toks.append(W.match(ln, FAR[int(rng.integers(0, 3))]))
                p += ln
        nb = int(rng.integers(1, 5))
        cuts = sorted({int(c) for c in rng.choice(at_match[1:], nb - 1, replace=False)}) if nb > 1 else []
        for c in cuts + ([0] if at_match and at_match[0] == 0 else []):
            toks[c] = W.match(((toks[c] >> 16) & 0xFF) + 3, 32768)
        edges = [0] + cuts + [len(toks)]
        for j in range(len(edges) - 1):
            part = toks[edges[j]: edges[j + 1]]
            fin = g == G and j == len(edges) - 2
            if mixed and g % 5 == 2 and j == 1:
                b.fixed(part, fin)
            else:
                b.dynamic(part, fin)
        if mixed and g % 7 == 3 and g != G:
            b.stored(rng.integers(0, 256, 200 + g, dtype=np.uint8).tobytes())
    return b.case(f"generations-{G}-{run}")


def sized_block(rng, n, lits=600):
    """tokens of n output bytes: a 258-byte match at distance 32768, then matches at FAR and at distance 1 around about
    `lits` fresh literals (all of the rest, when n is small)"""
    toks, left = [W.match(258, 32768)], n - 258
    assert left >= 0
    budget = min(lits, left)
    per = -(-budget // max(1, (left - budget) // 258))
    while left:
        k = min(per, budget, left)
        toks += [int(x) for x in rng.integers(0, 256, k)]
        budget -= k
        left -= k
        if left >= 3:
            ln = min(left, 258 if rng.integers(0, 3) else int(rng.integers(3, 259)))
            if 0 < left - ln < 3:
                ln = left if left <= 258 else ln - 3
            toks.append(W.match(ln, (FAR + (1,))[int(rng.integers(0, 4))]))
            left -= ln
        elif budget == 0:
            toks += [int(x) for x in rng.integers(0, 256, left)]
            left = 0
    return toks


SIZED = (700, 32767, 32768, 32769, 3 * 32768 + 5, 700, 32767, 700, 32769, 700, 5 * 32768, 700, 650)


def chunk_sizes(seed, sizes=SIZED):
    """32769 random literals, then one block per entry of `sizes` with exactly that many output bytes (sized_block)"""
    rng = np.random.default_rng(seed)
    b = Builder()
    b.dynamic([int(x) for x in rng.integers(0, 256, WIN + 1)])
    for k, n in enumerate(sizes):
        b.dynamic(sized_block(rng, n), final=k == len(sizes) - 1)
    return b.case("chunk-sizes", sizes=(WIN + 1,) + tuple(sizes))


FAULT_STATUS = {"type3": INVALID_BLOCK_HEADER, "lenmis": LEN_MISMATCH}
CUT_STATUS = INVALID_LIT_OR_LEN  # a stream that ends inside a block's symbols, as the serial decoder answers it
MATCH_LEN = 100


def first_window(seed, pos=None, delta=0, fault=None, fault_block=None, nblocks=30):
    """nblocks blocks of 1000 to 1500 literals below 64 (the same ones for one seed).  pos: a match of MATCH_LEN bytes at
    output position pos with distance pos + delta (delta 0: the farthest legal one; 1: InvalidDistance); it is the first
    token of its block when pos is a block's output offset (see edges()).  fault, in front of block fault_block: "type3"
    (a block header of type 3), "lenmis" (a stored block whose NLEN is wrong), or "cut" (the stream ends in the middle of
    that block).  Blocks behind a fault are written as if nothing had happened: they are there to be parsed, and the
    writer's bytes end in front of the first fault.  -> Case with events: [(output position, status)] in stream order."""
    rng = np.random.default_rng(seed)
    lits = [[int(x) for x in rng.integers(0, 64, s)] for s in rng.integers(1000, 1501, nblocks)]
    b = Builder()
    events, frozen, cut_at, where, o = [], None, None, pos, 0  # o: the output offset as if nothing failed
    for k in range(nblocks):
        toks = lits[k]
        if fault in ("type3", "lenmis") and k == fault_block:
            b.bw.put(0, 1)
            if fault == "type3":
                b.bw.put(3, 2)
            else:
                b.bw.put(0, 2)
                b.bw.align()
                b.bw.put(50, 16)
                b.bw.put(50 ^ 0xFFFE, 16)
                b.bw.put(int.from_bytes(bytes(range(50)), "little"), 400)
            events.append((o, FAULT_STATUS[fault]))
            frozen = bytes(b.out) if frozen is None else frozen
        if pos is not None and o <= pos < o + len(toks):
            toks = toks[: pos - o] + [W.match(MATCH_LEN, pos + delta)] + toks[pos - o:]
            if delta > 0:
                events.append((pos, INVALID_DISTANCE))
                frozen = bytes(b.out) + bytes(toks[: pos - o]) if frozen is None else frozen
            pos = None
        start = b.bw.n
        b.dynamic(toks, final=k == nblocks - 1, expand=frozen is None)
        b.blocks[-1] = (start, o)
        o += len(toks) + (MATCH_LEN - 1) * (len(toks) > len(lits[k]))
        if fault == "cut" and k == fault_block:
            cut_at = (start + b.bw.n) // 16
            if not events:  # (where the serial decoder stops inside the cut block: its own count)
                st, w, got = H.serial(b.bw.bytes().tobytes()[:cut_at], "raw", 1 << 20)
                assert st != OK
                events.append((w, CUT_STATUS))
                frozen = bytes(b.out[:w])
    raw = b.bw.bytes().tobytes()
    c = Case(f"first-window-{seed}-{where}-{delta}-{fault}-{fault_block}", raw if cut_at is None else raw[:cut_at],
             b.out if frozen is None else frozen, b.blocks, events=events, cut=cut_at)
    if events:
        c.fault_out, c.status = events[0]
    return c


def edges(seed, nblocks=30):
    """output offsets of first_window's blocks while no match has been put in front of them"""
    rng = np.random.default_rng(seed)
    return [0] + [int(x) for x in np.cumsum(rng.integers(1000, 1501, nblocks))]


def predict(case, S):
    """The chunk partition of the stream decoder with nominal chunks of S stream bytes: chunk 0 at bit 0, then the first
    candidate of the strict predicate in every nominal chunk (as the library's driver picks them).  -> dict: picks (bits), false (the
    picks that are no block start), bases (O_i of the picks that are block starts), outs (their chunks' output bytes)"""
    raw = case.raw
    starts = dict(case.blocks)
    cands = np.asarray(H.scan(raw), np.uint64)
    bits, nc = 8 * len(raw), max(1, -(-len(raw) // S))
    picks = [0]
    for c in range(1, nc):
        lo, hi = 8 * c * S, min(8 * (c + 1) * S, bits)
        k = int(np.searchsorted(cands, lo))
        if k < len(cands) and int(cands[k]) < hi:
            picks.append(int(cands[k]))
    false = [p for p in picks if p not in starts]
    bases = [starts[p] for p in picks if p in starts]
    outs = [int(x) for x in np.diff(bases + [case.n])]
    return {"picks": picks, "false": false, "bases": bases, "outs": outs, "confirmed": len(picks), "longest_chunk": max(outs)}


# ---- the cases both modules run (built once per process) ----

_CACHE = {}


def cached(key, fn, *a, **kw):
    if key not in _CACHE:
        _CACHE[key] = fn(*a, **kw)
    return _CACHE[key]


def gens40():
    """G = 40: about 55 KB of stream, 1.3 MB of output, 47 chunks at S = 512"""
    return cached("gens40", generations, 40, 1)


def rich():
    """the literal-rich variant: 12 generations with 40 runs of 300 fresh literals each, 160 KB of stream: 10 chunks (3 groups)
    on a default context"""
    return cached("rich", generations, 12, 2, runs=40, run=300)


def sizes():
    return cached("sizes", chunk_sizes, 3)


FW_SEED = 5
FAULT_BLOCKS = {"behind": 20, "front": 4}  # the second fault's block; the bad distance sits in block 12


def places():
    """name -> output position of first_window's match: in the first chunk, in a middle chunk and in the last chunk that
    ends before 32 KiB (at S = 512 every block but the last is a chunk), as a block's first token and in its middle, and
    the two positions next to 32768 itself"""
    e = edges(FW_SEED)
    last = max(k for k in range(len(e) - 1) if e[k + 1] + MATCH_LEN <= WIN)
    return {"first-mid": e[0] + 500, "middle-token0": e[12], "middle-mid": e[12] + 611, "last-token0": e[last],
            "last-mid": e[last] + 300, "at-32768": WIN, "at-32767": WIN - 1}


def window_cases():
    """[(name, Case)]: dist == out_pos (Success) and dist == out_pos + 1 (InvalidDistance) at every place; at-32768 /
    at-32767 are the two that a 32768 distance allows"""
    out = []
    for name, pos in places().items():
        for delta in (0, 1):
            if (name, delta) in (("at-32768", 1), ("at-32767", 0)):
                continue
            if name == "at-32767":  # (dist 32768 at out_pos 32767)
                pos, delta = WIN - 1, 1
            key = f"{name}-{'bad' if delta else 'ok'}"
            out.append((key, cached(key, first_window, FW_SEED, pos=pos, delta=delta)))
    return out


def fault_cases():
    """[(name, Case)]: a bad (and, for comparison, a legal) distance in block 12 with a second fault in a later and in an
    earlier chunk, and each second fault alone in the last block"""
    out = []
    pos = places()["middle-mid"]
    for fault in ("type3", "lenmis", "cut"):
        for where, blk in FAULT_BLOCKS.items():
            for delta in (1, 0):
                key = f"{'bad' if delta else 'ok'}-dist-{fault}-{where}"
                out.append((key, cached(key, first_window, FW_SEED, pos=pos, delta=delta, fault=fault, fault_block=blk)))
        key = f"{fault}-last-block"
        out.append((key, cached(key, first_window, FW_SEED, fault=fault, fault_block=29)))
    return out


def clean_window():
    return cached("clean-window", first_window, FW_SEED)


def capacities(case):
    """dst capacities for a first_window case: the whole output and one less, the first fault's (or the match's) position
    and one either side, the base offsets of two chunks (S = 512 on the clean stream: the one holding the middle match and
    the one in front of the earlier fault) and one either side, and one far above everything"""
    clean = clean_window()
    n = clean.n + MATCH_LEN
    bases = predict(clean, 512)["bases"]
    marks = {n, n - 1, 1 << 20}
    for p in (case.fault_out, places()["middle-mid"], bases[12], bases[FAULT_BLOCKS["front"]], bases[FAULT_BLOCKS["front"] + 1]):
        marks |= {p - 1, p, p + 1}
    return sorted(marks)
