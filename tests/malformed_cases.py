"""Malformed DEFLATE segments, one per exit of the serial decoder (include/starflate/decompress.hpp), for the tests of
the indexed decoders (tests/test_malformed_core_host.py on the CPU, tests/test_gpu_malformed.py on the GPU).

TEST INFRASTRUCTURE ONLY.  Built over deflate_writer's BitWriter and block writers.

THE RULE the tests state.  The judge is container.hpp's decompress compiled for the host (stream_host.serial(stream, "raw",
cap)).  For a segment that must yield out_n bytes, let (s, w) be the judge's answer on the segment's bytes alone with a
capacity of out_n.  The indexed decoders must report s, except where a segment is not a stream (starflate_hip.h):
  * s == 0 with w < out_n is SrcTooSmall: the index promised more;
  * a segment of well-formed non-final blocks whose bits end between two blocks (the judge: InvalidBlockHeader) is Success
    if w == out_n, else SrcTooSmall -- the generator labels these segments (`boundary`), it never guesses them;
  * a segment of zero bytes is InvalidBlockHeader.
Every malformed segment here is built so that its error lies before its end or its last block is final: the judge's answer
then applies as it is.  And no byte outside [seg_begin, seg_end) may change the status.

Every class starts on a byte boundary (a segment's first bit, or the bit behind a stored block), so its layout and the
byte at which a truncating class is cut do not depend on what precedes it.  A class is a function of a Ctx that writes the
damaged block (final unless the error comes first) and returns how many output bytes the index promises beyond those the
serial decoder writes before it stops; `hint` is the status the class was built for, asserted against the judge on the CPU
so that a class cannot silently turn into another."""
import numpy as np

import deflate_writer as W

OK, ERROR, BAD_HEADER, LEN_MISMATCH, DST_SMALL, SRC_SMALL, BAD_LITLEN, BAD_DIST = range(8)
SEG = W.SEGMENT
SLACK = 300  # output a class that never gets that far is promised anyway


def rule(judge, seg_bytes, out_n, boundary=False):
    """the status the indexed decoders owe a segment -> (status, judge's status, bytes the judge wrote, its output)"""
    if len(seg_bytes) == 0:
        return BAD_HEADER, BAD_HEADER, 0, np.zeros(0, np.uint8)
    s, w, dst = judge(np.asarray(seg_bytes, np.uint8), "raw", out_n)
    if boundary:
        assert s == BAD_HEADER, s
        return (OK if w == out_n else SRC_SMALL), s, w, dst
    if s == OK and w < out_n:
        return SRC_SMALL, s, w, dst
    return s, s, w, dst


# ---- fixed blocks, symbol by symbol ----

def fx(bw, sym):  # RFC 1951 3.2.6
    if sym < 144:
        bw.put_code(0x30 + sym, 8)
    elif sym < 256:
        bw.put_code(0x190 + sym - 144, 9)
    elif sym < 280:
        bw.put_code(sym - 256, 7)
    else:
        bw.put_code(0xC0 + sym - 280, 8)


def fx_len(bw, length):
    s, ne, ev = W.len_symbol(length)
    fx(bw, s)
    bw.put(ev, ne)


def fx_dist(bw, dist):
    ds, de, dv = W.dist_symbol(dist)
    bw.put_code(ds, 5)
    bw.put(dv, de)


def fixed_block(bw, tokens, final=False):
    bw.put(int(final), 1)
    bw.put(1, 2)
    for t in np.asarray(tokens, np.uint32).tolist():
        if t & W.MATCH:
            fx_len(bw, ((t >> 16) & 0xFF) + 3)
            fx_dist(bw, (t & 0x7FFF) + 1)
        else:
            fx(bw, t)
    fx(bw, 256)


# ---- dynamic headers, item by item ----

CL = {0: 2, 1: 2, 18: 2, 2: 3, 16: 3}  # a complete code-length code


def zeros(n):
    items = []
    while n >= 11:
        c = min(n, 138)
        items.append((18, c - 11))
        n -= c
    return items + [(0, 0)] * n


def dyn_raw(bw, final, hlit_field, hdist_field, items, cl=CL):
    """header bits of a dynamic block; items: (code-length symbol, extra value).  -> bit offsets (HLIT, first code-length
    length, first item)"""
    bw.put(int(final), 1)
    bw.put(2, 2)
    a = bw.n
    bw.put(hlit_field, 5)
    bw.put(hdist_field, 5)
    bw.put(15, 4)
    b = bw.n
    for s in W.CL_ORDER:
        bw.put(cl.get(s, 0), 3)
    c = bw.n
    codes = W.canonical([cl.get(s, 0) for s in range(19)])
    for s, e in items:
        bw.put_code(codes[s], cl[s])
        if s >= 16:
            bw.put(e, (2, 3, 7)[s - 16])
    return a, b, c


# literal 0 and end-of-block, one bit each ('0' and '1'); no distance code
LL_TINY = [(1, 0)] + zeros(255) + [(1, 0)]


class Ctx:
    def __init__(self, bw, out):
        self.bw, self.out = bw, out  # out: the segment's good output so far (bytearray)
        self.w = len(out)            # bytes the serial decoder has written when it stops
        self.cut = None              # stream byte at which the segment is cut

    def lit(self, sym):
        fx(self.bw, sym)
        self.w += 1

    def pad9(self, mod):  # 9-bit literals until the next bit is bit `mod` of its byte
        while self.bw.n % 8 != mod:
            self.lit(200)

    def cut_in(self, a, b=None):  # cut at the first byte boundary inside the bit field [a, b)
        k = a // 8 + 1
        assert a < 8 * k and (b is None or 8 * k < b), (a, b)
        self.cut = k


def _hdr(c, final, btype):
    c.bw.put(final, 1)
    c.bw.put(btype, 2)


# ---- the classes ----

def c_btype3(c):
    _hdr(c, 1, 3)
    return 0


def c_stored_nlen(c):
    _hdr(c, 1, 0)
    c.bw.align()
    c.bw.put(4, 16)
    c.bw.put(4 ^ 0xFFFF ^ 0x0100, 16)
    c.bw.put(0x64756272, 32)
    return 4


def c_stored_cut_len(c):
    _hdr(c, 1, 0)
    c.bw.align()
    a = c.bw.n
    c.bw.put(4, 16)
    c.cut_in(a, a + 16)
    return 4


def c_stored_cut_nlen(c):
    _hdr(c, 1, 0)
    c.bw.align()
    c.bw.put(4, 16)
    a = c.bw.n
    c.bw.put(4 ^ 0xFFFF, 16)
    c.cut_in(a, a + 16)
    return 4


def c_stored_cut_header(c):
    a = c.bw.n
    _hdr(c, 1, 0)
    c.bw.align()
    c.cut = a // 8 + 1  # right behind the byte that holds the header bits
    return 4


def c_stored_cut_payload(c):
    _hdr(c, 1, 0)
    c.bw.align()
    c.bw.put(10, 16)
    c.bw.put(10 ^ 0xFFFF, 16)
    c.bw.put(0x64756272, 32)
    return 10


def c_stored_len_over(c):
    _hdr(c, 1, 0)
    c.bw.align()
    c.bw.put(10, 16)
    c.bw.put(10 ^ 0xFFFF, 16)
    c.bw.put(int.from_bytes(b"0123456789", "little"), 80)
    return 9


def c_dyn_cut_counts(c):
    a, b, _ = dyn_raw(c.bw, 1, 0, 0, LL_TINY + [(0, 0)])
    c.cut_in(a + 5, b)  # inside HDIST or HCLEN
    return SLACK


def c_dyn_cut_cl(c):
    _, b, cc = dyn_raw(c.bw, 1, 0, 0, LL_TINY + [(0, 0)])
    c.cut_in(b + 8, cc)
    return SLACK


def c_dyn_cut_seq_code(c):
    # items of two bits each from an even bit on: the byte boundary lies between two codes, where the code-length
    # decoder finds no bit at all
    _, _, cc = dyn_raw(c.bw, 1, 0, 0, [(1, 0)] * 40)
    c.cut_in(cc + 16)
    return SLACK


def c_dyn_cut_seq_code_inside(c):
    # three-bit items: some byte boundary falls inside one
    _, _, cc = dyn_raw(c.bw, 1, 0, 0, [(2, 0)] * 40)
    k = next(k for k in range(cc // 8 + 1, cc // 8 + 8) if (8 * k - cc) % 3)
    c.cut = k
    return SLACK


def c_dyn_cut_seq_extra(c):
    # a run of 138 zeros: two code bits and seven extra bits, cut inside the extra bits
    bw = c.bw
    codes = W.canonical([CL.get(s, 0) for s in range(19)])
    dyn_raw(bw, 1, 0, 0, [(1, 0)])
    if bw.n % 2 == 0:
        bw.put_code(codes[2], 3)  # a three-bit item: the two-bit ones below then end on odd bits
    while (bw.n + 2) % 8 != 7:  # single lengths until the extra bits start on bit 7 of a byte
        bw.put_code(codes[1], 2)
    bw.put_code(codes[18], 2)
    a = bw.n
    bw.put(127, 7)
    c.cut_in(a, a + 7)
    return SLACK


def c_cl_oversubscribed(c):
    bw = c.bw
    _hdr(c, 1, 2)
    bw.put(0, 5)
    bw.put(0, 5)
    bw.put(0, 4)
    for v in (1, 1, 1, 0):  # three one-bit codes
        bw.put(v, 3)
    bw.put(0xFFFF, 16)
    bw.put(0xFFFF, 16)
    return SLACK


def c_cl_unassigned(c):
    cl = {0: 1, 1: 2}  # '0' and '10': nothing is '11'
    dyn_raw(c.bw, 1, 0, 0, [(1, 0), (0, 0)], cl)
    c.bw.put(3, 2)
    c.bw.put(0xFFFF, 16)
    return SLACK


def c_rep_at_ll0(c):
    dyn_raw(c.bw, 1, 0, 0, [(16, 0)] + LL_TINY)
    c.bw.put(0, 16)
    return SLACK


def c_rep_at_d0(c):
    # the last literal/length length is 1, and three distance lengths repeat it: Error for the serial decoder, which reads
    # two sequences, and an over-subscribed distance code for a decoder that reads one (RFC 1951 3.2.7), zlib included
    dyn_raw(c.bw, 1, 0, 2, LL_TINY + [(16, 0)])
    c.bw.put(0, 16)
    return SLACK


def c_run_past_end(c):
    dyn_raw(c.bw, 1, 0, 0, [(1, 0), (18, 127), (18, 127)])
    c.bw.put(0, 16)
    return SLACK


def c_ll_oversubscribed(c):
    dyn_raw(c.bw, 1, 0, 0, [(1, 0), (1, 0)] + zeros(254) + [(1, 0), (0, 0)])
    c.bw.put(0, 16)
    return SLACK


def c_d_oversubscribed(c):
    dyn_raw(c.bw, 1, 0, 2, LL_TINY + [(1, 0)] * 3)
    c.bw.put(0, 16)
    return SLACK


def c_no_eob(c):
    # literals 0 and 1 take the whole code space: symbols until the bits run out, then no code
    dyn_raw(c.bw, 1, 0, 0, [(1, 0), (1, 0)] + zeros(255) + [(0, 0)])
    c.bw.put(0x5A5A, 16)
    return SLACK


def c_all_zero(c):
    dyn_raw(c.bw, 1, 0, 0, zeros(257) + [(0, 0)])  # (no run across the two sequences)
    c.bw.put(0, 16)
    return SLACK


def _accepted(hlit_field, hdist_field):
    def f(c):
        # literal 0 and end-of-block, a one-bit distance code that is not used: '0' '1'
        dyn_raw(c.bw, 1, hlit_field, hdist_field, LL_TINY + zeros(hlit_field) + [(1, 0)] + zeros(hdist_field))
        c.bw.put(0b10, 2)
        c.w += 1
        c.out.append(0)
        return 0
    return f


def c_ll_unassigned(c):
    # literal 0 '0', end-of-block '10': nothing is '11'
    dyn_raw(c.bw, 1, 0, 0, [(1, 0)] + zeros(255) + [(2, 0), (0, 0)])
    c.bw.put(0, 1)
    c.w += 1
    c.bw.put(3, 2)
    c.bw.put(0xFFFF, 16)
    return SLACK


def _fixed_bad_ll(sym):
    def f(c):
        _hdr(c, 1, 1)
        c.lit(ord("a"))
        fx(c.bw, sym)
        c.bw.put(0, 16)
        return SLACK
    return f


def c_len_no_dist(c):
    # literal 0 '0', end-of-block '10', length 3 '11'; no distance code at all
    dyn_raw(c.bw, 1, 1, 0, [(1, 0)] + zeros(255) + [(2, 0), (2, 0), (0, 0)])
    c.bw.put(0, 1)
    c.w += 1
    c.bw.put(3, 2)
    c.bw.put(0, 16)
    return SLACK


def c_d_unassigned(c):
    # ... and one distance code, '0': nothing is '1'
    dyn_raw(c.bw, 1, 1, 0, [(1, 0)] + zeros(255) + [(2, 0), (2, 0), (1, 0)])
    c.bw.put(0, 1)
    c.w += 1
    c.bw.put(3, 2)
    c.bw.put(1, 1)
    c.bw.put(0xFFFF, 16)
    return SLACK


def _fixed_bad_d(dsym):
    def f(c):
        _hdr(c, 1, 1)
        c.lit(ord("a"))
        fx(c.bw, 257)
        c.bw.put_code(dsym, 5)
        fx(c.bw, 256)
        c.bw.put(0, 16)
        return SLACK
    return f


def c_too_far(c, hist=0):
    _hdr(c, 1, 1)
    c.lit(ord("a"))
    fx(c.bw, 257)
    fx_dist(c.bw, c.w + hist + 1)  # one beyond the bytes written
    fx(c.bw, 256)
    return 3


def c_cut_ll_code(c):
    _hdr(c, 1, 1)
    c.pad9(7)
    a = c.bw.n
    fx(c.bw, 200)
    c.cut_in(a, a + 9)
    return SLACK


def c_cut_len_extra(c):
    _hdr(c, 1, 1)
    c.lit(ord("a"))
    c.pad9(7)
    fx(c.bw, 281)  # eight code bits, then five extra bits
    a = c.bw.n
    c.bw.put(31, 5)
    c.cut_in(a, a + 5)
    return SLACK


def c_cut_d_code(c):
    _hdr(c, 1, 1)
    c.lit(ord("a"))
    c.pad9(0)
    fx(c.bw, 257)
    a = c.bw.n
    c.bw.put_code(0, 5)
    c.cut_in(a, a + 5)
    return SLACK


def c_cut_d_extra(c):
    _hdr(c, 1, 1)
    c.lit(ord("a"))
    fx(c.bw, 257)
    c.bw.put_code(20, 5)  # nine extra bits
    a = c.bw.n
    c.bw.put(0x1FF, 9)
    c.cut_in(a, a + 9)
    return SLACK


def c_lit_too_many(c):
    _hdr(c, 1, 1)
    c.lit(ord("a"))
    fx(c.bw, ord("b"))
    fx(c.bw, 256)
    return 0


def c_match_crosses_end(c):
    _hdr(c, 1, 1)
    c.lit(ord("a"))
    fx_len(c.bw, 10)
    fx_dist(c.bw, 1)
    fx(c.bw, 256)
    return 9


def c_ends_short(c):
    _hdr(c, 1, 1)
    c.lit(ord("a"))
    c.lit(ord("b"))
    fx(c.bw, 256)
    return 1


# (name, writer, the status it was built for)
CLASSES = [
    ("btype3", c_btype3, BAD_HEADER),
    ("stored_nlen_mismatch", c_stored_nlen, LEN_MISMATCH),
    ("stored_cut_in_len", c_stored_cut_len, ERROR),
    ("stored_cut_in_nlen", c_stored_cut_nlen, ERROR),
    ("stored_cut_behind_header", c_stored_cut_header, ERROR),
    ("stored_payload_cut", c_stored_cut_payload, SRC_SMALL),
    ("stored_len_over_capacity", c_stored_len_over, DST_SMALL),
    ("dyn_cut_in_counts", c_dyn_cut_counts, ERROR),
    ("dyn_cut_in_cl_lengths", c_dyn_cut_cl, ERROR),
    ("dyn_cut_between_length_codes", c_dyn_cut_seq_code, BAD_LITLEN),
    ("dyn_cut_in_length_code", c_dyn_cut_seq_code_inside, BAD_LITLEN),
    ("dyn_cut_in_run_extra", c_dyn_cut_seq_extra, ERROR),
    ("cl_oversubscribed", c_cl_oversubscribed, ERROR),
    ("cl_unassigned_pattern", c_cl_unassigned, BAD_LITLEN),
    ("repeat_at_ll_index0", c_rep_at_ll0, ERROR),
    ("repeat_at_d_index0", c_rep_at_d0, ERROR),
    ("run_past_last_length", c_run_past_end, ERROR),
    ("ll_oversubscribed", c_ll_oversubscribed, ERROR),
    ("d_oversubscribed", c_d_oversubscribed, ERROR),
    ("no_end_of_block_code", c_no_eob, BAD_LITLEN),
    ("all_lengths_zero", c_all_zero, BAD_LITLEN),
    ("hlit_287_accepted", _accepted(30, 0), OK),
    ("hlit_288_accepted", _accepted(31, 0), OK),
    ("hdist_31_accepted", _accepted(0, 30), OK),
    ("hdist_32_accepted", _accepted(0, 31), OK),
    ("ll_unassigned_code", c_ll_unassigned, BAD_LITLEN),
    ("ll_symbol_286", _fixed_bad_ll(286), BAD_LITLEN),
    ("ll_symbol_287", _fixed_bad_ll(287), BAD_LITLEN),
    ("length_without_distance_code", c_len_no_dist, BAD_DIST),
    ("d_unassigned_code", c_d_unassigned, BAD_DIST),
    ("d_symbol_30", _fixed_bad_d(30), BAD_LITLEN),
    ("d_symbol_31", _fixed_bad_d(31), BAD_LITLEN),
    ("distance_too_far", c_too_far, BAD_DIST),
    ("cut_in_ll_code", c_cut_ll_code, BAD_LITLEN),
    ("cut_in_length_extra", c_cut_len_extra, ERROR),
    ("cut_in_d_code", c_cut_d_code, BAD_DIST),
    ("cut_in_d_extra", c_cut_d_extra, ERROR),
    ("one_literal_too_many", c_lit_too_many, DST_SMALL),
    ("match_crosses_end", c_match_crosses_end, DST_SMALL),
    ("final_block_ends_short", c_ends_short, SRC_SMALL),
]
ACCEPTED = {n for n, _, h in CLASSES if h == OK}               # the reference accepts HLIT 287/288 and HDIST 31/32; zlib does not
ZLIB_KNOWN = {"ll_unassigned_code"}                              # (an incomplete literal/length code: zlib refuses its header as well)
HEADER_CLASSES = [n for n, _, _ in CLASSES[:25]]                 # refused (or accepted) before the first symbol


# ---- good blocks ----

def _tokens_for(n, rng, have):
    """tokens for exactly n bytes; have: bytes of the segment before them (matches stay inside the block)"""
    toks, made = [], 0
    while made < min(n, 24):
        toks.append(int(rng.integers(97, 105)))
        made += 1
    while n - made >= 3:
        ln = int(min(258, n - made, rng.integers(3, 259)))
        toks.append(W.match(ln, int(rng.integers(1, min(made, 32768) + 1))))
        made += ln
    toks += [int(rng.integers(97, 105)) for _ in range(n - made)]
    return toks


def good_fill(c, n, rng):
    """good non-final blocks for exactly n bytes: a dynamic, a fixed and a stored block (n > 2100; fewer kinds below that),
    the stored one last, so that what follows starts on a byte"""
    if n == 0:
        return
    n_st = min(n, 1500)
    n_fx = min(n - n_st, 600)
    n_dy = n - n_st - n_fx
    if n_dy:
        toks = _tokens_for(n_dy, rng, len(c.out))
        t, ll, dl, _ = W.huffman_block(toks)
        W.write_dynamic(c.bw, t, ll, dl)
        c.out += W.expand(toks, bytes(c.out))
    if n_fx:
        toks = _tokens_for(n_fx, rng, len(c.out))
        fixed_block(c.bw, toks)
        c.out += W.expand(toks, bytes(c.out))
    data = rng.integers(0, 256, n_st, dtype=np.uint8).tobytes()
    W.write_stored(c.bw, data)
    c.out += data
    c.w = len(c.out)


class Case:
    """One stream with one segment under test.  stream: the bytes; idx: the segment index (byte offsets, nseg + 1); total:
    output bytes the index promises (every segment but the last SEG of them); seg: the segment under test, [lo, hi) its
    stream bytes and out_n its promise; good: {segment: its output bytes} of the good neighbours; head: the good output
    of the segment under test that precedes its damage; hint: the status the class was built for (None: not stated)."""

    def __init__(self, name, stream, idx, total, seg, out_n, hint, good=None, head=b"", boundary=False, cls=None, place=None):
        self.name, self.stream, self.idx, self.total, self.seg, self.out_n = name, np.asarray(stream, np.uint8), idx, total, seg, out_n
        self.hint, self.good, self.head, self.boundary, self.cls, self.place = hint, good or {}, bytes(head), boundary, cls, place
        self.lo, self.hi = idx[seg], idx[seg + 1]

    def __iter__(self):  # (name, stream, out_n)
        return iter((self.name, self.segment(), self.out_n))

    def segment(self):
        return self.stream[self.lo:self.hi]


def _need(writer):
    c = Ctx(W.BitWriter(), bytearray())
    extra = writer(c)
    return c.w + extra


def _bad_segment(writer, out_n, prefix, rng, tail=None):
    """-> (segment bytes, out_n, head bytes).  prefix: list of good_fill sizes; out_n None: what prefix and class make, else the
    first fill is stretched so that the segment promises exactly out_n."""
    need = _need(writer)
    if out_n is not None:
        prefix = [out_n - need - sum(prefix[1:])] + prefix[1:] if prefix else [out_n - need]
        assert prefix[0] >= 0
    c = Ctx(W.BitWriter(), bytearray())
    for n in prefix:
        good_fill(c, n, rng)
    assert c.bw.n % 8 == 0
    w0 = c.w
    head = bytes(c.out)
    extra = writer(c)
    assert c.w - w0 + extra == need, "a class's layout must not depend on what precedes it"
    if tail:
        tail(c)
    seg = c.bw.bytes()
    if c.cut is not None:
        assert c.cut <= len(seg)
        seg = seg[: c.cut]
    return seg, c.w + extra, head + bytes(c.out[len(head):])


def class_behind(writer, head=b"", tail=None, final=True):
    """a class written from a byte boundary behind good blocks whose output is `head` -> (its stream bytes, cut where the class
    cuts; the output the class promises, head included; the good output in front of its damage).  final False: the class's
    block header says "not final" (every class writes BFINAL as its first bit), for a class with more blocks behind it."""
    c = Ctx(W.BitWriter(), bytearray(head))
    extra = writer(c)
    if tail:
        tail(c)
    seg = c.bw.bytes()
    if c.cut is not None:
        assert c.cut <= len(seg)
        seg = seg[: c.cut]
    if not final:
        assert seg[0] & 1
        seg[0] &= 0xFE
    return seg, c.w + extra, bytes(c.out)


def _good_segment(n, rng, final):
    c = Ctx(W.BitWriter(), bytearray())
    if final:  # a stream's last segment as a compressor leaves it: one final dynamic block
        toks = _tokens_for(n, rng, 0)
        t, ll, dl, _ = W.huffman_block(toks)
        W.write_dynamic(c.bw, t, ll, dl, final=True)
        c.out += W.expand(toks)
    else:
        good_fill(c, n, rng)
    return c.bw.bytes(), bytes(c.out)


def _single(name, seg, out_n, hint, head, **kw):
    return Case(name, seg, [0, len(seg)], out_n, 0, out_n, hint, head=head, **kw)


def _btype3_tail(c):
    c.bw.put(1, 1)
    c.bw.put(3, 2)


def class_cases(seed=11):
    """every class in placements (a), (b), (c) and (e) [the real next segment behind it], plus (d), (f), the empty segment
    and the boundary segments"""
    rng = np.random.default_rng(seed)
    g0, out0 = _good_segment(SEG, rng, final=False)
    g2, out2 = _good_segment(700, rng, final=True)
    cases = []
    for name, writer, hint in CLASSES:
        seg, out_n, head = _bad_segment(writer, None, [], rng)
        cases.append(_single(name + "/a", seg, out_n, hint, head, cls=name, place="a"))
        seg, out_n, head = _bad_segment(writer, None, [20000], rng)
        cases.append(_single(name + "/b", seg, out_n, hint, head, cls=name, place="b"))
        seg, out_n, head = _bad_segment(writer, None, [3000, 2500, 2200], rng)
        cases.append(_single(name + "/c", seg, out_n, hint, head, cls=name, place="c"))
        seg, out_n, head = _bad_segment(writer, SEG, [0], rng)
        stream = np.concatenate([g0, seg, g2])
        idx = [0, len(g0), len(g0) + len(seg), len(stream)]
        cases.append(Case(name + "/e", stream, idx, 2 * SEG + len(out2), 1, SEG, hint, good={0: out0, 2: out2}, head=head,
                          cls=name, place="e"))
    # (d) two errors in one segment: the earlier one counts
    for pre, tag in (([], "a"), ([20000], "b")):
        seg, out_n, head = _bad_segment(c_too_far_nonfinal, None, pre, rng, tail=_btype3_tail)
        cases.append(_single("too_far_then_btype3/d" + tag, seg, out_n, BAD_DIST, head, cls="two_errors", place="d"))
    # (f) the middle and the last segment malformed, with different statuses: the middle one counts
    seg, out_n, head = _bad_segment(c_stored_nlen, SEG, [0], rng)
    last, _, _ = _bad_segment(c_btype3, None, [], rng)
    stream = np.concatenate([g0, seg, last])
    cases.append(Case("nlen_mismatch_then_btype3/f", stream, [0, len(g0), len(g0) + len(seg), len(stream)], 2 * SEG + 5, 1, SEG,
                      LEN_MISMATCH, good={0: out0}, head=head, cls="two_segments", place="f"))
    # a segment of zero bytes, alone and between good neighbours
    cases.append(Case("empty/a", np.zeros(0, np.uint8), [0, 0], 0, 0, 0, BAD_HEADER, cls="empty", place="a"))
    stream = np.concatenate([g0, g2])
    cases.append(Case("empty/e", stream, [0, len(g0), len(g0), len(stream)], 2 * SEG + len(out2), 1, SEG, BAD_HEADER,
                      good={0: out0, 2: out2}, cls="empty", place="e"))
    # the exception the generator labels: non-final blocks that end on the segment's last bit, full and short
    cases.append(Case("boundary_full", g0, [0, len(g0)], SEG, 0, SEG, OK, head=out0, boundary=True, cls="boundary", place="a"))
    gs, outs = _good_segment(5000, rng, final=False)
    cases.append(Case("boundary_short", gs, [0, len(gs)], 5001, 0, 5001, SRC_SMALL, head=outs, boundary=True, cls="boundary", place="a"))
    return cases


def c_too_far_nonfinal(c):
    """c_too_far in a block that is not final, so that the BTYPE 3 behind it is a second error of the same segment"""
    _hdr(c, 0, 1)
    c.lit(ord("a"))
    fx(c.bw, 257)
    fx_dist(c.bw, c.w + 1)
    fx(c.bw, 256)
    return 3


def gap_variant(case, seed=3):
    """placement (e) with 64 noise bytes of no segment behind the segment under test: -> (stream, lo, hi)"""
    noise = np.random.default_rng(seed).integers(0, 256, 64, dtype=np.uint8)
    s = np.concatenate([case.stream[: case.hi], noise, case.stream[case.hi:]])
    return s, case.lo, case.hi


# ---- strips: a segment whose matches may reach `hist` bytes before it ----

def strip_cases(seed=5):
    """-> [(name, strip stream, begin of the second segment, hist, out_n of the second segment, hint)]: a distance that
    reaches the strip's first byte, and one beyond it.  Judged on the whole strip."""
    out = []
    for name, beyond, hint in (("strip_reaches_first_byte", 0, OK), ("strip_one_beyond", 1, BAD_DIST)):
        rng = np.random.default_rng(seed)
        c = Ctx(W.BitWriter(), bytearray())
        good_fill(c, 4000, rng)
        lo, hist = c.bw.n // 8, c.w
        _hdr(c, 1, 1)
        c.lit(ord("a"))
        fx(c.bw, 257)
        fx_dist(c.bw, hist + 1 + beyond)
        fx(c.bw, 256)
        out.append((name, c.bw.bytes(), lo, hist, 4, hint))
    return out


# ---- the truncation sweep ----

def sweep_stream(seed=9):
    """one stream of at most 300 bytes that holds a dynamic, a fixed and a stored block -> (stream, output)"""
    rng = np.random.default_rng(seed)
    c = Ctx(W.BitWriter(), bytearray())
    text = rng.integers(97, 105, 330, dtype=np.uint8).tolist()  # eight letters
    toks = text + [W.match(40, 7), W.match(258, 300), W.match(9, 1)]
    t, ll, dl, _ = W.huffman_block(toks)
    W.write_dynamic(c.bw, t, ll, dl)
    c.out += W.expand(toks)
    toks = [int(x) for x in rng.integers(97, 105, 40)] + [W.match(100, 500), 200, 201, W.match(3, 2)]
    fixed_block(c.bw, toks)
    c.out += W.expand(toks, bytes(c.out))
    data = rng.integers(0, 256, 60, dtype=np.uint8).tobytes()
    W.write_stored(c.bw, data, final=True)
    c.out += data
    s = c.bw.bytes()
    assert len(s) <= 300, len(s)
    return s, bytes(c.out)


TRAILERS = ("nothing", "zeros", "ones", "continuation", "noise")


def sweep_cuts():
    """-> (stream, output, [cut byte counts 1 .. len - 1])"""
    s, out = sweep_stream()
    return s, out, list(range(1, len(s)))


def with_trailer(stream, cut, kind, seed=17):
    """the first `cut` bytes of stream with a trailer behind them -> buffer (the segment is its first `cut` bytes)"""
    head = np.asarray(stream[:cut], np.uint8)
    if kind == "nothing":
        return head.copy()
    if kind == "zeros":
        tail = np.zeros(96, np.uint8)
    elif kind == "ones":
        tail = np.full(96, 0xFF, np.uint8)
    elif kind == "continuation":
        tail = np.asarray(stream[cut:], np.uint8)
    else:
        tail = np.random.default_rng(seed + cut).integers(0, 256, 96, dtype=np.uint8)
    return np.concatenate([head, tail])


# ---- the sub-indexed path: one block per segment, 32 regions of 1024 bytes, and damage that keeps every bit offset ----

def sub_fixed_segment(seed=21):
    """One final fixed block of SEG bytes in which no match crosses a region, with its sub-index, and two in-place
    patches of a match's distance code that take the same number of bits, so that the later regions keep their entries.
    -> (segment bytes, sub uint32[32, 2], output, {name: (patched segment, status it was built for)})"""
    rng = np.random.default_rng(seed)
    bw = W.BitWriter()
    bw.put(1, 1)
    bw.put(1, 2)
    sub, out, ntok, spots = [], bytearray(), 0, {}
    for r in range(32):
        sub.append((bw.n, ntok))
        left = W.REGION
        for _ in range(2):
            b = int(rng.integers(97, 105))
            fx(bw, b)
            out.append(b)
            left -= 1
            ntok += 1
        while left:
            if left < 3:
                b = int(rng.integers(97, 105))
                fx(bw, b)
                out.append(b)
                left -= 1
                ntok += 1
                continue
            ln = int(min(258, left, rng.integers(3, 259)))
            first = r == 0 and left == W.REGION - 2
            dist = 1 if first else int(rng.integers(max(1, len(out) // 2), len(out) + 1))
            if r == 5 and "d_symbol_30" not in spots:
                dist = len(out)  # 5122 bytes back: symbol 24, eleven extra bits
            fx_len(bw, ln)
            at = bw.n
            fx_dist(bw, dist)
            if first:
                spots["distance_too_far"] = (at, 3, 0)       # symbol 3 = distance 4 with two bytes written, no extra bits
            elif r == 5 and "d_symbol_30" not in spots:
                spots["d_symbol_30"] = (at, 30, W.dist_symbol(dist)[1])
            for _ in range(ln):
                out.append(out[-dist])
            left -= ln
            ntok += 1
    fx(bw, 256)
    seg = bw.bytes()
    patched = {}
    for name, (at, dsym, extra) in spots.items():
        bits = np.unpackbits(seg, bitorder="little")
        bits[at: at + 5] = [(dsym >> (4 - k)) & 1 for k in range(5)]  # the code goes MSB first
        patched[name] = (np.packbits(bits, bitorder="little"), BAD_LITLEN if dsym == 30 else BAD_DIST)
    assert len(out) == SEG and len(patched) == 2
    return seg, np.array(sub, np.uint32), bytes(out), patched


# ---- a segment's status without a label: is it a run of whole non-final blocks? ----

TERMINATOR = np.array([0x03, 0x00], np.uint8)  # a final fixed block that holds the end-of-block code alone


def rule_auto(judge, seg_bytes, out_n):
    """rule() for a segment nobody labelled (a bit flip in a good stream): the judge's InvalidBlockHeader means 'whole
    non-final blocks, then no header' exactly when the same bytes with a final empty block behind them are a good stream."""
    seg_bytes = np.asarray(seg_bytes, np.uint8)
    if len(seg_bytes) == 0:
        return BAD_HEADER
    s, w, _ = judge(seg_bytes, "raw", out_n)
    if s == BAD_HEADER and judge(np.concatenate([seg_bytes, TERMINATOR]), "raw", out_n)[0] == OK:
        return OK if w == out_n else SRC_SMALL
    return SRC_SMALL if s == OK and w < out_n else s


def first_failing(judge, stream, idx, total, strip_segments=1):
    """the status an indexed decode of the whole stream owes: segment by segment in stream order, each judged on its own
    bytes with its own size -- a later segment of a strip, whose matches may reach the strip's earlier output, on the strip's
    bytes up to its end once the segments before it are known to be good"""
    stream = np.asarray(stream, np.uint8)
    nseg = len(idx) - 1
    for c in range(nseg):
        first = c - c % strip_segments
        out_n = sum(min(SEG, total - k * SEG) for k in range(first, c + 1))
        st = rule_auto(judge, stream[int(idx[first]): int(idx[c + 1])], out_n)
        if st:
            return st
    return OK


# ---- wide rows: a class behind byte 40000 of a 65280-byte BGZF member's body ----

WIDE = 65280
NOT_WIDE = {"distance_too_far"}  # (no distance reaches beyond 32768 bytes, so behind byte 40000 none is too far)


def wide_cases(seed=13):
    """-> [(name, body, hint)]: a raw DEFLATE body that promises WIDE bytes, each class once behind good blocks"""
    rng = np.random.default_rng(seed)
    out = []
    for name, writer, hint in CLASSES:
        if name in NOT_WIDE:
            continue
        seg, out_n, head = _bad_segment(writer, WIDE, [0], rng)
        assert out_n == WIDE and len(head) >= 40000 and len(seg) < 65000
        out.append((name, seg, hint))
    return out


# ---- index-free decode: a flushed three-segment stream with the class in its middle segment ----

MARKER = np.array([0x00, 0x00, 0x00, 0xFF, 0xFF], np.uint8)  # the empty stored block of a flush, from a byte boundary


def any_cases(seed=15):
    """-> [(name, stream, total, end of the middle segment, flushed)].  flushed: the middle segment ends with the flush's empty
    stored block like the other two; a class that cuts its segment short cuts that block off, and the stream is then not
    block-flushed every 32 KiB, which the index-free calls refuse as such (SFH_E_NOT_INDEXABLE)"""
    rng = np.random.default_rng(seed)
    g0, _ = _good_segment(SEG, rng, final=False)
    g2, out2 = _good_segment(700, rng, final=True)
    out = []
    for name, writer, _ in CLASSES:
        seg, out_n, _ = _bad_segment(writer, SEG, [0], rng, tail=write_marker)
        flushed = len(seg) >= 4 and bytes(seg[-4:]) == bytes(MARKER[1:])
        out.append((name, np.concatenate([g0, MARKER, seg, g2]), 2 * SEG + len(out2), len(g0) + 5 + len(seg), flushed))
    return out


def any_rule(judge, stream, total, hi):
    """What the index-free decode owes such a stream -> (status, why).  The judge reads the whole stream.  Where it stops
    inside the middle segment with an error, that error is the answer ("before_end"; DstTooSmall is an error against the
    32768 bytes a segment between two flush points holds, which the whole stream's capacity cannot show, so there the judge
    reads the stream up to the middle segment's end with that capacity).  Where the middle segment's last block is FINAL and
    good, the stream ends inside it: the recovered index's end rule (starflate_hip.h; decode_segment<true>) calls a final
    block in a segment that is not the last Error when the segment is complete, and SrcTooSmall when it ends short
    ("final_inside"); the judge on the whole stream says SrcTooSmall for both, the index promised more."""
    s, w, _ = judge(np.asarray(stream[:hi], np.uint8), "raw", 2 * SEG)
    if s != OK:
        if s != DST_SMALL:
            assert whole_stream_rule(judge, stream, total) == s
        return s, "before_end"
    assert whole_stream_rule(judge, stream, total) == SRC_SMALL
    return (ERROR if w == 2 * SEG else SRC_SMALL), "final_inside"


def write_marker(c):
    W.write_stored_empty(c.bw)


def whole_stream_rule(judge, stream, total):
    s, w, _ = judge(np.asarray(stream, np.uint8), "raw", total)
    return SRC_SMALL if s == OK and w < total else s
