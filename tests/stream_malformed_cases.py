"""Malformed raw DEFLATE streams for the stream decoders (sfh_inflate_stream*, sfh_inflate_stream_batch*): every class of
tests/malformed_cases.py, one per exit of the serial decoder, placed where the stream decoders can get its status wrong --
alone in chunk 0, behind good blocks in a record that started on a speculative candidate, dozens of records in, right behind a
false candidate, as the payload of a good stored stream, and two faults in one stream -- and one stream cut at every byte.
(The CPU side: tests/test_stream_malformed_cases.py; the GPU side: tests/test_gpu_stream_malformed.py.)

TEST INFRASTRUCTURE ONLY.  Built on malformed_cases (CLASSES, Ctx, good_fill, sweep_stream, with_trailer) and deflate_writer;
fixed seeds, nothing on disk, built once per process (stream_cases.cached).

THE JUDGE is never the code under test: every expected status is stream_host.serial(stream, container, cap), container.hpp's
decompress compiled for the host, on the whole stream at the capacity the call is given (Case.judge).  The judge reads a
stream, not a segment, so none of the indexed decoders' exceptions applies: `final_block_ends_short` is a good, shorter
stream here (Success with w < out_n), there being no index that promised more.

Every case is a raw stream.  Placements:
  P0  the class alone: an item of a few bytes, in chunk 0
  M   behind 12 good_fill groups (18.9 KB of stream, 27600 bytes of output: below 32768, so `distance_too_far` can be
      written); with 16384-byte nominal chunks the fault lies in the second record
  L   behind 24 groups (37.8 KB, 55200 bytes), every class but NOT_LONG: with 512-byte nominal chunks the fault lies dozens of
      records in, in the item's last group of chunks; with 16384-byte ones in the third record
  F   one representative per status behind the 12 groups and one more stored block whose payload starts with a look-alike of
      a block start (a dynamic header, and a stored header): the first candidate of its nominal 512-byte chunk, so the record
      that decodes the class started off the chain and has to be repaired first
  D   one good stream of stored blocks whose payload is every L stream, one after the other: every candidate inside is false,
      and its speculative decode runs into a class
  T   two faults: a representative behind the sixth group and BTYPE 3 behind the twelfth, two of them the other way round, and
      a distance one too far (which only the write pass can see) in front of and behind a structural fault
and the truncation sweep: malformed_cases.sweep_stream() cut at every byte, alone and behind the 12 groups, each cut in front
of every trailer kind, and the same stream wrapped as zlib and as gzip with the wrapped file cut at every byte."""
import zlib

import numpy as np

import deflate_writer as W
import malformed_cases as M
import stream_host as H
import stream_lookalikes as LA
import stream_stored_host as SS
from stream_cases import cached

BIG = 1 << 20
FILL = 2300
M_FILLS, L_FILLS = 12, 24
CHUNKS = (512, 16384)
NOT_LONG = {"distance_too_far"}  # (no distance reaches beyond 32768 bytes, so behind 55200 bytes of output none is too far)
BY_NAME = {n: (w, h) for n, w, h in M.CLASSES}
# one class per status, none of them cut short, so that more blocks can follow one
REPS = ("hlit_287_accepted", "cl_oversubscribed", "btype3", "stored_nlen_mismatch", "one_literal_too_many", "stored_payload_cut",
        "ll_symbol_286", "d_unassigned_code")
TERMINATOR = M.TERMINATOR.tobytes()


class Case:
    """name; stream: the raw stream; out_n: the output the writer promises (the capacity a caller would bring); good: the good
    output in front of the (first) fault, the writer's own bytes; w: the bytes the judge writes at capacity BIG; cls, place;
    hint: the status the class was built for (None: the judge alone says); head_n: the output of the good blocks in front of
    the class; at: the stream bit at which the class's block starts; starts: the true block starts in front of it (bits),
    stored: those of them that are stored blocks; look: the bit of the look-alike (F)."""

    def __init__(self, name, stream, out_n, good, cls, place, hint=None, head_n=0, at=0, starts=(0,), stored=(), look=None):
        self.name, self.stream, self.out_n, self.good, self.cls, self.place = name, bytes(stream), out_n, bytes(good), cls, place
        self.hint, self.head_n, self.at, self.starts, self.stored, self.look = hint, head_n, at, tuple(starts), tuple(stored), look
        self._judged = {}
        self.w = self.judge(BIG)[1]

    def judge(self, cap, container="raw", stream=None):
        """-> (status, bytes written, those bytes) of the serial decoder at this capacity (computed once)"""
        key = (cap, container, stream)
        if key not in self._judged:
            st, w, dst = H.serial(self.stream if stream is None else stream, container, cap)
            self._judged[key] = (st, w, dst[: cap if w is None else w].tobytes())
        return self._judged[key]

    def capacities(self):
        """the capacities every single call is tried at"""
        return sorted({c for c in (self.out_n, self.out_n - 1, self.w - 1, self.w, self.w + 1, self.head_n - 1, BIG) if c >= 1})


class Prefix:
    """n good_fill groups in one stream: stream, out, and the bit / output offset of every block start"""

    def __init__(self, fills, seed=101):
        rng = np.random.default_rng(seed)
        c = M.Ctx(W.BitWriter(), bytearray())
        self.cuts = [(0, 0)]  # (stream bytes, output bytes) behind every group
        for _ in range(fills):
            M.good_fill(c, FILL, rng)
            assert c.bw.n % 8 == 0
            self.cuts.append((c.bw.n // 8, len(c.out)))
        self.stream, self.out = c.bw.bytes().tobytes(), bytes(c.out)
        out, blocks = W.inflate(np.frombuffer(self.stream + TERMINATOR, np.uint8))
        assert out == self.out
        self.starts = [b["start"] for b in blocks[:-1]]
        self.stored = [b["start"] for b in blocks[:-1] if b["type"] == 0]

    def first(self, k):
        """the first k groups -> (stream bytes, output bytes, block starts, those of stored blocks)"""
        s, o = self.cuts[k]
        return self.stream[:s], self.out[:o], [b for b in self.starts if b < 8 * s], [b for b in self.stored if b < 8 * s]

    def groups(self, a, b):
        return self.stream[self.cuts[a][0]: self.cuts[b][0]], self.out[self.cuts[a][1]: self.cuts[b][1]]


def prefix():
    """the 24 groups; M's 12 are its first 12"""
    return cached("sm-prefix", Prefix, L_FILLS)


def _placed(place, name, head):
    """class `name` behind the good blocks `head` = (stream, out, starts, stored starts)"""
    writer, hint = BY_NAME[name]
    stream, out, starts, stored = head
    seg, out_n, good = M.class_behind(writer, out)
    if name == "final_block_ends_short":
        hint = M.OK
    return Case(f"{name}/{place}", stream + seg.tobytes(), out_n, good, name, place, hint, len(out), 8 * len(stream),
                list(starts) if stream else [0], stored)


def _classes(place, fills, skip=frozenset()):
    head = prefix().first(fills)
    return [_placed(place, name, head) for name, _, _ in M.CLASSES if name not in skip]


def p0_cases():
    return cached("sm-P0", _classes, "P0", 0)


def m_cases():
    return cached("sm-M", _classes, "M", M_FILLS)


def l_cases():
    return cached("sm-L", _classes, "L", L_FILLS, NOT_LONG)


def _f_cases():
    stream, out, starts, stored = prefix().first(M_FILLS)
    cases = []
    for kind, payload in (("dynamic", LA.dynamic_payload(31)), ("stored", LA.stored_payload(32))):
        # (its last padding bit is set: this header is no candidate itself, whatever stands behind its payload)
        block = b"\x80" + len(payload).to_bytes(2, "little") + (len(payload) ^ 0xFFFF).to_bytes(2, "little") + payload
        head = (stream + block, out + payload, starts + [8 * len(stream)], stored + [8 * len(stream)])
        for name in REPS:
            c = _placed("F", name, head)
            c.name, c.look = f"{name}/F-{kind}", 8 * (len(stream) + 5)
            cases.append(c)
    return cases


def f_cases():
    return cached("sm-F", _f_cases)


def outer_starts(stream_n, piece=65535):
    """the block starts of stored_stream's output: one header every piece + 5 bytes"""
    return list(range(0, 8 * stream_n, 8 * (piece + 5)))


def stored_stream(payload, piece=65535):
    """a good stream of stored blocks only that carries payload"""
    bw = W.BitWriter()
    n = max(1, -(-len(payload) // piece))
    for k in range(n):
        W.write_stored(bw, payload[k * piece: (k + 1) * piece], final=k == n - 1)
    return bw.bytes().tobytes()


def _d_case():
    payload = b"".join(c.stream for c in l_cases())
    s = stored_stream(payload)
    starts = outer_starts(len(s))
    return Case("classes-as-data/D", s, len(payload), payload, "as_data", "D", M.OK, len(payload), 8 * len(s), starts, starts)


def d_case():
    return cached("sm-D", _d_case)


def _chain(tag, parts, cls, hint=None):
    """parts: good pieces (stream, out) and classes (name or writer, final[, tail]) in stream order -> the Case; out_n is the first
    class's promise and good the output in front of it; its chain_end is the bit at which the first class given by name
    starts (the count pass finds that fault, and the chain of records ends with the record that holds it)"""
    stream, out, first, chain_end = b"", b"", None, None
    for p in parts:
        if isinstance(p[0], bytes):
            stream, out = stream + p[0], out + p[1]
        else:
            writer = BY_NAME[p[0]][0] if isinstance(p[0], str) else p[0]
            seg, out_n, good = M.class_behind(writer, out, p[2] if len(p) > 2 else None, final=p[1])
            if first is None:
                first = (out_n, good, len(out), 8 * len(stream))
            if chain_end is None and isinstance(p[0], str):
                chain_end = 8 * len(stream)
            stream += seg.tobytes()
            out = good  # (what lies behind a fault is only there to be parsed)
    c = Case(f"{tag}/T", stream, first[0], first[1], cls, "T", hint, first[2], first[3])
    c.chain_end = chain_end
    return c


def _t_cases():
    P = prefix()
    a, b, tail = P.groups(0, 6), P.groups(6, M_FILLS), (TERMINATOR, b"")
    # (a class that stops the decoder keeps its status; behind the others the stream goes on, and the judge alone says how)
    stops = (M.ERROR, M.BAD_HEADER, M.LEN_MISMATCH, M.BAD_LITLEN, M.BAD_DIST)
    cases = [_chain(f"{name}-then-btype3", [a, (name, False), b, ("btype3", True)], name,
                    BY_NAME[name][1] if BY_NAME[name][1] in stops and name != "stored_payload_cut" else None) for name in REPS]
    cases += [_chain(f"btype3-then-{name}", [a, ("btype3", False), b, (name, True)], "btype3", M.BAD_HEADER)
              for name in ("cl_oversubscribed", "ll_symbol_286")]
    # a distance one too far behind the second group: the count pass cannot see it, the write pass can.  An empty stored
    # block behind it ends it on a byte, so that the good groups behind it are read as what they are
    far, c, d, e = (M.c_too_far_nonfinal, True, M.write_marker), P.groups(0, 2), P.groups(2, M_FILLS), P.groups(2, 10)
    for name in ("ll_symbol_286", "stored_nlen_mismatch"):
        cases.append(_chain(f"too-far-then-{name}", [c, far, d, (name, True)], "too_far", M.BAD_DIST))
        cases.append(_chain(f"{name}-then-too-far", [c, (name, False), e, far, P.groups(10, M_FILLS), tail], name, BY_NAME[name][1]))
    return cases


def t_cases():
    return cached("sm-T", _t_cases)


# ---- the truncation sweep ----

def _sweeps():
    s, out = M.sweep_stream()
    stream, head, starts, stored = prefix().first(M_FILLS)
    cases = []
    for k in range(1, len(s)):
        for kind in M.TRAILERS:
            buf = M.with_trailer(s, k, kind).tobytes()
            cases.append(Case(f"cut-{k}-{kind}/S0", buf, len(out), b"", "cut", "S0"))
            cases.append(Case(f"cut-{k}-{kind}/SM", stream + buf, len(head) + len(out), head, "cut", "SM", None, len(head),
                              8 * len(stream), starts, stored))
    return cases


def sweep_cases():
    return cached("sm-sweeps", _sweeps)


def wrap(raw, data, container, isize=None):
    """the raw stream in its container, made on the host; data: the bytes the trailer speaks of; isize: gzip's ISIZE field"""
    if container == "raw":
        return bytes(raw)
    if container == "zlib":
        return b"\x78\x9c" + bytes(raw) + zlib.adler32(data).to_bytes(4, "big")
    n = len(data) if isize is None else isize
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + bytes(raw) + zlib.crc32(data).to_bytes(4, "little") + \
        (n & 0xFFFFFFFF).to_bytes(4, "little")


def _wrapped_sweep(container):
    """a truncated download: the wrapped file cut at every byte (header, body and trailer cuts), and whole
    -> [(buffer, capacity, judge's status)]"""
    s, out = M.sweep_stream()
    f = wrap(s, out, container)
    return [(f[:k], len(out), H.serial(f[:k], container, len(out))[0]) for k in range(1, len(f) + 1)]


def wrapped_sweep(container):
    return cached("sm-wrapped-" + container, _wrapped_sweep, container)


# ---- the chunk partition a context must arrive at ----

def candidates(stream):
    """the bits k_stream_find takes for block starts: dynamic headers, and stored headers with a stored header behind their payload"""
    return sorted(set(H.scan(stream)) | set(SS.scan(stream, look=True)))


def partition(case, S):
    """stream_cases.predict for a Case of this module: chunk 0 at bit 0, then the first candidate of every nominal chunk of S
    bytes -> dict: picks (bits); false: the picks that are no block start (a stored header's candidate is the last bit at which
    its three header bits may stand in front of its LEN field, so it counts as its block's start when both have the same LEN
    byte); confirmed: the chain's records when the fault lies in the last one -- all of them, since a record that started off
    the chain is decoded again, or settled as empty, and counted"""
    cands = np.asarray(cached(("sm-cands", case.name), candidates, case.stream), np.uint64)
    bits, nc = 8 * len(case.stream), max(1, -(-len(case.stream) // S))
    picks = [0]
    for c in range(1, nc):
        lo, hi = 8 * c * S, min(8 * (c + 1) * S, bits)
        k = int(np.searchsorted(cands, lo))
        if k < len(cands) and int(cands[k]) < hi:
            picks.append(int(cands[k]))
    starts, len_bytes = set(case.starts), {(b + 10) // 8 for b in case.stored}
    true = [p for p in picks if p in starts or ((p + 10) // 8 in len_bytes and p in SS.scan(case.stream, p, p + 1))]
    return {"picks": picks, "false": [p for p in picks if p not in true], "confirmed": len(picks)}
