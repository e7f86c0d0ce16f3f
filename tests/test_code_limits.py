"""Length-limited Huffman codes at the caps of RFC 1951 (15 bits for literal/length and distance codes, 7 bits for the
code-length code), on the CPU: the test writer's streams (tests/deflate_writer.py) against zlib and the host build of the
lane decoder (sf_inflate_core.h, per segment and with the sub-index), and inputs that drive the encoder specification
(the oracle) past the caps, with the coverage asserted: each input's unconstrained Huffman tree is deeper than the cap,
and 15-bit length / distance codes with their 5 / 13 extra bits and 7-bit code-length codes are written.

The input builders and the writer-made streams are module-level functions: tests/test_gpu_code_limits.py runs the same
ones through the GPU kernels."""
import functools
import zlib

import numpy as np
import pytest

import deflate_writer as W
import oracle_lib as O
from test_inflate_core_host import core, decode_segment  # noqa: F401  (core: the host build of the lane decoder)

CHUNK = 32768
FIB = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597]
STRIPS = (32768, 65536, 131072)
STRATEGIES = (("dynamic", 3), ("auto", 0))


# ---- inputs that drive the compressor past the caps ----

def lit_deep_chunk(seed):
    """32768 bytes drawn from 200 values, a Fibonacci tail of 12 rare values (2, 3, 5, .. 377) and one copy of 150 bytes
    (length symbol 281, extra value 19: the top one of its 5 extra bits set).  The end-of-block code and that match are the
    tail's two 1s: the unconstrained literal/length tree is 17 deep."""
    rng = np.random.default_rng(seed)
    tail = np.repeat(np.arange(200, 212, dtype=np.uint8), FIB[2:14])
    a = np.concatenate([rng.integers(0, 200, CHUNK - tail.size - 150, dtype=np.uint8), tail])
    rng.shuffle(a)
    return np.concatenate([a[:20000], a[1000:1150], a[20000:]])


def dist_deep_chunk(seed):
    """32768 random bytes with 4..5-byte copies planted at Fibonacci counts over 17 distance codes, the rarest one a copy
    from 30000 bytes back (code 29, extra value 5423: the top one of its 13 extra bits set).  Each copy's source is the
    most recent place of its first four bytes, the bytes around it differ from those around every older one, and no copy
    crosses a 512-byte parse region: an exact-chain search finds each of them as planted, so the unconstrained distance tree
    is 16 deep."""
    rng = np.random.default_rng(seed)
    codes = [6, 7, 5, 8, 4, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19]
    plan = np.array([c for c, f in zip(codes, FIB[1:]) for _ in range(f)])
    rng.shuffle(plan)
    a, occ = bytearray(), {}

    def push(b):
        a.append(b)
        if len(a) >= 4:
            occ.setdefault(bytes(a[-4:]), []).append(len(a) - 4)

    def rnd():
        push(int(rng.integers(0, 256)))

    def plant(c, length, dist=None):
        while True:
            rnd()
            p = len(a)
            if p // 512 != (p + length) // 512:
                continue
            for _ in range(20):
                lo = max(W.DIST_BASE[c], length)
                d = dist or int(rng.integers(lo, W.DIST_BASE[c] + (1 << W.DIST_EXTRA[c])))
                q = p - d
                if q < 1:
                    continue
                xs = occ.get(bytes(a[q:q + 4]), [])
                if not xs or xs[-1] != q or any(a[x - 1] == a[p - 1] for x in xs if x != q and x >= 1):
                    continue
                for k in range(length):
                    push(a[q + k])
                bad = {a[x + length] for x in xs if x + length < len(a)}
                push(next(v for v in rng.permutation(256).tolist() if v not in bad))
                return

    for _ in range(64):
        rnd()
    for c in plan:
        plant(int(c), int(rng.integers(4, 6)))
    assert len(a) < 30000
    while len(a) < 30800:
        rnd()
    plant(29, 5, 30000)
    while len(a) < CHUNK:
        rnd()
    return np.frombuffer(bytes(a[:CHUNK]), np.uint8).copy()


def skewed_lit_lengths(seed):
    """Literal code lengths (5..15, Kraft sum 1, the end-of-block code one of the longest) whose code-length items
    (oracle-style run-length coding, HDIST = 1) have an unconstrained Huffman tree deeper than 7: found by a seeded search."""
    for s in range(seed, seed + 100000):
        rng = np.random.default_rng(s)
        nsym = int(rng.integers(150, 258))
        leaves = [5] * 32
        while len(leaves) < nsym:
            i = int(rng.integers(0, len(leaves)))
            if leaves[i] < 15:
                l = leaves.pop(i)
                leaves += [l + 1, l + 1]
        leaves.sort()
        ll = np.zeros(286, np.int64)
        ll[256] = leaves.pop()
        ll[rng.permutation(256)[: len(leaves)]] = rng.permutation(leaves)
        if cl_depth(ll, np.zeros(30, np.int64)) > 7:
            return ll
    raise AssertionError("no lengths found")


def cl_items(ll_lens, d_lens):
    hlit = max([257] + [s + 1 for s in range(286) if ll_lens[s]])
    hdist = max([1] + [s + 1 for s in range(30) if d_lens[s]])
    return W.rle(list(ll_lens[:hlit])) + W.rle(list(d_lens[:hdist]))


def cl_depth(ll_lens, d_lens):
    f = np.zeros(19, np.int64)
    for s, _ in cl_items(ll_lens, d_lens):
        f[s] += 1
    return int(W.huffman_depths(f).max())


def cl_deep_chunk(seed, lens):
    """2^15 - 1 bytes whose counts are 2^(15 - length) for the literal lengths `lens` (the end-of-block code the 1), in an
    order in which no four bytes repeat: no match, so the Huffman lengths are exactly `lens`."""
    rng = np.random.default_rng(seed)
    a = np.repeat(np.arange(256), [(1 << (15 - int(l))) if l else 0 for l in lens[:256]]).astype(np.uint8)
    assert a.size == CHUNK - 1
    rng.shuffle(a)
    seen = set()
    for i in range(3, a.size):
        for _ in range(1000):
            g = a[i - 3:i + 1].tobytes()
            if g not in seen:
                break
            j = int(rng.integers(i, a.size))
            a[i], a[j] = a[j], a[i]
        else:
            raise AssertionError("no 4-gram free order")
        seen.add(g)
    return a


@functools.lru_cache(maxsize=1)
def deep_input():
    """One input, its chunks: [0] unconstrained distance tree 16 deep, [1] literal/length tree 17 deep, [2] text, [3] (the
    last, 2^15 - 1 bytes) literal lengths whose code-length code is deeper than 7.  -> (bytes, {what: chunk})"""
    from starflate_amd import synth

    lens = skewed_lit_lengths(2705)
    data = np.concatenate([dist_deep_chunk(2), lit_deep_chunk(0), synth.gen_text(CHUNK, seed=3), cl_deep_chunk(1, lens)])
    return data, {"d": 0, "ll": 1, "cl": 3}


def oracle_params(strategy, strip, **kw):
    # the exact-chain effort of depth 8 (the library's effort "best"); no stored fast path
    return O.default_params(strategy=strategy, strip_bytes=strip, fast_skip=0, chain_depth=8, **kw)


def chunk_histograms(data, p):
    out = []
    for flat, nt, tarr in O.chunk_tokens(data, p):
        out.append(O.histogram(tarr, nt, p.region_bytes))
    return out


def unconstrained(ll, d):
    """unconstrained depths of the literal/length and distance trees of one chunk's histograms (end-of-block counted)"""
    return int(W.huffman_depths(ll).max()), int(W.huffman_depths(d).max())


def stream_blocks(stream, index, chunks):
    """the blocks of the segments `chunks`, read by the test decoder -> {segment: block list}"""
    return {c: W.inflate(stream, 8 * int(index[c]), stop_at_segment_end=True)[1] for c in chunks}


def check_code(lens, maxbits, freq=None):
    """the lengths of one code: at most maxbits, the maximum reached, Kraft sum exactly 1 with two or more codes, and
    (freq given) a rarer symbol never has the shorter code"""
    lens = np.asarray(lens, np.int64)
    used = np.flatnonzero(lens)
    assert lens.max() == maxbits, lens.max()
    if used.size >= 2:
        assert W.kraft(lens, maxbits) == 1 << maxbits
    if freq is not None:
        f = np.asarray(freq, np.int64)
        assert np.array_equal(np.flatnonzero(f), used)
        order = np.lexsort((used, f[used]))  # by frequency
        assert np.all(np.diff(lens[used][order]) <= 0), "a rarer symbol got a shorter code"


def assert_edges_written(blocks, deep):
    """the 15-bit length code with 5 extra bits (the top one set), the 15-bit distance code with 13 (the top one set)
    and a 7-bit code-length code were all written"""
    lb = [b for seg in blocks.values() for b in seg if b["type"] == 2]
    assert any(cl == 15 and ne == 5 and ev >= 16 for b in lb for cl, ne, ev in b["len_items"])
    assert any(cl == 15 and ne == 13 and ev >= 4096 for b in lb for cl, ne, ev in b["dist_items"])
    hdr = blocks[deep["cl"]][0]["header"]
    assert max(hdr["cl_lens"]) == 7 and max(W.huffman_depths(hdr["cl_freq"])) > 7


# ---- writer-made streams with every edge of the decoders ----

def random_tokens(rng, ll, dl, out_n, hist=0, sub=True, late=()):
    """tokens of out_n bytes using the symbols that have codes in ll / dl (each of them at least once where it fits:
    the symbols are drawn at probabilities between 2^-length and a floor); matches reach at most `hist` bytes before the
    segment and (sub) never cross a 1024-byte region"""
    ll, dl = np.asarray(ll), np.asarray(dl)
    lsyms = [s for s in range(286) if ll[s] and s != 256]
    dsyms = [s for s in range(30) if dl[s]]
    pw = np.array([max(2.0 ** -ll[s], 0.004) for s in lsyms])
    pw /= pw.sum()
    dw = np.array([max(2.0 ** -dl[s], 0.01) for s in dsyms]) if dsyms else None
    if dw is not None:
        dw /= dw.sum()
    toks, pos = [], 0
    while pos < out_n:
        s = lsyms[int(rng.choice(len(lsyms), p=pw))]
        if s < 256:
            toks.append(s)
            pos += 1
            continue
        k = s - 257
        length = W.LEN_BASE[k] + int(rng.integers(0, 31 if s == 284 else 1 << W.LEN_EXTRA[k]))  # 284 + 31 would be 258
        ds = dsyms[int(rng.choice(len(dsyms), p=dw))] if dsyms else None
        if ds is None:
            continue
        dmax = min(W.DIST_BASE[ds] + (1 << W.DIST_EXTRA[ds]) - 1, pos + hist)
        if dmax < W.DIST_BASE[ds] or pos + length > out_n or (sub and pos // W.REGION != (pos + length - 1) // W.REGION):
            lit = [x for x in lsyms if x < 256]
            if lit:
                toks.append(lit[int(rng.integers(0, len(lit)))])
                pos += 1
            continue
        toks.append(W.match(length, int(rng.integers(W.DIST_BASE[ds], dmax + 1))))
        pos += length
    return np.array(toks, np.uint32)


def _all_lengths_code(n_syms, first):
    """lengths 1, 2, .. 14, 15, 15 over the symbols first[0..16)"""
    lens = np.zeros(n_syms, np.int64)
    for k, s in enumerate(first):
        lens[s] = min(k + 1, 15)
    return lens


def edge_segments(seed=11):
    """-> {name: (segments for write_stream, one block per segment?, what the reports must show)}"""
    rng = np.random.default_rng(seed)
    cases = {}
    # literal/length codes of every length 1..15, the end-of-block code one of the two 15-bit ones; one distance code of
    # length 1; 16/17/18 at their longest repeats
    ll = _all_lengths_code(286, [65, 257, 66, 258, 267, 67, 270, 68, 269, 69, 72, 70, 284, 71, 256, 282])
    dl = np.zeros(30, np.int64)
    dl[4] = 1
    segs = [[(random_tokens(rng, ll, dl, n), ll, dl, {"cl_lens": "skewed"})] for n in (CHUNK, CHUNK, 5000)]
    cases["ll_1_to_15"] = (segs, {"ll": set(range(1, 16)), "d": {1}, "eob": 15, "cl": {7}})
    # distance codes of every length 1..15, code 29 (extra 13 bits) one of the 15-bit ones; literal/length code from
    # package-merge
    dl = _all_lengths_code(30, [10, 3, 11, 0, 12, 13, 1, 14, 15, 16, 17, 2, 18, 19, 29, 28])
    f = np.zeros(286, np.int64)
    f[:256] = rng.integers(1, 2000, 256)
    f[256:286] = rng.integers(100, 4000, 30)
    f[256] = 1
    ll = W.package_merge(f, 15)
    segs = [[(random_tokens(rng, ll, dl, CHUNK), ll, dl, {})] for _ in range(3)]
    cases["d_1_to_15"] = (segs, {"d": set(range(1, 16)), "ll": {9, 10}})
    # HDIST = 1 with no distance code and no matches, HLIT = 286 sent in full, HCLEN untrimmed, 16/17/18 never used
    ll = np.zeros(286, np.int64)
    ll[:257] = 8
    ll[254] = ll[255] = 9  # 255 codes of 8 bits, two of 9
    dl = np.zeros(30, np.int64)
    toks = rng.integers(0, 256, CHUNK).astype(np.uint32)
    segs = [[(toks, ll, dl, {"hlit": 286, "hdist": 1, "trim_hclen": False, "avoid_repeats": True})]]
    cases["no_distances"] = (segs, {"d": set(), "hdist": 1, "hlit": 286})
    # repeats across the HLIT/HDIST boundary (zeros and a non-zero length), HDIST = 30, shortest repeats
    f = np.zeros(286, np.int64)
    f[:200] = rng.integers(1, 300, 200)
    f[256], f[257:266] = 1, rng.integers(50, 200, 9)
    fd = np.zeros(30, np.int64)
    fd[5:30] = rng.integers(1, 100, 25)
    ll, dl = W.package_merge(f, 15), W.package_merge(fd, 15)
    segs = [[(random_tokens(rng, ll, dl, CHUNK), ll, dl, {"cross": True, "hlit": 286, "hdist": 30, "max_repeats": False})]]
    cases["cross_boundary"] = (segs, {"hlit": 286, "hdist": 30})
    # several dynamic blocks with different trees in one segment (three, and six: more than the speculative kernel follows)
    multi = []
    for nb in (3, 6):
        blocks = []
        for k in range(nb):
            f = np.zeros(286, np.int64)
            f[:256] = (rng.pareto(1.0, 256) * 10).astype(np.int64) * (rng.random(256) < 0.7)
            f[256], f[257:285] = 1, (rng.pareto(1.0, 28) * 5).astype(np.int64)
            fd = (rng.pareto(1.0, 30) * 5).astype(np.int64)
            fd[0] = max(fd[0], 1)
            ll, dl = W.package_merge(f, 15), W.package_merge(fd, 15)
            blocks.append((random_tokens(rng, ll, dl, CHUNK // nb + (CHUNK % nb if k == nb - 1 else 0), sub=False), ll, dl, {"cl_lens": "skewed" if k % 2 else None}))
        multi.append(blocks)
    cases["multi_block"] = (multi, {})
    return cases


def edge_streams():
    """-> {name: (stream, index, subindex or None, output bytes, reports)}: every segment independent (strips of 32 KiB
    and more decode them alike)"""
    out = {}
    for name, (segs, _) in edge_segments().items():
        one = all(len(b) == 1 for b in segs)
        out[name] = W.write_stream(segs, subindex=one)
    return out


def random_pages(n=300, seed=5):
    """n single-segment pages (at most 32 KiB each) with random legal codes: package-merge over heavy-tailed frequencies,
    random token streams.  -> list of (stream, bytes, report)"""
    rng = np.random.default_rng(seed)
    pages = []
    for _ in range(n):
        f = np.zeros(286, np.int64)
        nl = int(rng.integers(1, 257))
        f[rng.permutation(256)[:nl]] = (rng.pareto(rng.uniform(0.3, 2.0), nl) * 50).astype(np.int64) + 1
        f[256] = 1
        nm = int(rng.integers(0, 30))
        f[257 + rng.permutation(29)[:nm]] = (rng.pareto(1.0, nm) * 20).astype(np.int64) + 1
        fd = np.zeros(30, np.int64)
        if nm:
            k = int(rng.integers(1, 31))
            fd[rng.permutation(30)[:k]] = (rng.pareto(0.8, k) * 20).astype(np.int64) + 1
            if rng.random() < 0.3:  # geometric counts: the limit binds, the code reaches 15 bits when k > 15
                fd[rng.permutation(30)[:k]] = 1 << np.arange(k)
        ll, dl = W.package_merge(f, 15), W.package_merge(fd, 15)
        size = int(rng.choice([1, 100, 4096, int(rng.integers(1, CHUNK + 1)), CHUNK]))
        toks = random_tokens(rng, ll, dl, size, sub=False)
        opt = {"cl_lens": "skewed"} if rng.random() < 0.3 else {}
        s, idx, _, data, reps = W.write_stream([[(toks, ll, dl, opt)]])
        pages.append((s, data, reps[0]))
    return pages


# ---- the tests ----

def test_package_merge_and_writer_helpers():
    rng = np.random.default_rng(3)
    for _ in range(200):
        f = np.minimum(rng.pareto(rng.uniform(0.2, 2.0), int(rng.integers(2, 287))) * 100, 1e6).astype(np.int64)
        f[rng.integers(0, f.size, 2)] += 1
        for maxbits in (7, 9, 15):
            if np.count_nonzero(f) > 1 << maxbits:
                continue
            lens = W.package_merge(f, maxbits)
            assert lens.max() <= maxbits and np.array_equal(lens > 0, f > 0)
            if np.count_nonzero(f) >= 2:
                assert W.kraft(lens, maxbits) == 1 << maxbits
            h = W.huffman_depths(f)
            if h.max() <= maxbits:  # no limit binding: as short as Huffman's
                assert (lens * f).sum() == (h * f).sum()
            else:  # never worse than the oracle's clamp-and-repair
                assert (lens * f).sum() <= (O.build_lengths(f, maxbits).astype(np.int64) * f).sum()
    assert W.huffman_depths(np.array(FIB[:14])).max() == 13
    for items in (W.rle([0] * 300 + [5] * 20), W.rle([0] * 139 + [7] * 7, max_repeats=False), W.rle([3] * 9, avoid=True)):
        assert len(items)


def test_writer_streams_decode_with_zlib_and_host_core(core):
    """Every writer-made stream decodes with zlib to the intended bytes, and with the host lane decoder per segment and
    (one block per segment) region by region with the sub-index; the reports show every edge each one was built for."""
    import ctypes as C

    for name, (segs, want) in edge_segments().items():
        stream, idx, sub, data, reps = W.write_stream(segs, subindex=all(len(b) == 1 for b in segs))
        assert zlib.decompress(stream.tobytes(), -15) == data, name
        back, blocks = W.inflate(stream)
        assert back == data
        for key, v in want.items():
            if key in ("ll", "d"):
                assert v <= set().union(*[set(r[key]) for r in reps]) if v else not any(r[key] for r in reps), (name, key)
            elif key == "cl":
                assert v <= set().union(*[set(r["cl"]) for r in reps]), name
            else:
                assert all(r[key] == v for r in reps), (name, key)
        arr = np.frombuffer(data, np.uint8)
        for c in range(idx.size - 1):
            out_n = min(CHUNK, arr.size - c * CHUNK)
            st, got = decode_segment(core, stream, int(idx[c]), int(idx[c + 1]), out_n)
            assert st == 0 and np.array_equal(got, arr[c * CHUNK: c * CHUNK + out_n]), (name, c, st)
            if sub is None:
                continue
            buf = np.zeros(stream.size + 3, np.uint8)
            buf[: stream.size] = stream
            tok = np.zeros(CHUNK + 4, np.uint32)
            ntok, raw, raw_off = C.c_uint32(), C.c_uint32(), C.c_uint64()
            sc = np.ascontiguousarray(sub[c])
            st = core.sfi_decode_segment_sub(buf.ctypes.data, stream.size, int(idx[c]), int(idx[c + 1]), out_n, sc.ctypes.data,
                                             tok.ctypes.data, C.byref(ntok), C.byref(raw), C.byref(raw_off))
            assert st == 0 and not raw.value, (name, c, st)
            assert np.array_equal(tok[: ntok.value], segs[c][0][0]), (name, c)  # the writer's own tokens
    # the edges, over all the cases together
    allrep = [r for _, (s, i, x, d, reps) in edge_streams().items() for r in reps]
    assert set(range(1, 16)) <= set().union(*[set(r["ll"]) for r in allrep])
    assert set(range(1, 16)) <= set().union(*[set(r["d"]) for r in allrep])
    assert any(r["eob"] == 15 for r in allrep) and any(7 in r["cl"] for r in allrep)
    assert any(cl == 15 and ne == 5 for r in allrep for cl, ne, ev in r["len_items"])
    assert any(cl == 15 and ne == 13 for r in allrep for cl, ne, ev in r["dist_items"])


def test_random_pages_decode_with_zlib_and_host_core(core):
    lens_seen, d15 = set(), False
    for s, data, rep in random_pages(120):
        assert zlib.decompress(s.tobytes(), -15) == data
        st, got = decode_segment(core, s, 0, s.size, len(data))
        assert st == 0 and got.tobytes() == data
        lens_seen |= set(rep["ll"]) | set(rep["d"])
        d15 = d15 or 15 in rep["d"]
    assert 15 in lens_seen and d15


@pytest.mark.parametrize("strategy_name,strategy", STRATEGIES)
def test_inputs_drive_the_specification_past_the_caps(strategy_name, strategy):
    """The deep input's intended chunks have unconstrained trees deeper than the caps at every strip size, and the
    specification's lengths are clamped to exactly 15 / 7, legal, and ordered by frequency."""
    data, deep = deep_input()
    for strip in STRIPS:
        p = oracle_params(strategy, strip)
        hists = chunk_histograms(data, p)
        assert unconstrained(*hists[deep["ll"]])[0] > 15, strip
        assert unconstrained(*hists[deep["d"]])[1] > 15, strip
        for c, (ll, d) in enumerate(hists):
            pl = O.plan_chunk(ll, d, min(CHUNK, data.size - c * CHUNK), c + 1 == len(hists), p)
            assert pl.btype == 2 or c == 2, (strip, c, pl.btype)
            if pl.btype != 2:
                continue
            lens = np.frombuffer(pl.ll_lens, np.uint8)[:286]
            dlen = np.frombuffer(pl.d_lens, np.uint8)[:30]
            if c in (deep["ll"], deep["d"]):
                check_code(lens if c == deep["ll"] else dlen, 15, ll if c == deep["ll"] else d)
            if c == deep["ll"]:
                assert lens[281] == 15 and ll[281] == 1
            if c == deep["d"]:
                assert dlen[29] == 15 and d[29] == 1
            if c == deep["cl"]:
                assert cl_depth(lens, dlen) > 7
        stream = O.compress(data, p)
        assert zlib.decompress(stream.tobytes(), -15) == data.tobytes()
        s2, index, _ = O.compress_indexed(data, p)
        assert np.array_equal(s2, stream)
        blocks = stream_blocks(stream, index, deep.values())
        assert_edges_written(blocks, deep)
        hdr = blocks[deep["cl"]][0]["header"]
        check_code(hdr["cl_lens"], 7, hdr["cl_freq"])
