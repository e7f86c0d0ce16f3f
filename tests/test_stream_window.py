"""The streams of tests/stream_cases.py are what they claim to be, on the CPU (the GPU side: tests/test_gpu_stream_window.py).

Every Success stream decodes with zlib and with the serial decoder (container.hpp's decompress) to the writer's own bytes, and
every failing stream gets the status its case names from the serial decoder, at every capacity the GPU module uses.  The
writer's reader (W.inflate) finds the far distances the streams were built for, and the chunk partition the GPU module expects
(stream_host.scan's candidates, the first one per nominal chunk, blk["start"] / blk["out"]) has no false start in it and holds
the chunk sizes, chunk-leading distance-32768 matches and group counts that the window kernels' edges need.

No stream here gives a confirmed chunk without output: the strict predicate took every block start these builders wrote (each
carries a complete distance code), so no link breaks and the chain rule's "settled empty" chunk does not arise; the block of
type 3 and the cut streams end the chain instead of emptying a chunk."""
import zlib

import numpy as np
import pytest

import deflate_writer as W
import stream_cases as SC
import stream_host as H

CHUNKS = (512, 16384)  # the GPU module's two nominal chunk sizes


def _walk(case):
    m = []
    out, blocks = W.inflate(np.frombuffer(case.raw, np.uint8), matches=m)
    assert out == case.data
    return m, blocks


def _decodes(case):
    assert zlib.decompressobj(-15).decompress(case.raw) == case.data
    for container in ("raw", "zlib", "gzip"):
        s = case.wrapped(container)
        st, n, out = H.serial(s, container, case.n)
        assert st == SC.OK and out.tobytes() == case.data and n in (None, case.n), (case.name, container, st)
        assert zlib.decompressobj({"raw": -15, "zlib": 15, "gzip": 31}[container]).decompress(s) == case.data


def _partition(case, blocks):
    """the writer's block starts are the reader's, and no nominal chunk of either size picks a false start"""
    assert [(b["start"], b["out"]) for b in blocks] == case.blocks
    pred = {}
    for S in CHUNKS:
        p = pred[S] = SC.predict(case, S)
        assert p["false"] == [], (case.name, S, p["false"])
        assert sum(p["outs"]) == case.n and len(p["outs"]) == p["confirmed"]
    return pred


@pytest.mark.parametrize("which", ["gens40", "rich"])
def test_generations(which):
    case = getattr(SC, which)()
    _decodes(case)
    m, blocks = _walk(case)
    pred = _partition(case, blocks)
    dist = np.array([d for _, d, _ in m])
    assert (dist > 32506).all()  # zlib's farthest
    first = {pos: d for pos, d, _ in m}
    lead = sum(first.get(o) == 32768 for o in pred[512]["bases"])
    print(which, len(case.raw), case.n, "matches", len(m), "at 32768:", int((dist == 32768).sum()), "32507..32767:",
          int((dist < 32768).sum()), "chunks", {S: pred[S]["confirmed"] for S in CHUNKS}, "led by 32768:", lead)
    if which == "gens40":
        assert (dist == 32768).sum() >= 1000 and ((dist >= 32507) & (dist <= 32767)).sum() >= 1000
        assert lead >= 30
        # more than one group carried in k_stream_link's loop: ceil(n / ceil(sqrt(n))) groups of the n chunks
        assert pred[512]["confirmed"] >= 36
    else:
        assert pred[16384]["confirmed"] >= 7  # at least 3 groups on a default context
        fresh = case.n - sum(ln for _, _, ln in m)
        assert fresh >= case.n // 3
    assert {b["type"] for b in blocks} == {0, 1, 2}


def test_chunk_sizes():
    case = SC.sizes()
    _decodes(case)
    m, blocks = _walk(case)
    pred = _partition(case, blocks)
    outs = pred[512]["outs"]
    print("chunk outputs at S = 512:", outs)
    for n in SC.SIZE_CLASSES:
        assert n in outs, (n, outs)
    short = [k for k, n in enumerate(outs) if n < 1000]
    assert any(outs[k - 1] > 32768 for k in short) and any(outs[k + 1] > 32768 for k in short if k + 1 < len(outs))
    first = {pos: (d, ln) for pos, d, ln in m}
    assert all(first.get(o) == (32768, 258) for o in pred[512]["bases"][1:])
    assert {1, 32767, 32768, 32768 - 257} == {d for _, d, _ in m}


@pytest.mark.parametrize("name,case", SC.window_cases(), ids=[n for n, _ in SC.window_cases()])
def test_first_window(name, case):
    pos = SC.places()[name.rsplit("-", 1)[0]]
    st, n, out = H.serial(case.raw, "raw", 1 << 20)
    assert (st, n) == (case.status, case.fault_out) and out[:n].tobytes() == case.data[:n]
    assert case.status == (SC.INVALID_DISTANCE if name.endswith("bad") else SC.OK)
    clean = SC.predict(SC.clean_window(), 512)
    assert clean["false"] == [] and clean["confirmed"] == 29  # every block but the final one is a chunk
    if case.status == SC.OK:
        _decodes(case)
        m, blocks = _walk(case)
        assert m == [(pos, pos, SC.MATCH_LEN)]
        pred = _partition(case, blocks)
        assert pred[512]["confirmed"] == 29 and pred[16384]["confirmed"] == 2
    else:
        assert case.fault_out == pos and case.events == [(pos, SC.INVALID_DISTANCE)]
        assert SC.predict(case, 512)["false"] == []
    chunk = max(k for k, o in enumerate(clean["bases"]) if o <= pos)
    # (seed FW_SEED: block 26 is the last that ends, match included, before 32768; 32767 and 32768 lie in block 27)
    want = {"first": (0,), "middle": (12,), "last": (26,), "at": (27, 28)}[name.split("-")[0]]
    assert chunk in want, (name, chunk)
    assert ("token0" in name) == (pos in clean["bases"])


@pytest.mark.parametrize("name,case", SC.fault_cases(), ids=[n for n, _ in SC.fault_cases()])
def test_fault_order(name, case):
    """which failure is first: the serial decoder's status at every capacity is the first event's in stream order, or
    DstTooSmall when the bytes in front of it do not fit"""
    st, n, out = H.serial(case.raw, "raw", 1 << 20)
    assert (st, n) == (case.status, case.fault_out) and out[:n].tobytes() == case.data
    kind = name.split("-")[-2] if "dist" in name else name.split("-")[0]
    second = {"type3": SC.INVALID_BLOCK_HEADER, "lenmis": SC.LEN_MISMATCH, "cut": SC.CUT_STATUS}[kind]
    if name.startswith("bad-dist") and name.endswith("behind"):
        assert case.status == SC.INVALID_DISTANCE
    else:
        assert case.status == second
    bases = SC.predict(SC.clean_window(), 512)["bases"]
    chunk = [max(k for k, o in enumerate(bases) if o <= p) for p, _ in case.events]
    assert chunk == sorted(chunk) and len(set(chunk)) == len(chunk)  # each fault in a chunk of its own, in stream order
    caps = SC.capacities(case)
    assert {case.fault_out - 1, case.fault_out, case.fault_out + 1, 1 << 20} <= set(caps)
    for cap in caps:
        assert H.serial(case.raw, "raw", cap)[0] == case.expected(cap), (name, cap)


def test_named_statuses():
    """the figures the cases were designed around: a bad distance in block 12 wins over whatever follows it, loses to
    whatever precedes it, and a capacity that ends in front of the first fault is DstTooSmall"""
    cases = dict(SC.fault_cases())
    p = SC.places()["middle-mid"]
    for kind in ("type3", "lenmis", "cut"):
        assert cases[f"bad-dist-{kind}-behind"].expected(1 << 20) == SC.INVALID_DISTANCE
        assert cases[f"bad-dist-{kind}-behind"].expected(p) == SC.INVALID_DISTANCE
        assert cases[f"bad-dist-{kind}-behind"].expected(p - 1) == SC.DST_TOO_SMALL
    assert cases["bad-dist-type3-front"].expected(1 << 20) == SC.INVALID_BLOCK_HEADER
    assert cases["bad-dist-lenmis-front"].expected(1 << 20) == SC.LEN_MISMATCH
    last = cases["type3-last-block"]
    assert last.expected(last.fault_out) == SC.INVALID_BLOCK_HEADER and last.expected(last.fault_out - 1) == SC.DST_TOO_SMALL


def test_wrapped():
    """gzip ISIZE below, equal to and above the body's size and a wrong Adler-32 behind a clean body: the statuses the GPU
    module's wrapped cases go by are the serial decoder's"""
    for case in (SC.clean_window(), dict(SC.window_cases())["middle-mid-ok"]):
        n = case.n
        for isize, cap, want in ((n - 1, n, SC.DST_TOO_SMALL), (n - 1, n - 1, SC.DST_TOO_SMALL), (n, n, SC.OK),
                                 (n + 1, n, SC.DST_TOO_SMALL), (n + 1, n + 1, SC.ERROR)):
            assert H.serial(case.wrapped("gzip", isize=isize), "gzip", cap)[0] == want, (isize, cap)
        assert H.serial(case.wrapped("zlib", adler=zlib.adler32(case.data) ^ 1), "zlib", n)[0] == SC.ERROR
        assert H.serial(case.wrapped("zlib"), "zlib", n - 1)[0] == SC.DST_TOO_SMALL
    bad = dict(SC.window_cases())["middle-mid-bad"]
    for isize in (bad.fault_out - 1, bad.fault_out, bad.fault_out + 1, SC.clean_window().n + SC.MATCH_LEN):
        want = SC.DST_TOO_SMALL if isize < bad.fault_out else SC.INVALID_DISTANCE
        assert H.serial(bad.wrapped("gzip", isize=isize), "gzip", 1 << 20)[0] == want, isize
