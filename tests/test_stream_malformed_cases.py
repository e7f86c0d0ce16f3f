"""The streams of tests/stream_malformed_cases.py are what they claim to be, on the CPU (the GPU side:
tests/test_gpu_stream_malformed.py), so that the GPU module cannot silently test less than it says: every class is there in
every placement, the judge (container.hpp's decompress, stream_host.serial) gives each the status its class was built for,
and each fault lies where the placement says -- inside a record that started on a speculative candidate, behind a false
candidate, or inside a payload."""
import ast
import inspect
import zlib
from collections import Counter

import pytest

import malformed_cases as M
import stream_malformed_cases as G

NAMES = [n for n, _, _ in M.CLASSES]
STATUSES = set(range(8))


def _prefix_part(c):
    """the good output in front of the class is the writer's, and the judge's bytes start with it"""
    st, w, got = c.judge(G.BIG)
    n = min(w, len(c.good))
    assert got[:n] == c.good[:n], c.name
    assert w >= c.head_n, c.name


@pytest.mark.parametrize("place,cases,missing", [("P0", G.p0_cases, set()), ("M", G.m_cases, set()), ("L", G.l_cases, G.NOT_LONG)],
                         ids=["P0", "M", "L"])
def test_every_class_gets_its_status(place, cases, missing):
    """no class is missing but for the named set, and the judge at the promised capacity says what the class was built for"""
    cases = cases()
    assert [c.cls for c in cases] == [n for n in NAMES if n not in missing]
    assert len(cases) == len(NAMES) - len(missing) and missing <= set(NAMES)
    seen = Counter()
    for c in cases:
        st, w, _ = c.judge(c.out_n)
        want = dict((n, h) for n, _, h in M.CLASSES)[c.cls]
        if c.cls == "final_block_ends_short":  # a good stream that is shorter: no index promised more
            assert (st, c.hint) == (M.OK, M.OK) and w == c.w < c.out_n, c.name
        else:
            assert st == want == c.hint, (c.name, st, want)
        seen[st] += 1
        _prefix_part(c)
        if c.w > c.head_n and c.head_n:  # the good blocks in front do not fit: DstTooSmall before the fault
            assert c.judge(c.head_n - 1)[0] == M.DST_SMALL, c.name
    if place != "P0":
        assert set(seen) == STATUSES, seen
    assert len(cases[0].stream) == len(G.prefix().first({"P0": 0, "M": G.M_FILLS, "L": G.L_FILLS}[place])[0]) + 1  # (btype3: one byte)


def test_generator_cannot_drop_a_case():
    tree = ast.parse(inspect.getsource(G))
    assert not [n for n in ast.walk(tree) if isinstance(n, (ast.Try, ast.Continue, ast.Break))]
    assert len(G.f_cases()) == 2 * len(G.REPS) and len(G.t_cases()) == len(G.REPS) + 2 + 4
    assert {G.BY_NAME[n][1] for n in G.REPS} == STATUSES
    s, _ = M.sweep_stream()
    assert len(G.sweep_cases()) == 2 * len(M.TRAILERS) * (len(s) - 1)
    assert len(G.wrapped_sweep("zlib")) == len(s) + 6 and len(G.wrapped_sweep("gzip")) == len(s) + 18


def test_good_parts_decode_with_zlib():
    P = G.prefix()
    assert (len(P.stream), len(P.out)) == P.cuts[G.L_FILLS] and len(P.out) == G.L_FILLS * G.FILL
    for k in (G.M_FILLS, G.L_FILLS):
        stream, out, starts, stored = P.first(k)
        assert zlib.decompressobj(-15).decompress(stream + G.TERMINATOR) == out and len(out) == k * G.FILL
        assert len(starts) == 3 * k and len(stored) == k
    assert len(P.first(G.M_FILLS)[1]) < 32768 < len(P.out)
    for c in G.f_cases():
        assert zlib.decompressobj(-15).decompress(c.stream[: c.at // 8] + G.TERMINATOR) == c.good[: c.head_n], c.name
    d = G.d_case()
    assert zlib.decompressobj(-15).decompress(d.stream) == d.good and d.judge(d.out_n) == (M.OK, d.out_n, d.good)
    assert d.good == b"".join(c.stream for c in G.l_cases()) and len(d.good) > 1400000


@pytest.mark.parametrize("cases,records", [(G.m_cases, {512: 12, 16384: 2}), (G.l_cases, {512: 20, 16384: 3})], ids=["M", "L"])
def test_fault_lies_in_the_last_record(cases, records):
    """the class's block is no chunk start itself and lies behind the last one, which is a true block start: the fault is found
    by a lane that started on a speculative candidate in front of it and came through good blocks"""
    for c in cases():
        for S, least in records.items():
            p = G.partition(c, S)
            assert p["false"] == [], (c.name, S, p["false"])
            assert c.at not in p["picks"] and max(p["picks"]) < c.at, (c.name, S)
            assert len(p["picks"]) >= least, (c.name, S, len(p["picks"]))
            assert c.at not in G.candidates(c.stream), c.name


def test_false_candidate_in_front():
    """F: the look-alike is the last pick at S = 512 and no block start; every other pick is one; the class behind it is none"""
    for c in G.f_cases():
        p = G.partition(c, 512)
        assert p["picks"][-1] == c.look and p["false"] == [c.look], (c.name, p["picks"][-3:], p["false"])
        assert c.look not in c.starts and c.look < c.at
        kind = c.name.rsplit("-", 1)[1]
        assert (c.look in G.H.scan(c.stream)) == (kind == "dynamic") and (c.look in G.SS.scan(c.stream, look=True)) == (kind == "stored")
        st, w, _ = c.judge(c.out_n)
        assert st == c.hint and c.hint == G.BY_NAME[c.cls][1], c.name
        _prefix_part(c)
    assert {c.hint for c in G.f_cases()} == STATUSES


def test_classes_as_data_are_false_candidates():
    d = G.d_case()
    p = G.partition(d, 512)
    assert len(p["false"]) >= 500, len(p["false"])
    assert all(b in d.starts for b in p["picks"] if b not in p["false"])


def test_two_faults():
    """the first fault in stream order is the judge's answer at every capacity that holds the bytes in front of it"""
    cases = {c.name: c for c in G.t_cases()}
    for c in cases.values():
        st, w, _ = c.judge(G.BIG)
        assert st != M.OK, c.name
        if c.hint is not None:
            assert st == c.hint and c.judge(c.out_n)[0] == c.hint, (c.name, st)
        _prefix_part(c)
        assert c.judge(c.head_n - 1)[0] == (M.DST_SMALL if w >= c.head_n else st), c.name
    # behind an accepted block and behind a literal too many the stream goes on: the status is the next fault's
    assert cases["hlit_287_accepted-then-btype3/T"].judge(G.BIG)[0] not in (M.OK, M.DST_SMALL)
    assert cases["one_literal_too_many-then-btype3/T"].judge(cases["one_literal_too_many-then-btype3/T"].out_n)[0] == M.DST_SMALL
    for name in ("ll_symbol_286", "stored_nlen_mismatch"):
        assert cases[f"too-far-then-{name}/T"].judge(G.BIG)[0] == M.BAD_DIST
        assert cases[f"{name}-then-too-far/T"].judge(G.BIG)[0] == G.BY_NAME[name][1] != M.BAD_DIST
    # both faults of a pair lie in records of their own at S = 512; where the first class stops the decoder, the chain ends
    # with the record that holds its block
    for c in cases.values():
        p = G.partition(c, 512)
        assert sum(b > c.at for b in p["picks"]) >= 4, c.name
        if c.hint is not None:
            n = sum(b <= c.chain_end for b in p["picks"])
            assert c.at <= c.chain_end and (n == len(p["picks"]) if c.cls == "too_far" else 1 <= n < len(p["picks"]) - 3), c.name
            assert c.chain_end == c.at or c.cls == "too_far", c.name


def test_sweeps():
    s, out = M.sweep_stream()
    seen = Counter(c.judge(c.out_n)[0] for c in G.sweep_cases())
    assert set(seen) == STATUSES, seen
    for c in G.sweep_cases():
        k = int(c.name.split("-")[1])
        if "continuation" in c.name:
            assert c.judge(c.out_n) == (M.OK, c.out_n, c.good + out), c.name
        elif "nothing" in c.name:
            assert c.judge(c.out_n)[0] != M.OK and len(c.stream) == c.at // 8 + k, c.name
    for container in ("zlib", "gzip"):
        w = G.wrapped_sweep(container)
        assert [st == M.OK for _, _, st in w] == [False] * (len(w) - 1) + [True]
        assert len({st for _, _, st in w}) >= 3
