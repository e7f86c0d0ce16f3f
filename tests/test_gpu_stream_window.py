"""Far distances and the carried window in the stream decoders (decompress_stream, decompress_stream_batch: one decoder, a
single stream being a call of one item; sf_stream.hip, sf_stream_core.h), on the streams of tests/stream_cases.py (their CPU side: tests/test_stream_window.py).

zlib never emits a distance above 32506, so its streams do not reach window entry 0, nor a marker that survives many chunks
and groups.  These do: generations of 32 KiB copied through matches at 32768, 32767 and 32768 - 257 (47 chunks in 7 groups
with 512-byte nominal chunks, 10 chunks in 3 groups on a default context), chunks whose outputs are 32767, 32768, 32769, a
few hundred, 3 x 32768 + 5 and 5 x 32768 bytes (both branches of window_step, a short chunk behind a long one and the
reverse), dist == out_pos against dist == out_pos + 1 in the first 32 KiB, and a second fault in front of or behind the bad
distance at capacities around every edge.

The reference is never the code under test: the status is the serial decoder's (container.hpp's decompress through
stream_host.serial) and the bytes are the writer's own.  A run only counts if it was the predicted one: the confirmed
chunks and the longest chunk equal the CPU prediction (stream_cases.predict) and no repair round was needed.  (A stream with
a structural fault ends its chain at the fault, so only its status and bytes are compared.)"""
import zlib

import numpy as np
import pytest

import stream_cases as SC
import stream_host as H
from starflate_amd import Compressor, synth

pytestmark = pytest.mark.gpu

OK, DST_TOO_SMALL = SC.OK, SC.DST_TOO_SMALL
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
CONTAINERS = ("raw", "zlib", "gzip")


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def _ctx(mp, **env):
    for k, v in env.items():
        mp.setenv(k, v)
    c = Compressor(0)
    for k in env:
        mp.delenv(k)
    return c


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(monkeypatch_module):
    c = _ctx(monkeypatch_module, SFH_STREAM_CHUNK="512")
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiny_batches(monkeypatch_module):
    c = _ctx(monkeypatch_module, SFH_BATCH_CHUNKS="4")
    yield c
    c.close()


def _check(c, stream, container, cap, data):
    """GPU status == serial status; Success only with the writer's bytes.  -> status"""
    want = H.serial(stream, container, cap)[0]
    out, st = c.decompress_stream(stream, cap, container)
    assert st == want, (st, want, container, cap)
    if st == OK:
        assert len(out) == len(data), (len(out), len(data))
        if out != data:
            a, b = np.frombuffer(out, np.uint8), np.frombuffer(data, np.uint8)
            assert False, ("first differing byte", int(np.nonzero(a != b)[0][0]), "of", len(data))
    return st


def _predicted(c, case, S):
    """the last single call ran the predicted chunks"""
    s, p = c.last_stream_stats(), SC.predict(case, S)
    assert (s["confirmed"], s["repair_rounds"]) == (p["confirmed"], 0), (case.name, S, s, p["confirmed"])
    if case.status == OK:
        assert s["longest_chunk"] == p["longest_chunk"], (case.name, S, s, p["longest_chunk"])


def _both(comp, small):
    return ((comp, 16384), (small, 512))


def _whole(comp, small, case):
    """a clean stream in every container on both contexts: exact capacity, size query, one byte short"""
    for container in CONTAINERS:
        s = case.wrapped(container)
        for c, S in _both(comp, small):
            assert _check(c, s, container, case.n, case.data) == OK
            _predicted(c, case, S)
            assert c.decompress_stream(s, None, container) == (case.data, OK)
            _predicted(c, case, S)
            assert _check(c, s, container, case.n - 1, case.data) == DST_TOO_SMALL


@pytest.mark.parametrize("which", ["gens40", "rich"])
def test_generations(comp, small, which):
    _whole(comp, small, getattr(SC, which)())


def test_chunk_sizes(comp, small):
    _whole(comp, small, SC.sizes())


@pytest.mark.parametrize("name,case", SC.window_cases(), ids=[n for n, _ in SC.window_cases()])
def test_first_window(comp, small, name, case):
    for c, S in _both(comp, small):
        for cap in SC.capacities(case):
            st = _check(c, case.raw, "raw", cap, case.data)
            assert st == case.expected(cap), (name, S, cap, st)
            _predicted(c, case, S)  # (a bad distance and a short dst are the write pass's to find: the same chunks)
    if case.status == OK:
        _whole(comp, small, case)


@pytest.mark.parametrize("name,case", SC.fault_cases(), ids=[n for n, _ in SC.fault_cases()])
def test_fault_order(comp, small, name, case):
    for c, S in _both(comp, small):
        for cap in SC.capacities(case):
            st = _check(c, case.raw, "raw", cap, case.data)
            assert st == case.expected(cap), (name, S, cap, st)
        for container in ("zlib", "gzip"):  # (behind a cut the trailer is read as body bits: the serial decoder names the status)
            assert _check(c, case.wrapped(container), container, 1 << 16, case.data) != OK


def test_wrapped(comp, small):
    """gzip ISIZE below, equal to and above the body's size, a wrong Adler-32 behind a clean body, a bad distance in a gzip
    body whose ISIZE ends before, on and behind it"""
    cases = dict(SC.window_cases())
    for c, _ in _both(comp, small):
        for case in (SC.clean_window(), cases["middle-mid-ok"], SC.sizes()):
            n = case.n
            for isize, cap in ((n - 1, n), (n - 1, n - 1), (n, n), (n + 1, n), (n + 1, n + 1)):
                _check(c, case.wrapped("gzip", isize=isize), "gzip", cap, case.data)
            assert _check(c, case.wrapped("zlib", adler=zlib.adler32(case.data) ^ 1), "zlib", n, case.data) == SC.ERROR
            assert _check(c, case.wrapped("gzip", isize=n + 1), "gzip", n + 1, case.data) == SC.ERROR
        bad = cases["middle-mid-bad"]
        for isize in (bad.fault_out - 1, bad.fault_out, bad.fault_out + 1, SC.clean_window().n + SC.MATCH_LEN):
            st = _check(c, bad.wrapped("gzip", isize=isize), "gzip", 1 << 20, bad.data)
            assert st == (DST_TOO_SMALL if isize < bad.fault_out else SC.INVALID_DISTANCE)


# ---- batches ----

def _zlib(data, container, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[container])
    return c.compress(data) + c.flush()


def _batch(container, gens_first):
    """-> [(stream, capacity, Case or None, bytes)]: the window streams between ordinary zlib-made items and failing ones"""
    w, f = dict(SC.window_cases()), dict(SC.fault_cases())
    full = SC.clean_window().n + SC.MATCH_LEN
    plain = [synth.gen_mixed(n, seed=k, stripe=40000).tobytes() for k, n in enumerate((70000, 1000, 200000))]
    plain = [(_zlib(d, container, 6 if k else 1), len(d), None, d) for k, d in enumerate(plain)]
    good = [SC.gens40(), SC.sizes(), SC.rich(), w["first-mid-ok"], w["at-32768-ok"], w["last-token0-ok"]]
    bad = [w["middle-mid-bad"], f["bad-dist-type3-behind"], f["bad-dist-lenmis-front"], w["at-32767-bad"], f["cut-last-block"]]
    good = [(c.wrapped(container), c.n, c, c.data) for c in good]
    bad = [(c.wrapped(container), full, c, c.data) for c in bad]
    # a one-group item next to items of many groups; a window case (its first chunk sees an empty window) right behind
    # the items that leave a full one
    items = [good[0], plain[0], bad[0], good[3], good[1], plain[1], bad[1], good[2], good[4], bad[2], plain[2], bad[3],
             good[5], bad[4]]
    return items if gens_first else items[::-1]


def _check_batch(c, S, items, container, short):
    """one call; every item against the single call on it alone, the serial decoder and the writer's bytes.  short: every
    other item gets a capacity one byte short"""
    streams = [it[0] for it in items]
    caps = [cap - 1 if short and k % 2 == 0 else cap for k, (_, cap, _, _) in enumerate(items)]
    outs, sts = c.decompress_stream_batch(streams, caps, container)
    batch = c.last_stream_stats()
    singles = []
    for k, (s, _, case, data) in enumerate(items):
        want = H.serial(s, container, caps[k])[0]
        out1, st1 = c.decompress_stream(s, caps[k], container)
        one = c.last_stream_stats()
        singles.append(one)
        assert sts[k] == st1 == want, (k, sts[k], st1, want)
        assert outs[k] == out1, k
        if st1 == OK:
            assert out1 == data, k
            assert caps[k] == len(data)
            if case is not None:
                _predicted(c, case, S)
        elif case is None or case.status == OK:
            assert st1 == DST_TOO_SMALL and caps[k] == len(data) - 1, (k, st1)
    for key in ("chunks", "candidates", "confirmed"):
        assert batch[key] == sum(s[key] for s in singles), (key, batch, singles)
    assert batch["longest_chunk"] == max(s["longest_chunk"] for s in singles)
    assert batch["repair_rounds"] == max(s["repair_rounds"] for s in singles)
    return sts


@pytest.mark.parametrize("gens_first", [True, False], ids=["generations-first", "generations-last"])
@pytest.mark.parametrize("container", CONTAINERS)
def test_batches(comp, small, tiny_batches, container, gens_first):
    items = _batch(container, gens_first)
    for c, S in ((comp, 16384), (small, 512), (tiny_batches, 16384)):
        sts = _check_batch(c, S, items, container, False)
        assert [st == OK for st in sts] == [case is None or case.status == OK for _, _, case, _ in items], sts
        sts = _check_batch(c, S, items, container, True)
        assert sum(st == DST_TOO_SMALL for st in sts) >= 4, sts
