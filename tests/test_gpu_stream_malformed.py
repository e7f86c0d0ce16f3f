"""One status per malformation class on the stream decoders (sfh_inflate_stream*, sfh_inflate_stream_batch*: sf_stream.hip,
sf_stream_core.h, sf_stream_chain.h and stream_batch_run in sf_capi.hip), on the streams of tests/stream_malformed_cases.py
(their CPU side: tests/test_stream_malformed_cases.py).

stream_decode has a symbol loop of its own with exits of its own; every chunk but an item's first starts on a speculative
candidate, and a chunk started on a false one usually ends in one of these very exits, whose status must never surface; the
real fault must surface through the host's chain rounds, the follow lanes and the write pass, in the serial decoder's order
against DstTooSmall and InvalidDistance, which only the write pass can see; the item's destination must stay untouched and
the other items of a batch unharmed.

The judge is never the code under test: every expected status is stream_host.serial(stream, container, cap), container.hpp
compiled for the host, on the whole stream at the capacity the call is given; expected bytes are the writer's own in front of
the class and the judge's behind it.  Three contexts: a default one (16384-byte nominal chunks), `small` (512-byte ones: the
fault lies dozens of records in, and small items carry many speculative starts) and `tiny_batches` (launch batches of 128 KiB
of output)."""
import zlib

import numpy as np
import pytest
import torch

import malformed_cases as M
import stream_malformed_cases as G
from starflate_amd import Compressor, synth

pytestmark = pytest.mark.gpu

OK, BIG = M.OK, G.BIG
GUARD = 64


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


def _single(ctx, case, cap):
    """one raw stream at one capacity: the judge's status; on Success the judge's bytes, whose part in front of the class is
    the writer's; on failure nothing -> status"""
    want_st, w, want = case.judge(cap)
    out, st = ctx.decompress_stream(case.stream, cap, "raw")
    assert st == want_st, (case.name, cap, st, want_st)
    if st == OK:
        assert len(out) == w and out == want, (case.name, cap)
        n = min(w, len(case.good))
        assert out[:n] == case.good[:n], (case.name, cap)
    else:
        assert out == b"", (case.name, cap)
    return st


@pytest.mark.parametrize("place", ["P0", "M", "L"])
def test_classes_single(comp, small, place):
    """every class alone, behind 12 and behind 24 groups of good blocks, at capacities around the promise, the judge's count
    and the good blocks' output"""
    cases = {"P0": G.p0_cases, "M": G.m_cases, "L": G.l_cases}[place]()
    assert len(cases) == len(M.CLASSES) - (len(G.NOT_LONG) if place == "L" else 0)
    seen = set()
    for ctx, S in ((comp, 16384), (small, 512)):
        for case in cases:
            for cap in case.capacities():
                seen.add(_single(ctx, case, cap))
                if S == 512 and place != "P0" and cap == BIG:  # the run was the predicted one: the fault in the last record
                    s = ctx.last_stream_stats()
                    assert s["confirmed"] == G.partition(case, S)["confirmed"], (case.name, s)
    assert seen == set(range(8)), seen


def test_false_candidate_in_front(comp, small):
    """the record that decodes the class started on a look-alike inside the stored block in front of it"""
    for case in G.f_cases():
        for cap in (case.out_n, BIG):
            _single(small, case, cap)
            s = small.last_stream_stats()
            assert s["repair_rounds"] >= 1 and s["confirmed"] == G.partition(case, 512)["confirmed"], (case.name, s)
            _single(comp, case, cap)


def test_classes_as_data(comp, small):
    """every class inside the payload of a good stored stream: hundreds of false candidates whose decodes fail, and none of
    those statuses surfaces"""
    d = G.d_case()
    false = len(G.partition(d, 512)["false"])
    for ctx in (comp, small):
        assert _single(ctx, d, d.out_n) == OK
        s = ctx.last_stream_stats()
        # a run of false candidates is mended by one follow lane per round (tests/test_gpu_stream.py::
        # test_stored_deflate_one_round: at most two rounds)
        assert s["repair_rounds"] <= 2, s
        if ctx is small:
            assert s["candidates"] >= false >= 500, (s, false)


def test_two_faults(comp, small):
    """the earlier fault wins, whichever pass finds it, and the chain of records ends with the record that holds the first
    structural fault: no record behind it is counted or written"""
    for ctx in (comp, small):
        for case in G.t_cases():
            for cap in (case.out_n, BIG):
                assert _single(ctx, case, cap) != OK
                if ctx is small and case.hint is not None:
                    s = ctx.last_stream_stats()
                    want = sum(b <= case.chain_end for b in G.partition(case, 512)["picks"])
                    assert s["confirmed"] == want, (case.name, cap, s, want)
                    assert want < s["candidates"] or case.cls == "too_far", (case.name, s)  # (a structural fault at the very end)


@pytest.mark.parametrize("which", ["default", "small"])
def test_containers(comp, small, which):
    """every L stream as zlib and as gzip, the trailer made on the host from the judge's bytes.  container.hpp takes a zlib dst
    to be exactly the output size, the library checks the Adler-32 over the bytes produced (starflate_hip.h), so a zlib stream
    whose body decodes is asked at the capacity w, where both agree.  With a size query first (out_n None) the answer is the
    judge's at a capacity that is no obstacle, 1 << 20 (zlib: w)."""
    ctx = comp if which == "default" else small
    seen = set()
    for case in G.l_cases():
        st_big, w, data = case.judge(BIG)
        z = G.wrap(case.stream, data, "zlib")
        for cap in {w} | ({case.out_n} if case.judge(case.out_n)[0] != OK else set()):
            want = case.judge(cap, "zlib", z)[0]
            out, st = ctx.decompress_stream(z, cap, "zlib")
            assert st == want and out == (data if st == OK else b""), (case.name, "zlib", cap, st, want)
        want = case.judge(w if st_big == OK else BIG, "zlib", z)[0]
        assert want == st_big
        assert ctx.decompress_stream(z, None, "zlib") == ((data if want == OK else b""), want), (case.name, "zlib query", want)
        for isize in (w, case.out_n):
            g = G.wrap(case.stream, data, "gzip", isize)
            for cap in (BIG, case.out_n):
                want = case.judge(cap, "gzip", g)[0]
                out, st = ctx.decompress_stream(g, cap, "gzip")
                assert st == want and out == (data if st == OK else b""), (case.name, "gzip", isize, cap, st, want)
                seen.add(st)
            want = case.judge(BIG, "gzip", g)[0]
            got = ctx.decompress_stream(g, None, "gzip")
            assert got == ((data if want == OK else b""), want), (case.name, "gzip query", isize, got[1], want)
    assert seen == set(range(8)), seen


def test_query_isize_above_body(comp, small):
    """A gzip file whose body is good and whose ISIZE claims more than the body gives (`final_block_ends_short` behind 24 groups
    with ISIZE = out_n = 55203, the body giving w = 55202 bytes), decoded with a size query first through each of the four
    entry points: the judge's answer at a capacity that is no obstacle, which is Error -- the body decodes and its size is not
    ISIZE.  (A decode behind the query with exactly the 55202 queried bytes would be DstTooSmall, a gzip dst below ISIZE being
    refused before the body is read: the entry points give the decode room for ISIZE.)  A good neighbour in the same batch
    decodes."""
    case = {c.cls: c for c in G.l_cases()}["final_block_ends_short"]
    st_big, w, data = case.judge(BIG)
    assert st_big == OK and w == case.out_n - 1
    g = G.wrap(case.stream, data, "gzip", case.out_n)
    good = G.wrap(case.stream, data, "gzip", w)
    want = case.judge(BIG, "gzip", g)[0]
    assert want == M.ERROR and case.judge(w, "gzip", g)[0] == M.DST_SMALL and case.judge(BIG, "gzip", good)[0] == OK
    tg, tgood = (torch.from_numpy(np.frombuffer(x, np.uint8).copy()).cuda() for x in (g, good))
    for ctx in (comp, small):
        assert ctx.decompress_stream(g, None, "gzip") == (b"", want)
        out, st = ctx.decompress_stream_tensor(tg, None, "gzip")
        assert (out.numel(), st) == (0, want)
        assert ctx.decompress_stream_batch([g, good], None, "gzip") == ([b"", data], [want, OK])
        outs, sts = ctx.decompress_stream_batch_tensors([tg, tgood], None, "gzip")
        assert sts == [want, OK] and outs[0].numel() == 0 and outs[1].cpu().numpy().tobytes() == data


# ---- one batch holds them all ----

def _good_items():
    """zlib-made raw items -> [(stream, capacity, status, bytes)]"""
    out = []
    for k, n in enumerate((0, 1, 32767, 32769, 150001)):
        data = synth.gen_mixed(n, seed=k, stripe=40000).tobytes() if n else b""
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        out.append((z.compress(data) + z.flush(), n, OK, data))
    return out


def _raw_items():
    """every P0, M, L, F and T case and every sweep item at its promised capacity, a good item behind every fourth"""
    cases = G.p0_cases() + G.m_cases() + G.l_cases() + G.f_cases() + G.t_cases() + G.sweep_cases()
    good, items = _good_items(), []
    for k, c in enumerate(cases):
        st, w, data = c.judge(c.out_n)
        items.append((c.stream, c.out_n, st, data))
        if k % 4 == 3:
            items.append(good[(k // 4) % len(good)])
    return items


@pytest.fixture(scope="module")
def raw_items():
    return _raw_items()


def _run_device_batch(ctx, items, container):
    """one decompress_stream_batch_tensors call; the destinations carved from one allocation of 0xA5 with guard bands"""
    soff, o = [], 0
    for s, _, _, _ in items:
        soff.append(o)
        o = (o + len(s) + 15) // 16 * 16
    packed = np.zeros(max(o, 16), np.uint8)
    for a, (s, _, _, _) in zip(soff, items):
        packed[a: a + len(s)] = np.frombuffer(s, np.uint8)
    src = torch.from_numpy(packed).cuda()
    srcs = [src[a: a + len(s)] for a, (s, _, _, _) in zip(soff, items)]
    doff, o = [], GUARD
    for _, cap, _, _ in items:
        doff.append(o)
        o = (o + cap + GUARD + 15) // 16 * 16
    buf = torch.full((o + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = [buf[a: a + cap] for a, (_, cap, _, _) in zip(doff, items)]
    got, sts = ctx.decompress_stream_batch_tensors(srcs, [cap for _, cap, _, _ in items], container, outs=outs)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    untouched = np.ones(host.size, bool)
    want_sts = [st for _, _, st, _ in items]
    assert sts == want_sts, [(k, a, b) for k, (a, b) in enumerate(zip(sts, want_sts)) if a != b][:20]
    for k, (a, (_, cap, st, data)) in enumerate(zip(doff, items)):
        if st == OK:
            assert got[k].numel() == len(data) and host[a: a + len(data)].tobytes() == data, k
            untouched[a: a + len(data)] = False
    # a failed item's destination, the rest of a good one's and every guard band
    assert (host[untouched] == 0xA5).all(), np.nonzero(untouched & (host != 0xA5))[0][:10]
    return sts


@pytest.mark.parametrize("which", ["default", "small"])
def test_one_batch_holds_them_all(comp, small, raw_items, which):
    """thousands of failing items and good ones between them in one call: the per-item judge's statuses, good items byte for
    byte, and an item's destination written only on its status 0 (starflate_hip.h)"""
    sts = _run_device_batch(comp if which == "default" else small, raw_items, "raw")
    assert set(sts) == set(range(8))
    assert len(raw_items) >= 3500 and sum(st != OK for st in sts) >= 1800


@pytest.mark.parametrize("third", [0, 1, 2])
def test_launch_batches_hold_them_all(tiny_batches, raw_items, third):
    """the same items where a launch batch holds 128 KiB of output, so that failing and good items share launch batches
    hundreds of times over.  A launch batch decodes a handful of records lane-serially, which takes its time however few
    they are, so the list goes in three calls of consecutive thirds: each case stays within a few seconds."""
    n = len(raw_items)
    part = raw_items[third * n // 3: (third + 1) * n // 3]
    sts = _run_device_batch(tiny_batches, part, "raw")
    assert len(set(sts)) >= 7 and min(sum(st != OK for st in sts), sum(st == OK for st in sts)) >= 100


@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_truncated_downloads(comp, small, container):
    """the sweep stream in its container, the file cut at every byte: header, body and trailer cuts in one call"""
    items = [(f, cap, st, M.sweep_stream()[1] if st == OK else b"") for f, cap, st in G.wrapped_sweep(container)]
    for ctx in (comp, small):
        sts = _run_device_batch(ctx, items, container)
        assert sts[-1] == OK and all(st != OK for st in sts[:-1])


def test_host_buffer_batch(comp, raw_items):
    """the same item lists through the host-buffer entry point"""
    for container, items in (("raw", raw_items),
                             ("zlib", [(f, cap, st, M.sweep_stream()[1] if st == OK else b"") for f, cap, st in G.wrapped_sweep("zlib")]),
                             ("gzip", [(f, cap, st, M.sweep_stream()[1] if st == OK else b"") for f, cap, st in G.wrapped_sweep("gzip")])):
        outs, sts = comp.decompress_stream_batch([s for s, _, _, _ in items], [cap for _, cap, _, _ in items], container)
        want = [st for _, _, st, _ in items]
        assert sts == want, [(k, a, b) for k, (a, b) in enumerate(zip(sts, want)) if a != b][:20]
        assert outs == [data if st == OK else b"" for _, _, st, data in items]
