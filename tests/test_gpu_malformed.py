"""One status per malformation class on the GPU's indexed decode paths: every class and placement of tests/malformed_cases.py
and its truncation sweep must get the status that module's rule states (the serial decoder's, container.hpp compiled for the
host, on the segment's own bytes) from the index-only path (speculative wave + lane-serial kernel), from a context made with
SFH_INFLATE_SERIAL=1, from ONE decompress_batch call that holds them all, from decompress_ranges, from the sub-indexed
region lanes, from the wide rows (the device call and decompress_bgzf) and from decompress_any.  Every buffer has its true
size; where a segment stands in front of other bytes (its real neighbour, or a trailer of zeros, 0xFF, its own continuation
or noise behind a one-segment index), those bytes belong to the buffer and must not change the status.  An index holds
contiguous offsets, so bytes of no segment BETWEEN two segments cannot be given to these calls: that variant of placement
(e) is the CPU test's.  (The same cases on the core compiled for the host: tests/test_malformed_core_host.py.)"""
import numpy as np
import pytest
import torch

import bgzf_files as BZ
import bgzf_wide_cases as K
import malformed_cases as M
import stream_host as S
from starflate_amd import _capi

pytestmark = pytest.mark.gpu
BB = 32768
SERIAL_BIT = 2  # SegInfo.raw: decoded by the lane-serial kernel


@pytest.fixture(scope="module")
def serial():
    """a context made with SFH_INFLATE_SERIAL=1: the lane-serial kernel decodes every segment"""
    from starflate_amd import Compressor

    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SFH_INFLATE_SERIAL", "1")
        c = Compressor(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    return M.class_cases()


@pytest.fixture(scope="module")
def judged(cases):
    return {c.name: M.rule(S.serial, c.segment(), c.out_n, c.boundary) for c in cases}


@pytest.fixture(scope="module")
def sweep():
    s, out, cuts = M.sweep_cuts()
    return s, out, cuts, [M.rule(S.serial, s[:k], len(out))[0] for k in cuts]


def _callable(c):
    return len(c.stream) > 0  # (a stream of no bytes at all is no call: the host API wants a buffer)


def _device_call(ctx, c):
    """the device-buffer call on a destination filled with 0xA5 -> (destination bytes, a guard behind them, status)"""
    src = torch.from_numpy(np.ascontiguousarray(c.stream)).cuda()
    out = torch.full((c.total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    _, st = ctx.decompress_tensor(src, torch.from_numpy(np.array(c.idx, np.int64)).cuda(), c.total, out=out, block_bytes=BB)
    torch.cuda.synchronize()
    back = out.cpu().numpy()
    return back[: c.total].tobytes(), back[c.total:], int(st)


def _through(ctx, cases, judged, serial_rows):
    bad = []
    noise = np.random.default_rng(23).integers(0, 256, 64, dtype=np.uint8)
    for c in cases:
        if not _callable(c):
            continue
        want, s, w, dst = judged[c.name]
        got, st = ctx.decompress(c.stream, np.array(c.idx, np.uint64), c.total, block_bytes=BB)
        if st != want:
            bad.append((c.name, want, st))
            continue
        if want == 0:
            assert got[c.seg * M.SEG: c.seg * M.SEG + w] == dst[:w].tobytes(), c.name
        else:
            assert got == b"", c.name  # the host-buffer call hands out nothing of a failed stream
        info = ctx.debug(_capi.DBG_SEGINFO, len(c.idx) - 1)
        if serial_rows and want != 0:
            assert info[c.seg, 2] & SERIAL_BIT, c.name  # the failing row was finished by the lane-serial kernel
            assert info[c.seg, 0] == want, c.name
            for g in c.good:  # ... and its good neighbours were not
                assert info[g, 0] == 0 and not info[g, 2] & SERIAL_BIT, (c.name, g)
        if c.good:
            # the device-buffer call decodes straight into dst: whatever the middle segment's status, its good neighbours'
            # bytes are there and nothing behind the stream's size is written
            back, guard, dst_st = _device_call(ctx, c)
            assert dst_st == want, c.name
            for g, b in c.good.items():
                assert back[g * M.SEG: g * M.SEG + len(b)] == b, (c.name, g)
            assert np.all(guard == 0xA5), c.name
        if len(c.idx) == 2:  # the same segment in front of 64 bytes of noise that the one-segment index leaves out
            st2 = ctx.decompress(np.concatenate([c.stream, noise]), np.array(c.idx, np.uint64), c.total, block_bytes=BB)[1]
            if st2 != want:
                bad.append((c.name + "+noise", want, st2))
    assert not bad, bad


def test_index_only(compressor, cases, judged):
    _through(compressor, cases, judged, True)


def test_lane_serial_context(serial, cases, judged):
    _through(serial, cases, judged, False)


def test_sweep_index_only_and_serial(compressor, serial, sweep):
    """every cut in front of each of the five trailers: the buffer holds cut + trailer bytes, the index says [0, cut]"""
    s, out, cuts, want = sweep
    for ctx in (compressor, serial):
        for t in M.TRAILERS:
            got = [ctx.decompress(M.with_trailer(s, k, t), np.array([0, k], np.uint64), len(out), block_bytes=BB)[1] for k in cuts]
            assert got == want, (t, [(k, w, g) for k, w, g in zip(cuts, want, got) if w != g][:20])
        assert ctx.decompress(s, np.array([0, len(s)], np.uint64), len(out), block_bytes=BB) == (out, 0)


def test_one_batch_holds_them_all(compressor, cases, judged, sweep):
    """every case's segment, and every sweep cut in front of each trailer, as raw items of one call: one status per item, and
    the good items' bytes.  An item's index is [0, its segment's bytes]; the trailer lies behind that inside the item."""
    s, out, cuts, sweep_want = sweep
    noise = np.random.default_rng(29).integers(0, 256, 64, dtype=np.uint8)
    items, sizes, want, good, index = [], [], [], {}, []
    for c in cases:
        w_st, _, w, dst = judged[c.name]
        for tail in (np.zeros(0, np.uint8), noise):
            if w_st == 0:
                good[len(items)] = dst[:w].tobytes()
            items.append(np.concatenate([c.segment(), tail]).tobytes())
            index += [0, len(c.segment())]
            sizes.append(c.out_n)
            want.append(w_st)
    for t in M.TRAILERS:
        for k, w_st in zip(cuts, sweep_want):
            items.append(M.with_trailer(s, k, t).tobytes())
            index += [0, k]
            sizes.append(len(out))
            want.append(w_st)
    good[len(items)] = out
    items.append(s.tobytes())
    index += [0, len(s)]
    sizes.append(len(out))
    want.append(0)
    outs, st = compressor.decompress_batch(items, sizes, index=np.array(index, np.uint64), block_bytes=[BB] * len(items))
    assert st == want, [(i, w, g) for i, (w, g) in enumerate(zip(want, st)) if w != g][:20]
    for i, b in good.items():
        assert outs[i] == b, i
    # ... and without an index (every item one segment: the item's bytes are the segment's)
    plain = [i for i in range(len(items)) if index[2 * i + 1] == len(items[i])]
    outs, st = compressor.decompress_batch([items[i] for i in plain], [sizes[i] for i in plain])
    assert st == [want[i] for i in plain]
    assert all(outs[j] == good[i] for j, i in enumerate(plain) if i in good)


def test_ranges(compressor, cases, judged):
    """a range inside the malformed segment gets its status; ranges in the good neighbours get 0 and their bytes"""
    for c in cases:
        if c.place != "e" or len(c.good) != 2:
            continue
        want = judged[c.name][0]
        offs = [100, M.SEG + 10, 2 * M.SEG + 50]
        lens = [300, 100, 200]
        outs, st = compressor.decompress_ranges(c.stream, np.array(c.idx, np.uint64), c.total, offs, lens, block_bytes=BB)
        assert list(st) == [0, want, 0], (c.name, list(st), want)
        assert outs[0] == c.good[0][100:400] and outs[2] == c.good[2][50:250], c.name
        if want == 0:
            assert outs[1] == judged[c.name][3][10:110].tobytes(), c.name


def test_sub_indexed(compressor, cases, judged):
    """the region lanes: damage that keeps every bit offset, and every header class, get the rule's status"""
    seg, sub, out, patched = M.sub_fixed_segment()
    one = np.array([0, len(seg)], np.uint64)
    assert compressor.decompress(seg, one, M.SEG, subindex=sub[None], block_bytes=BB) == (out, 0)
    for name, (bad, hint) in patched.items():
        want = M.rule(S.serial, bad, M.SEG)[0]
        assert want == hint
        assert compressor.decompress(bad, one, M.SEG, subindex=sub[None], block_bytes=BB)[1] == want, name
        assert compressor.decompress(bad, one, M.SEG, block_bytes=BB)[1] == want, name
    wrong = sub.copy()
    wrong[7, 0] += 1
    assert compressor.decompress(seg, one, M.SEG, subindex=wrong[None], block_bytes=BB)[1] == M.ERROR
    zero = np.zeros((1, 32, 2), np.uint32)
    for c in cases:
        if c.cls in M.HEADER_CLASSES and c.place == "a" and c.hint != 0:
            st = compressor.decompress(c.stream, np.array(c.idx, np.uint64), c.total, subindex=zero, block_bytes=BB)[1]
            assert st == judged[c.name][0], c.name


def test_wide_rows(compressor):
    """each class behind byte 40000 of a 65280-byte BGZF member, through the wide device call and decompress_bgzf, judged on
    the member's body; a good member in front of it and one behind it keep their bytes"""
    txt = BZ.text(M.WIDE, seed=5)
    good = K.hand_member(K.zlib_body(txt), txt)
    for name, body, hint in M.wide_cases():
        want, s, w, dst = M.rule(S.serial, body, M.WIDE)
        assert want == hint, name
        payload = dst[:w].tobytes() if want == 0 else bytes(M.WIDE)
        member = K.hand_member(body.tobytes(), payload)
        if s == 0:
            # the body is a good stream: the member is a gzip stream, and the serial decoder's answer for it (container.hpp
            # with the wrapper: ISIZE and CRC-32 of what the body gave) is the row's -- a body that ends short is Error there
            want = S.serial(np.frombuffer(member, np.uint8), "gzip", M.WIDE)[0]
            assert want == (0 if w == M.WIDE else M.ERROR), name
        blob = good + member + good + BZ.EOF
        total = 3 * M.WIDE
        out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        _, n, st = compressor.decompress_bgzf_wide_tensor(torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda(), total, out=out)
        torch.cuda.synchronize()
        back = out.cpu().numpy()
        assert st == want, (name, st, want)
        assert back[: M.WIDE].tobytes() == txt and back[2 * M.WIDE: total].tobytes() == txt and np.all(back[total:] == 0xA5), name
        if want == 0:
            assert n == total and back[M.WIDE: 2 * M.WIDE].tobytes() == payload, name
        info = compressor.debug(_capi.DBG_SEGINFO, 3)
        assert [int(v) for v in info[:, 0]] == [0, want, 0], name
        host, hst = compressor.decompress_bgzf(blob)
        assert hst == want and host == (txt + payload + txt if want == 0 else b""), (name, hst, want)


def test_decompress_any(compressor):
    """no index: a flushed three-segment stream with the class in its middle segment, judged on the whole stream
    (malformed_cases.any_rule); a class that cuts the middle segment's flush marker off leaves a stream that is not
    block-flushed, which the call refuses as such"""
    from starflate_amd import StarflateError

    bad, kinds = [], set()
    for name, stream, total, hi, flushed in M.any_cases():
        try:
            got, st = compressor.decompress_any(stream, total)
        except StarflateError as e:
            if flushed or e.code != -8:
                bad.append((name, "rc %d" % e.code))
            kinds.add("refused")
            continue
        want, why = M.any_rule(S.serial, stream, total, hi)
        kinds.add(why)
        if not flushed or st != want or got != b"":
            bad.append((name, want, st, flushed))
    assert not bad, bad
    assert kinds == {"refused", "before_end", "final_inside"}
