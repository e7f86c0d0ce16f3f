"""Random access (sfh_decompress_range*): byte ranges of an indexed stream's output decoded on the GPU for roughly what they
hold.  Every range equals the slice of the input, through the device call, the host call, the single-range call and the
Python methods; nothing outside the destinations is written; the token scratch says that only the decode spans were decoded;
damage stays inside the decode spans that hold it; the lane-serial mode agrees; the whole-stream decoders are untouched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
from conftest import GOLDEN
from range_cases import edge_ranges, random_ranges
from starflate_amd import Compressor, realbytes, synth

pytestmark = pytest.mark.gpu

SEG = 32768
PATTERN = 0xA5


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


def _content(kind, n, seed):
    if kind == "text":
        return synth.gen_text(n, seed=seed)
    if kind == "real":
        buf = realbytes.source(limit=n + 4096)
        assert buf.size >= n
        return buf[:n].copy()
    if kind == "noise":
        return synth.gen_random(n, seed=seed)
    # a mixture: text, noise (stored segments in the middle of strips), runs, text again, cut at odd places
    parts, at, k = [], 0, 0
    while at < n:
        m = min(n - at, (50001, 70003, 40009, 131072 + 17)[k % 4])
        parts.append(synth.gen_text(m, seed=seed + k) if k % 4 in (0, 3) else synth.gen_random(m, seed=seed + k) if k % 4 == 1
                     else np.repeat(np.random.default_rng(seed + k).integers(0, 256, m // 61 + 1, dtype=np.uint8), 61)[:m])
        at += m
        k += 1
    return np.concatenate(parts)


def _ranges(total_n, bb, seed, n_random=120):
    rng = np.random.default_rng(seed)
    r = edge_ranges(total_n, bb) + random_ranges(rng, total_n, n_random)
    order = rng.permutation(len(r))
    return [r[i] for i in order]


def _layout(ranges, seed, pad=64):
    """destinations packed back to back in one buffer (so: at odd addresses), now and then a gap of a few bytes; -> (positions, size)"""
    rng = np.random.default_rng(seed)
    pos, at = [], pad + 1
    for _, ln in ranges:
        pos.append(at)
        at += ln + (int(rng.integers(1, 8)) if rng.integers(0, 5) == 0 else 0)
    return pos, at + pad


def _expected(data, ranges, pos, size, ok=None):
    want = np.full(size, PATTERN, np.uint8)
    for i, ((off, ln), p) in enumerate(zip(ranges, pos)):
        if ok is None or ok[i]:
            want[p: p + ln] = data[off: off + ln]
    return want


class Dev:
    """a stream with its index (and sub-index) on the device"""

    def __init__(self, stream, idx, sub, total_n, bb):
        self.stream = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
        self.idx = torch.from_numpy(np.asarray(idx).astype(np.int64)).cuda()
        self.sub = None if sub is None else torch.from_numpy(np.ascontiguousarray(sub).view(np.int32).ravel().copy()).cuda()
        self.total_n, self.bb = total_n, bb


def _device_call(comp, d, ranges, pos, size, use_sub=True):
    """sfh_decompress_ranges_device_async into one pre-filled buffer -> (buffer, statuses) on the host"""
    k = len(ranges)
    buf = torch.full((size,), PATTERN, dtype=torch.uint8, device="cuda")
    st = torch.full((max(k, 1),), -1, dtype=torch.int32, device="cuda")
    sub = d.sub if use_sub else None
    rc = comp._lib.sfh_decompress_ranges_device_async(
        comp._h, d.stream.data_ptr(), d.stream.numel(), d.idx.data_ptr(), sub.data_ptr() if sub is not None else None,
        d.idx.numel() - 1, d.total_n, d.bb, k, (C.c_uint64 * k)(*[r[0] for r in ranges]), (C.c_uint64 * k)(*[r[1] for r in ranges]),
        (C.c_void_p * k)(*[buf.data_ptr() + p for p in pos]), C.c_void_p(st.data_ptr()), None)
    assert rc == 0, comp.last_error()
    torch.cuda.synchronize()
    return buf.cpu().numpy(), st[:k].cpu().numpy()


def _check_all_paths(comp, data, stream, idx, sub, bb, seed, n_random=120):
    total_n = data.size
    ranges = _ranges(total_n, bb, seed, n_random)
    pos, size = _layout(ranges, seed)
    want = _expected(data, ranges, pos, size)
    d = Dev(stream, idx, sub, total_n, bb)
    for use_sub in ((False, True) if sub is not None else (False,)):
        got, st = _device_call(comp, d, ranges, pos, size, use_sub)
        assert (st == 0).all(), (use_sub, [(r, int(s)) for r, s in zip(ranges, st) if s])
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (use_sub, bb, int(bad[0]), [r for r, p in zip(ranges, pos) if p <= bad[0] < p + r[1]][:1])
        assert comp._lib.sfh_index_entries(comp._h) == 0
    # the host variant and the Python methods on a part of the ranges, the single-range calls on a few
    part = ranges[:: 3]
    s = sub
    outs, st = comp.decompress_ranges(stream, idx, total_n, [r[0] for r in part], [r[1] for r in part], s, block_bytes=bb)
    assert (st == 0).all() and len(outs) == len(part)
    for (off, ln), o in zip(part, outs):
        assert o == data[off: off + ln].tobytes(), (off, ln)
    outs, st = comp.decompress_ranges(stream, idx, total_n, [r[0] for r in part], [r[1] for r in part], None, block_bytes=bb)
    assert (st == 0).all() and [o for o in outs] == [data[off: off + ln].tobytes() for off, ln in part]
    buf = torch.full((size,), PATTERN, dtype=torch.uint8, device="cuda")
    touts, tst = comp.decompress_ranges_tensors(d.stream, d.idx, total_n, [r[0] for r in ranges], [r[1] for r in ranges],
                                                outs=[buf[p: p + r[1]] for r, p in zip(ranges, pos)], subindex=d.sub, block_bytes=bb)
    torch.cuda.synchronize()
    assert (tst.cpu().numpy() == 0).all() and np.array_equal(buf.cpu().numpy(), want)
    touts, tst = comp.decompress_ranges_tensors(d.stream, d.idx, total_n, [r[0] for r in part], [r[1] for r in part], block_bytes=bb)
    torch.cuda.synchronize()
    assert (tst.cpu().numpy() == 0).all()
    for (off, ln), o in zip(part, touts):
        assert o[:ln].cpu().numpy().tobytes() == data[off: off + ln].tobytes()
    for off, ln in ranges[:: max(1, len(ranges) // 12)]:
        got, st1 = comp.decompress_range(stream, idx, total_n, off, ln, s, block_bytes=bb)
        assert st1 == 0 and got == data[off: off + ln].tobytes(), (off, ln)
        one = torch.full((ln + 9,), PATTERN, dtype=torch.uint8, device="cuda")
        st1 = C.c_uint32(99)
        rc = comp._lib.sfh_decompress_range_device(comp._h, d.stream.data_ptr(), d.stream.numel(), d.idx.data_ptr(),
                                                   d.sub.data_ptr() if d.sub is not None else None, d.idx.numel() - 1, total_n, bb,
                                                   off, ln, one.data_ptr() + 3, C.byref(st1), None)
        assert rc == 0 and st1.value == 0
        h = one.cpu().numpy()
        assert h[3: 3 + ln].tobytes() == data[off: off + ln].tobytes() and (h[:3] == PATTERN).all() and (h[3 + ln:] == PATTERN).all()


@pytest.mark.parametrize("kind", ["text", "real", "noise", "mixture"])
@pytest.mark.parametrize("block_bytes", [32768, 65536, 0, 1 << 20])
def test_parity(comp, kind, block_bytes):
    n = (2 << 20) + 70001 if block_bytes == 1 << 20 else 600000 + 12345
    data = _content(kind, n, seed=11)
    for effort in ("default", "best"):
        for container in ("raw", "gzip"):
            stream = comp.compress(data, block_bytes=block_bytes, effort=effort, container=container)
            idx, sub, bb = comp.last_index(), comp.last_subindex(), comp.last_block_bytes()
            _check_all_paths(comp, data, stream, idx, sub, bb, seed=block_bytes + len(effort) + len(container),
                             n_random=120 if block_bytes != 1 << 20 else 40)


def test_parity_whole_multiples_and_tiny(comp):
    for n in (0, 1, 32767, 32768, 32769, 4 * 262144):
        data = synth.gen_text(n, seed=n + 1) if n else np.zeros(0, np.uint8)
        stream = comp.compress(data, block_bytes=262144)
        idx, sub, bb = comp.last_index(), comp.last_subindex(), comp.last_block_bytes()
        _check_all_paths(comp, data, stream, idx, sub, bb, seed=n, n_random=30)


@pytest.mark.parametrize("name", ["starfleet.html.dynamic.flushed", "starfleet.html.fixed.flushed"])
def test_parity_flushed_fixtures(comp, starfleet, name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        stream = f.read()
    idx = np.fromfile(os.path.join(GOLDEN, name + ".index"), dtype="<u8").astype(np.uint64)
    _check_all_paths(comp, np.frombuffer(starfleet, np.uint8), stream, idx, None, 32768, seed=5)


def _damaged(comp, seed0):
    """a 256 KiB-strip stream of 5 strips with one byte flipped inside coded segment 11 (strip 1, its fourth segment), the
    seed chosen so that the serial decoder does not take the damaged stream for a sound one"""
    data = synth.gen_text(5 * 262144 + 4321, seed=77)
    stream = comp.compress(data, block_bytes=262144)
    idx, sub = comp.last_index(), comp.last_subindex()
    assert comp.last_block_bytes() == 262144
    g = 11
    for seed in range(seed0, seed0 + 50):
        rng = np.random.default_rng(seed)
        at = int(rng.integers(int(idx[g]) + 8, int(idx[g + 1]) - 8))
        bad = bytearray(stream)
        bad[at] ^= 1 << int(rng.integers(0, 8))
        st, _, _ = O.decompress(np.frombuffer(bytes(bad), np.uint8), data.size)
        if st != 0:
            return data, stream, bytes(bad), idx, sub, g
    raise AssertionError("no seed damages the stream for the serial decoder")


def _span_holds(off, ln, g, sps):
    """does the decode span of [off, off + ln) hold segment g"""
    return ln > 0 and off // SEG // sps * sps <= g <= (off + ln - 1) // SEG


def test_damage_isolation_and_no_stray_writes(comp):
    data, stream, bad, idx, sub, g = _damaged(comp, 0)
    n, bb, sps = data.size, 262144, 8
    ranges = [(8 * SEG + 5, 1000), (8 * SEG, 3 * SEG), (10 * SEG + 7, SEG - 7),   # strip 1 in front of the damage
              (100, 5000), (7 * SEG + 1, SEG - 1), (16 * SEG, 4 * SEG + 3), (n - 3000, 3000), (3 * 262144 - 5, 262144 + 10),
              (g * SEG + 10, 100), (g * SEG - 1, 2), (10 * SEG + 5, SEG + 10),       # over the damaged segment
              (12 * SEG + 3, 4000), (15 * SEG + 100, SEG - 100), (15 * SEG, SEG + 1),  # behind it in its strip
              (0, n)]
    ranges += random_ranges(np.random.default_rng(3), n, 60)
    pos, size = _layout(ranges, 9)
    hit = [_span_holds(off, ln, g, sps) for off, ln in ranges]
    assert sum(hit) >= 8 and sum(not h for h in hit) >= 20
    d = Dev(bad, idx, sub, n, bb)
    for use_sub in (False, True):
        full, fst = comp.decompress_tensor(d.stream, d.idx, n, block_bytes=bb, subindex=d.sub if use_sub else None)
        got, st = _device_call(comp, d, ranges, pos, size, use_sub)
        for (off, ln), s, h in zip(ranges, st, hit):
            assert (s != 0) == h, (off, ln, int(s), h)
            if h and fst != 0:
                assert s == fst, (off, ln, int(s), fst)
        # the sound ranges hold the input's bytes; whatever a failed range wrote stays inside its destination
        ok = [not h for h in hit]
        want = _expected(data, ranges, pos, size, ok)
        mask = np.ones(size, bool)
        for (off, ln), p, h in zip(ranges, pos, hit):
            if h:
                mask[p: p + ln] = False
        assert np.array_equal(got[mask], want[mask])
    # the host variant: statuses alike, a failed range is not copied back
    outs, st = comp.decompress_ranges(bad, idx, n, [r[0] for r in ranges], [r[1] for r in ranges], sub, block_bytes=bb)
    for (off, ln), o, s, h in zip(ranges, outs, st, hit):
        assert (s != 0) == h
        assert (o is None) if h else (o == data[off: off + ln].tobytes())
    # a wrong sub-index word on the sound stream: an error for exactly the ranges whose span holds that segment
    wrong = np.array(sub, copy=True).reshape(-1)
    wrong[g * 64 + 2 * 5] += 8
    d2 = Dev(stream, idx, wrong, n, bb)
    got, st = _device_call(comp, d2, ranges, pos, size, True)
    assert [(s != 0) for s in st] == hit
    want = _expected(data, ranges, pos, size, [not h for h in hit])
    mask = np.ones(size, bool)
    for (off, ln), p, h in zip(ranges, pos, hit):
        if h:
            mask[p: p + ln] = False
    assert np.array_equal(got[mask], want[mask])
    got, st = _device_call(comp, d2, ranges, pos, size, False)  # without it: all sound
    assert (st == 0).all() and np.array_equal(got, _expected(data, ranges, pos, size))


def test_work_done(comp, monkeypatch):
    data = synth.gen_text(6 * 262144 + 999, seed=21)
    stream = comp.compress(data, block_bytes=262144)
    idx, sub, bb = comp.last_index(), comp.last_subindex(), comp.last_block_bytes()
    assert bb == 262144
    per = SEG * 4
    # a range in the first, a middle and the last segment of a strip; over two strips; with independent segments
    for (off, ln), segs in (((8 * SEG + 100, 4096), 1), ((11 * SEG + 100, 4096), 4), ((15 * SEG + 100, 4096), 8),
                            ((13 * SEG + 5, 5 * SEG), 8 + 3), ((13 * SEG - 1, 2), 6)):
        for s in (None, sub):
            got, st = comp.decompress_range(stream, idx, data.size, off, ln, s, block_bytes=bb)
            assert st == 0 and got == data[off: off + ln].tobytes()
            assert comp.last_decode_scratch_bytes() == segs * per, (off, ln, segs)
    flat = comp.compress(data, block_bytes=32768)
    fidx = comp.last_index()
    got, st = comp.decompress_range(flat, fidx, data.size, 11 * SEG + 100, 4096, block_bytes=32768)
    assert st == 0 and got == data[11 * SEG + 100: 11 * SEG + 4196].tobytes() and comp.last_decode_scratch_bytes() == per
    # smaller launch batches: the scratch stays under the cap (a strip of 8 segments fits it), the bytes are the same
    monkeypatch.setenv("SFH_BATCH_CHUNKS", "16")
    small = Compressor(0)
    monkeypatch.delenv("SFH_BATCH_CHUNKS")
    try:
        ranges = _ranges(data.size, bb, 4, 80)
        pos, size = _layout(ranges, 4)
        d = Dev(stream, idx, sub, data.size, bb)
        for use_sub in (False, True):
            got, st = _device_call(small, d, ranges, pos, size, use_sub)
            assert (st == 0).all() and np.array_equal(got, _expected(data, ranges, pos, size))
            assert 0 < small.last_decode_scratch_bytes() <= 16 * per
        outs, st = small.decompress_ranges(stream, idx, data.size, [r[0] for r in ranges], [r[1] for r in ranges], block_bytes=bb)
        assert (st == 0).all() and outs == [data[o: o + m].tobytes() for o, m in ranges]
        assert small.last_decode_scratch_bytes() <= 16 * per
    finally:
        small.close()
    # a cap below one strip: that strip alone is a batch
    monkeypatch.setenv("SFH_BATCH_CHUNKS", "3")
    tiny = Compressor(0)
    monkeypatch.delenv("SFH_BATCH_CHUNKS")
    try:
        ranges = [(15 * SEG + 100, 4096), (100, 50), (9 * SEG, 2 * SEG), (3 * SEG + 1, 7 * SEG)]
        outs, st = tiny.decompress_ranges(stream, idx, data.size, [r[0] for r in ranges], [r[1] for r in ranges], sub, block_bytes=bb)
        assert (st == 0).all() and outs == [data[o: o + m].tobytes() for o, m in ranges]
        assert tiny.last_decode_scratch_bytes() == 8 * per
    finally:
        tiny.close()


def test_inflate_ms_after_a_range_call(comp):
    data = synth.gen_text(300000, seed=2)
    stream = comp.compress(data, block_bytes=65536)
    idx = comp.last_index()
    comp.set_profiling(True)
    try:
        got, st = comp.decompress_range(stream, idx, data.size, 70000, 5000, block_bytes=65536)
        ms = comp.inflate_ms()
    finally:
        comp.set_profiling(False)
    assert st == 0 and got == data[70000:75000].tobytes()
    assert set(ms) == {"k_inflate_tokens", "k_inflate_bytes"} and all(v > 0 for v in ms.values())


def test_lane_serial_mode_agrees(comp, monkeypatch):
    monkeypatch.setenv("SFH_INFLATE_SERIAL", "1")
    serial = Compressor(0)
    monkeypatch.delenv("SFH_INFLATE_SERIAL")
    try:
        data, stream, bad, idx, sub, g = _damaged(comp, 100)
        n, bb = data.size, 262144
        ranges = _ranges(n, bb, 6, 60)
        pos, size = _layout(ranges, 6)
        for s_bytes in (stream, bad):
            d = Dev(s_bytes, idx, sub, n, bb)
            a, ast = _device_call(comp, d, ranges, pos, size, False)
            b, bst = _device_call(serial, d, ranges, pos, size, False)
            assert np.array_equal(ast, bst)
            mask = np.ones(size, bool)
            for (off, ln), p, s in zip(ranges, pos, ast):
                if s:
                    mask[p: p + ln] = False
            assert np.array_equal(a[mask], b[mask])
            if s_bytes is stream:
                assert (ast == 0).all() and np.array_equal(a, _expected(data, ranges, pos, size))
            else:
                assert [s != 0 for s in ast] == [_span_holds(off, ln, g, 8) for off, ln in ranges]
    finally:
        serial.close()


def test_neighbours_unchanged_and_refusals_write_nothing(comp):
    data = synth.gen_text(700000, seed=31)
    stream = comp.compress(data, block_bytes=131072)
    idx, sub, bb = comp.last_index(), comp.last_subindex(), comp.last_block_bytes()
    d = Dev(stream, idx, sub, data.size, bb)
    before, st0 = comp.decompress_tensor(d.stream, d.idx, data.size, block_bytes=bb, subindex=d.sub)
    before = before.cpu().numpy().copy()
    bouts0, bst0 = comp.decompress_batch([stream, stream], [data.size] * 2, index=np.concatenate([idx, idx]), block_bytes=[bb, bb])
    ranges = _ranges(data.size, bb, 8, 50)
    pos, size = _layout(ranges, 8)
    got, st = _device_call(comp, d, ranges, pos, size)
    assert (st == 0).all() and np.array_equal(got, _expected(data, ranges, pos, size))
    assert comp._lib.sfh_index_entries(comp._h) == 0
    after, st1 = comp.decompress_tensor(d.stream, d.idx, data.size, block_bytes=bb, subindex=d.sub)
    assert st0 == 0 and st1 == 0 and np.array_equal(after.cpu().numpy(), before) and before.tobytes() == data.tobytes()
    bouts1, bst1 = comp.decompress_batch([stream, stream], [data.size] * 2, index=np.concatenate([idx, idx]), block_bytes=[bb, bb])
    assert bst0 == bst1 == [0, 0] and bouts0 == bouts1 == [data.tobytes()] * 2
    # refusals with a context: nothing is enqueued, nothing written
    lib, vp = comp._lib, C.c_void_p
    buf = torch.full((1 << 16,), PATTERN, dtype=torch.uint8, device="cuda")
    stt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    nseg = idx.size - 1

    def call(offs, lens, dsts, src=d.stream.data_ptr(), index=d.idx.data_ptr(), subp=None, nseg=nseg, total=data.size, bbv=bb,
             status=stt.data_ptr(), k=2):
        return lib.sfh_decompress_ranges_device_async(comp._h, src, d.stream.numel(), index, subp, nseg, total, bbv, k,
                                                      (C.c_uint64 * k)(*offs), (C.c_uint64 * k)(*lens), (vp * k)(*dsts), vp(status), None)

    base = buf.data_ptr()
    assert call([0, 10], [100, 100], [base, base + 50]) == -1                 # overlapping destinations
    assert call([0, data.size - 5], [100, 6], [base, base + 200]) == -1       # behind total_n
    assert call([0, (1 << 64) - 1], [100, 2], [base, base + 200]) == -1       # overflowing
    assert call([0, 10], [100, 100], [base, None]) == -1                      # a null destination with a length
    assert call([0, 10], [100, 100], [base, base + 200], nseg=nseg + 1) == -1
    assert call([0, 10], [100, 100], [base, base + 200], bbv=1000) == -1
    assert call([0, 10], [100, 100], [base, base + 200], src=d.stream.data_ptr() + 2) == -1
    assert call([0, 10], [100, 100], [base, base + 200], index=d.idx.data_ptr() + 4) == -1
    assert call([0, 10], [100, 100], [base, base + 200], subp=d.sub.data_ptr() + 2) == -1
    assert call([0, 10], [100, 100], [base, base + 200], status=stt.data_ptr() + 2) == -1
    assert lib.sfh_decompress_ranges_device_async(comp._h, d.stream.data_ptr(), d.stream.numel(), d.idx.data_ptr(), None, nseg,
                                                  data.size, bb, 2, None, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert (buf == PATTERN).all() and (stt == -1).all()
    assert lib.sfh_decompress_ranges_device_async(comp._h, None, 0, None, None, nseg, data.size, bb, 0, None, None, None, None, None) == 0
    # a destination of no bytes, null or inside another's, overlaps nothing; ranges may overlap each other
    assert call([5, 7], [100, 0], [base + 1, None]) == 0
    assert call([5, 50], [100, 100], [base + 1, base + 301]) == 0
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert h[1:101].tobytes() == data[5:105].tobytes() and h[301:401].tobytes() == data[50:150].tobytes()
    assert (h[:1] == PATTERN).all() and (h[101:301] == PATTERN).all() and (h[401:] == PATTERN).all()
    assert (stt[:2] == 0).all()
