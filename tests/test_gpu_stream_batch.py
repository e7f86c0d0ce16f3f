"""Batches of streams without flush points decoded in one call (sfh_inflate_stream_batch*, Compressor.decompress_stream_batch,
DESIGN.md 3a "Batches of streams without flush points").  Every item is compared with the single call on it alone (status,
output size, bytes), with the serial decoder of container.hpp for the status and with zlib for the bytes.  Each case runs on a
default context and on one with 512-byte nominal chunks, where small items carry many speculative starts and repairs."""
import ctypes as C
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import stream_host as H
import starflate_amd
from starflate_amd import Compressor, synth

pytestmark = pytest.mark.gpu

OK, ERROR, INVALID_BLOCK_HEADER, DST_TOO_SMALL = 0, 1, 2, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY,
              "rle": zlib.Z_RLE, "fixed": zlib.Z_FIXED}


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


def _zlib(data, container="raw", level=6, mem=8, strategy="default"):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[container], mem, STRATEGIES[strategy])
    return c.compress(data) + c.flush()


def _mixed(n, seed):
    return synth.gen_mixed(n, seed=seed, stripe=40000).tobytes() if n else b""


def _stats(c):
    return c.last_stream_stats()


def _check_batch(c, streams, container, caps):
    """the batch (host buffers) against the single call on every item alone, container.hpp and zlib -> (statuses, per-item stats)"""
    outs, sts = c.decompress_stream_batch(streams, caps, container)
    assert len(outs) == len(sts) == len(streams)
    singles = []
    for i, (s, cap) in enumerate(zip(streams, caps)):
        out1, st1 = c.decompress_stream(s, cap, container)
        singles.append(_stats(c))
        assert sts[i] == st1, (i, sts[i], st1)
        assert outs[i] == out1, i
        want_st = H.serial(s, container, cap)[0]
        if not (container == "zlib" and want_st == ERROR and st1 == OK):  # (a zlib dst larger than the output: documented)
            assert st1 == want_st, (i, st1, want_st)
        if sts[i] == OK:
            try:
                assert outs[i] == zlib.decompressobj(WBITS[container]).decompress(s)
            except zlib.error:  # (zlib refuses incomplete literal/length codes; the serial decoder takes them)
                assert container == "raw"
    return sts, singles


def _items(c, container, sizes_n=(0, 1, 32767, 32768, 32769, 150001)):
    """items of one container: zlib settings and sizes, gzip.compress output, starflate's own streams, stored DEFLATE payloads"""
    items = []
    data = _mixed(150001, 3)
    for level in list(range(10)) + [-1]:
        items.append(_zlib(data[: 20000 + 997 * (level + 1)], container, level))
    for strategy in STRATEGIES:
        items.append(_zlib(data[:70000], container, 6, 8, strategy))
    for mem in (1, 8, 9):
        items.append(_zlib(data[:90000], container, 6, mem))
    for n in sizes_n:
        items.append(_zlib(_mixed(n, n % 97), container))
    if container == "gzip":
        items.append(gzip.compress(synth.gen_text(100001, seed=5).tobytes()))
    items.append(c.compress(np.frombuffer(_mixed(200000, 7), np.uint8), container=container))
    inner = _zlib(synth.gen_text(60000, seed=9).tobytes(), "raw", 6, 1)
    items.append(_zlib(inner, container, 0))  # stored DEFLATE data
    items.append(_zlib(zlib.compress(synth.gen_text(80000, seed=4).tobytes(), 6), container, 6))
    return items


def _size(s, container):
    return len(zlib.decompressobj(WBITS[container]).decompress(s))


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
def test_mixed_batch(comp, small, container):
    items = _items(comp, container)
    if container == "raw":
        for name in ("starfleet.html.dynamic", "starfleet.html.fixed"):
            with open(os.path.join(GOLDEN, name), "rb") as f:
                items.append(f.read())
    caps = [_size(s, container) for s in items]
    for c in (comp, small):
        sts, _ = _check_batch(c, items, container, caps)
        assert all(st == OK for st in sts), sts


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
def test_five_mib_items(comp, container):
    items = [_zlib(_mixed(5 << 20, 1), container), _zlib(_mixed(1000, 2), container), _zlib(_mixed(5 << 20, 3), container, 1)]
    sts, _ = _check_batch(comp, items, container, [_size(s, container) for s in items])
    assert sts == [OK] * 3


def _damaged(container):
    rng = np.random.default_rng(77)
    good = [_zlib(_mixed(60000 + 1000 * k, k), container, 6) for k in range(6)]
    items, caps = [], []
    n0 = _size(good[0], container)

    def add(s, cap):
        items.append(s)
        caps.append(cap)
        g = good[len(items) % len(good)]
        items.append(g)
        caps.append(_size(g, container))

    add(good[0][:-1], n0)
    add(good[0][: len(good[0]) // 2], n0)
    for _ in range(4):
        b = bytearray(good[1])
        p = int(rng.integers(len(b) // 4, len(b) // 2))
        b[p] ^= 1 << int(rng.integers(0, 8))
        add(bytes(b), _size(good[1], container))
    hdr = {"raw": 0, "zlib": 2, "gzip": 10}[container]
    b = bytearray(good[2])
    b[hdr] |= 0x06  # BTYPE 3 on the first block
    add(bytes(b), _size(good[2], container))
    if container != "raw":
        b = bytearray(good[3])
        b[-5 if container == "gzip" else -1] ^= 0x10  # the CRC-32 / Adler-32
        add(bytes(b), _size(good[3], container))
    if container == "gzip":
        b = bytearray(good[4])
        b[-4:] = (_size(good[4], container) + 1000).to_bytes(4, "little")  # ISIZE above the capacity
        add(bytes(b), _size(good[4], container))
    if container == "zlib":
        b = bytearray(good[4])
        b[1] ^= 1  # FCHECK
        add(bytes(b), _size(good[4], container))
    add(good[5], _size(good[5], container) - 1)  # a capacity one short
    add(b"" if container == "raw" else good[0][:3], 100)
    return items, caps


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
def test_isolation(comp, small, container):
    """damaged items between good ones; every destination carved from one allocation with guard bands around it"""
    items, caps = _damaged(container)
    guard = 4096
    offs, o = [], guard
    for cap in caps:
        offs.append(o)
        o = (o + cap + guard + 15) // 16 * 16
    for c in (comp, small):
        want = [c.decompress_stream(s, cap, container) for s, cap in zip(items, caps)]
        buf = torch.full((o + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        srcs = [torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda() if s else torch.empty(0, dtype=torch.uint8, device="cuda")
                for s in items]
        outs = [buf[a: a + cap] if cap else buf[a: a] for a, cap in zip(offs, caps)]
        got, sts = c.decompress_stream_batch_tensors(srcs, caps, container, outs=outs)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        mask = np.ones(host.size, bool)
        for i, (a, cap) in enumerate(zip(offs, caps)):
            assert sts[i] == want[i][1], (i, sts[i], want[i][1])
            if sts[i] == OK:
                assert got[i].cpu().numpy().tobytes() == want[i][0]
            elif sts[i] != ERROR:  # (only a checksum mismatch may leave written bytes behind)
                assert (host[a: a + cap] == 0xA5).all(), i
            mask[a: a + cap] = False
        assert (host[mask] == 0xA5).all(), "bytes written outside the destinations"
        assert all(st == OK for st in sts[1::2]), sts  # (the good neighbours)
        assert sum(st != OK for st in sts[0::2]) >= 5, sts  # (a bit flip in a raw body may still decode)


def test_follow_lanes_stay_inside(small):
    """stored DEFLATE data back to back with 512-byte chunks: the follow lanes run through false candidates up to their item's
    end and never into the next item"""
    items = []
    for k in range(5):
        inner = _zlib(synth.gen_text(300000, seed=10 * k).tobytes(), "raw", 6, 1)  # (memLevel 1: many blocks)
        items.append(_zlib(inner, "zlib", 0 if k % 2 == 0 else 6))  # (level 0: stored blocks of DEFLATE data)
    caps = [_size(s, "zlib") for s in items]
    sts, singles = _check_batch(small, items, "zlib", caps)
    assert sts == [OK] * len(items)
    small.decompress_stream_batch(items, caps, "zlib")
    b = _stats(small)
    assert b["repair_rounds"] == max(s["repair_rounds"] for s in singles), (b, singles)
    for key in ("chunks", "candidates", "confirmed"):
        assert b[key] == sum(s[key] for s in singles), (key, b, singles)
    assert b["longest_chunk"] == max(s["longest_chunk"] for s in singles)
    assert b["candidates"] > b["confirmed"] and b["repair_rounds"] >= 1, b


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
def test_size_query(comp, small, container):
    items, _ = _damaged(container)
    items += _items(comp, container, (0, 1, 40000))
    for c in (comp, small):
        outs, sts = c.decompress_stream_batch(items, None, container)
        n = (C.c_uint64 * len(items))()
        st = (C.c_uint32 * len(items))()
        srcs = [np.frombuffer(s, np.uint8) for s in items]
        sp = (C.c_void_p * len(items))(*[a.ctypes.data if a.size else None for a in srcs])
        assert c._lib.sfh_inflate_stream_batch(c._h, len(items), sp, (C.c_uint64 * len(items))(*[a.size for a in srcs]),
                                               starflate_amd._capi.CONTAINER[container], None, None, n, st) == 0
        for i, s in enumerate(items):
            one_n, one_st = C.c_uint64(0), C.c_uint32(0)
            a = srcs[i]
            assert c._lib.sfh_inflate_stream(c._h, a.ctypes.data if a.size else None, a.size, starflate_amd._capi.CONTAINER[container],
                                             None, 0, C.byref(one_n), C.byref(one_st)) == 0
            assert (n[i], st[i]) == (one_n.value, one_st.value), i
            assert (outs[i], sts[i]) == c.decompress_stream(s, None, container), i


def test_launch_batches(comp, tiny_batches):
    """SFH_BATCH_CHUNKS=4 (128 KiB of output per launch batch): items straddle the limits and a 1 MiB item runs alone; the
    results equal the default context's and the scratch stays within its bound"""
    sizes = [50000, 70000, 30000, 1 << 20, 100000, 131072, 1, 0, 90000, 60000]
    for container in ("raw", "zlib", "gzip"):
        items = [_zlib(_mixed(n, k), container, 6 if k % 2 else 1) for k, n in enumerate(sizes)]
        caps = [n + 100 if container == "zlib" else n for n in sizes]
        a = comp.decompress_stream_batch(items, caps, container)
        b = tiny_batches.decompress_stream_batch(items, caps, container)
        assert a == b
        assert a[1] == [OK] * len(items), a[1]
        st = _stats(tiny_batches)
        # 60 bytes per nominal chunk (16-byte aligned arrays), and one launch batch: at most 2 bytes per output byte of the
        # largest (128 KiB, or the 1 MiB item alone, 16-entry aligned) and 64 KiB per group
        recs = 60 * st["chunks"] + 64
        wins = 65536 * st["confirmed"]
        assert st["scratch_bytes"] <= recs + 2 * ((1 << 20) + 16) + wins, st
        assert st["scratch_bytes"] == tiny_batches.last_decode_scratch_bytes()
    _check_batch(tiny_batches, items, "gzip", caps)


def test_counts(comp, small):
    assert comp.decompress_stream_batch([], None, "zlib") == ([], [])
    assert comp.decompress_stream_batch([], [], "raw") == ([], [])
    data = _mixed(100000, 8)
    s = _zlib(data, "gzip")
    assert comp.decompress_stream_batch([s], [len(data)], "gzip") == ([data], [OK])
    rng = np.random.default_rng(5)
    payloads = [rng.integers(0, 4, int(rng.integers(0, 200)), dtype=np.uint8).tobytes() for _ in range(10000)]
    items = [zlib.compress(p, int(k % 10)) for k, p in enumerate(payloads)]
    for c in (comp, small):
        outs, sts = c.decompress_stream_batch(items, None, "zlib")
        assert sts == [OK] * len(items)
        assert outs == payloads


def test_entry_points(comp):
    """host buffers, device buffers and the module-level function agree"""
    items = [_zlib(_mixed(n, n % 13), "gzip") for n in (0, 5000, 40000, 300000)]
    items.append(items[1][:-3])
    caps = [_size(s, "gzip") if k < 4 else 5000 for k, s in enumerate(items)]
    outs, sts = comp.decompress_stream_batch(items, caps, "gzip")
    srcs = [torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda() for s in items]
    touts, tsts = comp.decompress_stream_batch_tensors(srcs, caps, "gzip")
    assert tsts == sts
    assert [t.cpu().numpy().tobytes() for t in touts] == outs
    touts, tsts = comp.decompress_stream_batch_tensors(srcs, None, "gzip")  # (each item's own size query first)
    assert [(t.cpu().numpy().tobytes(), st) for t, st in zip(touts, tsts)] == [comp.decompress_stream(s, None, "gzip") for s in items]
    assert starflate_amd.decompress_stream_batch(items, caps, "gzip") == (outs, sts)
    assert sts[:4] == [OK] * 4 and sts[4] != OK


def test_cpp_host_api(tmp_path):
    """tests/cpp/stream_batch.cpp: compressor::decompress_stream_batch against starflate::decompress on every item"""
    from starflate_amd import build

    lib = build.build()
    exe = tmp_path / "stream_batch"
    libdir = os.path.dirname(lib)
    flags = ["-std=c++23", "-fno-exceptions", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror", "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(["/opt/rocm/llvm/bin/clang++", "-O2"] + flags + [os.path.join(ROOT, "tests", "cpp", "stream_batch.cpp"),
                                                                          "-L" + libdir, "-lstarflate_hip", "-Wl,-rpath," + libdir,
                                                                          "-o", str(exe)])
    r = subprocess.run([str(exe), GOLDEN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
