"""Streams without side information or flush points, decoded on the GPU (sfh_inflate_stream*, Compressor.decompress_stream,
DESIGN.md 3a "Streams without flush points").  Every result is compared with the serial decoder: container.hpp's
decompress(src, dst, container) for the status, zlib for the bytes.  A second context with 512-byte nominal chunks puts
hundreds of speculative starts into small streams, so the chain and its repairs are exercised everywhere."""
import gzip
import os
import zlib

import numpy as np
import pytest
import torch

import deflate_writer as W
import starflate_amd
import stream_host as H
from starflate_amd import Compressor, StarflateError, synth
from stream_cases import write_fixed

pytestmark = pytest.mark.gpu

OK, ERROR, DST_TOO_SMALL = 0, 1, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY,
              "rle": zlib.Z_RLE, "fixed": zlib.Z_FIXED}


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(monkeypatch_module):
    monkeypatch_module.setenv("SFH_STREAM_CHUNK", "512")
    c = Compressor(0)
    monkeypatch_module.delenv("SFH_STREAM_CHUNK")
    yield c
    c.close()


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def _zlib(data, container="raw", level=6, mem=8, strategy="default"):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[container], mem, STRATEGIES[strategy])
    return c.compress(data) + c.flush()


def _mixed(n, seed):
    return synth.gen_mixed(n, seed=seed, stripe=40000).tobytes() if n else b""


def _check(c, stream, container, cap):
    """GPU status == serial status; Success only with the serial decoder's (and zlib's) bytes.  -> status"""
    want_st, _, want = H.serial(stream, container, cap)
    out, st = c.decompress_stream(stream, cap, container)
    assert st == want_st, (st, want_st)
    if st == OK:
        try:
            assert out == zlib.decompressobj(WBITS[container]).decompress(stream)
        except zlib.error:  # (zlib refuses incomplete literal/length codes; the serial decoder takes them)
            assert container == "raw"
        if container != "zlib":  # (container.hpp's zlib dst is the output size exactly)
            assert out == want[: len(out)].tobytes()
    return st


def _roundtrip(c, stream, container, n):
    st = _check(c, stream, container, n)
    assert st == OK
    return st


@pytest.mark.parametrize("name", ["starfleet.html.dynamic", "starfleet.html.fixed"])
def test_golden(comp, small, name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        stream = f.read()
    with open(os.path.join(GOLDEN, "starfleet.html"), "rb") as f:
        data = f.read()
    for c in (comp, small):
        out, st = c.decompress_stream(stream, None, "raw")
        assert st == OK and out == data
    assert starflate_amd.decompress_stream(stream) == data


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
@pytest.mark.parametrize("mem", [1, 8, 9])
def test_zlib_matrix(comp, small, container, mem):
    data = _mixed(150000 + mem, mem)
    for level in range(10):
        for strategy in STRATEGIES:
            if strategy != "default" and level not in (1, 6, 9):
                continue
            stream = _zlib(data, container, level, mem, strategy)
            _roundtrip(small if (level + mem) % 2 else comp, stream, container, len(data))


def test_gzip_module(comp, small):
    data = synth.gen_text(300001, seed=5).tobytes()
    stream = gzip.compress(data)
    for c in (comp, small):
        assert c.decompress_stream(stream, None, "gzip") == (data, OK)
    assert starflate_amd.decompress_stream(stream, container="gzip") == data


@pytest.mark.parametrize("n", [0, 1, 32767, 32768, 32769, 5 << 20])
@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
def test_sizes(comp, small, n, container):
    data = _mixed(n, n % 97)
    stream = _zlib(data, container)
    _roundtrip(comp, stream, container, n)
    if n <= 32769:
        _roundtrip(small, stream, container, n)
        _roundtrip(small, _zlib(data, container, 0), container, n)


def test_large(comp):
    """a 256 MiB text stream: many chunks, the window carried across ~sqrt(N) groups"""
    data = synth.gen_text(256 << 20, seed=11).tobytes()
    stream = _zlib(data, "zlib", 6)
    t = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
    out, st = comp.decompress_stream_tensor(t, len(data), "zlib")
    assert st == OK and out.numel() == len(data)
    assert np.array_equal(out.cpu().numpy(), np.frombuffer(data, np.uint8))
    s = comp.last_stream_stats()
    assert s["confirmed"] > 1000 and s["scratch_bytes"] >= 2 * len(data)


def test_parallel_chain(comp):
    """16 MiB of zlib -6 text: hundreds of confirmed chunks and at most 2 repair rounds -- not a serial decode in disguise"""
    data = synth.gen_text(16 << 20, seed=3).tobytes()
    stream = _zlib(data, "zlib", 6)
    assert comp.decompress_stream(stream, len(data), "zlib") == (data, OK)
    s = comp.last_stream_stats()
    assert s["confirmed"] >= 200, s
    assert s["repair_rounds"] <= 2, s
    assert s["longest_chunk"] < 4 << 20, s


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
def test_library_streams(comp, small, container):
    data = np.frombuffer(_mixed(400000, 7), np.uint8)
    for bb in (None, 64 << 10):
        stream = comp.compress(data, container=container, **({"block_bytes": bb} if bb else {}))
        _roundtrip(small, stream, container, data.size)
        _roundtrip(comp, stream, container, data.size)


def _writer_stream(kind, seed):
    """blocks from tests/deflate_writer.py: incomplete codes, one distance code, long fixed and stored runs"""
    rng = np.random.default_rng(seed)
    bw = W.BitWriter()
    out = bytearray()
    nblocks = 40
    for b in range(nblocks):
        final = b == nblocks - 1
        lits = rng.integers(97, 123, 200, dtype=np.uint8)
        toks = [int(x) for x in lits]
        out += bytes(lits)
        for _ in range(30):
            ln = int(rng.integers(3, 259))
            d = 8 if kind == "one_dist" else int(rng.integers(1, min(len(out), 32768) + 1))
            toks.append(W.match(ln, d))
            for _ in range(ln):
                out.append(out[-d])
        if kind == "fixed" and b % 2:
            write_fixed(bw, toks, final)
            continue
        ll_f, d_f = W.token_symbols(np.asarray(toks, np.uint32))
        if kind == "incomplete":
            ll = [9 if (i < len(ll_f) and ll_f[i]) or i == 256 else 0 for i in range(286)]
            dl = [6 if i < len(d_f) and d_f[i] else 0 for i in range(30)]
        else:
            ll = W.package_merge(ll_f, 15)
            ll = [int(x) for x in ll]
            if not ll[256]:
                ll = W.package_merge(np.asarray(ll_f) + (np.arange(len(ll_f)) == 256), 15)
            dl = [1 if i == W.dist_symbol(8)[0] else 0 for i in range(30)] if kind == "one_dist" else \
                [int(x) for x in W.package_merge(d_f, 15)]
        W.write_dynamic(bw, toks, ll, dl, final=final)
        if kind == "stored" and b % 3 == 1:
            piece = bytes(rng.integers(0, 256, 20000, dtype=np.uint8))
            W.write_stored(bw, piece, final=False)
            out += piece
    return bw.bytes().tobytes(), bytes(out)


@pytest.mark.parametrize("kind", ["incomplete", "one_dist", "fixed", "stored"])
def test_writer_streams(comp, small, kind):
    stream, data = _writer_stream(kind, {"incomplete": 1, "one_dist": 2, "fixed": 3, "stored": 4}[kind])
    st, n, want = H.serial(stream, "raw", len(data))
    assert st == OK and n == len(data) and want.tobytes() == data
    for c in (comp, small):
        _roundtrip(c, stream, "raw", len(data))
        assert c.decompress_stream(stream, None, "raw") == (data, OK)


def test_deflate_payload(comp, small):
    """a level-0 stream whose payload is itself a DEFLATE stream: false candidates everywhere, none of them taken"""
    inner = _zlib(synth.gen_text(600000, seed=9).tobytes(), "raw", 6, 1)  # (memLevel 1: many blocks, many candidates)
    stream = _zlib(inner, "zlib", 0)
    for c in (comp, small):
        _roundtrip(c, stream, "zlib", len(inner))
    small.decompress_stream(stream, len(inner), "zlib")
    assert small.last_stream_stats()["candidates"] > 10


def test_damaged(comp, small):
    rng = np.random.default_rng(2026)
    data = _mixed(120000, 1)
    sources = [("raw", _zlib(data, "raw", 6)), ("zlib", _zlib(data, "zlib", 9, 9)), ("gzip", gzip.compress(data)),
               ("raw", _zlib(data, "raw", 1, 1, "fixed")), ("zlib", comp.compress(np.frombuffer(data, np.uint8), container="zlib"))]
    seen = {}
    for case in range(120):
        container, src = sources[case % len(sources)]
        b = bytearray(src)
        kind = case % 4
        if kind == 0:
            for _ in range(1 + case % 3):
                p = int(rng.integers(0, len(b)))
                b[p] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            b = b[: int(rng.integers(0, len(b)))]
        elif kind == 2:
            p = int(rng.integers(max(0, len(b) - 8), len(b)))  # the trailer: Adler-32 / CRC-32 / ISIZE
            b[p] ^= 1 << int(rng.integers(0, 8))
        else:
            p = int(rng.integers(0, len(b)))
            b[p] = int(rng.integers(0, 256))
        st = _check(small if case % 2 else comp, bytes(b), container, len(data))
        seen[st] = seen.get(st, 0) + 1
    assert sum(v for k, v in seen.items() if k != OK) > 60, seen


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
def test_dst_one_short(comp, small, container):
    data = _mixed(200000, 2)
    stream = _zlib(data, container)
    for c in (comp, small):
        assert _check(c, stream, container, len(data) - 1) == DST_TOO_SMALL
        assert _check(c, _zlib(data, container, 0), container, len(data) - 1) == DST_TOO_SMALL


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
def test_size_query(comp, small, container):
    data = _mixed(777777, 4)
    stream = _zlib(data, container, 5)
    t = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
    for c in (comp, small):
        out, st = c.decompress_stream_tensor(t, None, container)
        assert st == OK and out.cpu().numpy().tobytes() == data
        out, st = c.decompress_stream(stream, None, container)
        assert st == OK and out == data


def test_top_level_raises(comp):
    stream = bytearray(_zlib(_mixed(50000, 3), "zlib"))
    stream[-1] ^= 1
    with pytest.raises(StarflateError) as e:
        starflate_amd.decompress_stream(bytes(stream), container="zlib")
    assert e.value.code == ERROR


@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_empty_damaged_trailer_tensor(comp, container):
    """an empty body with a damaged trailer through the tensor API, with out_n None and 0: the status is the serial
    decoder's (a real decode always checks the trailer; only a null dst with capacity 0 is the size query) -- with out_n 0 at
    capacity 0, with out_n None (a size query first) at a capacity that is no obstacle: a gzip decode behind a query has room
    for ISIZE, so an ISIZE above the empty body is Error, not DstTooSmall"""
    good = zlib.compress(b"") if container == "zlib" else gzip.compress(b"")
    bad = [good[:-1] + bytes([good[-1] ^ 1])]  # Adler-32 / ISIZE
    if container == "gzip":
        bad += [good[:-8] + bytes([good[-8] ^ 1]) + good[-7:], good[:-4] + (7).to_bytes(4, "little")]  # CRC-32, ISIZE 7
    for stream in [good] + bad:
        t = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
        isize = int.from_bytes(stream[-4:], "little") if container == "gzip" else 0
        for out_n in (None, 0):
            want = H.serial(stream, container, isize if out_n is None else 0)[0]
            out, st = comp.decompress_stream_tensor(t, out_n, container)
            assert st == want and out.numel() == 0, (stream, out_n, st, want)
        want = H.serial(stream, container, 0)[0]
        assert comp.decompress_stream(stream, 0, container)[1] == want
    assert H.serial(bad[0], container, 0)[0] != OK


def test_zlib_larger_dst(comp):
    """a zlib dst larger than the output: Success with the output, the Adler-32 checked over the bytes produced (container.hpp
    checks it over all of dst and answers Error there: the one documented difference)"""
    data = _mixed(100000, 6)
    stream = _zlib(data, "zlib")
    assert comp.decompress_stream(stream, len(data) + 1000, "zlib") == (data, OK)
    bad = stream[:-1] + bytes([stream[-1] ^ 2])
    assert comp.decompress_stream(bad, len(data) + 1000, "zlib")[1] == ERROR


def test_stored_deflate_one_round(comp):
    """stored blocks full of DEFLATE data (gzip files packed again): a false candidate in nearly every nominal chunk, mended in
    at most two repair rounds, not one round per stored block"""
    inner = b"".join(zlib.compress(synth.gen_text(1 << 20, seed=s).tobytes(), 6) for s in range(6))
    stream = _zlib(inner, "zlib", 6)  # (zlib stores what it cannot compress)
    assert comp.decompress_stream(stream, len(inner), "zlib") == (inner, OK)
    s = comp.last_stream_stats()
    assert s["candidates"] > 50, s
    assert s["repair_rounds"] <= 2, s
