"""Decoding without side information (sfh_recover_index*, sfh_decompress_any*): the GPU recovers exactly the
index the compressing call wrote, and the Python walk rule's index for zlib's flushed streams; strips show as independent
segments; stored payloads full of flush markers and fake headers cost nothing and fool nothing; and whatever the damage,
Success comes only with zlib's own bytes."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import starflate_amd
import unindexed_walk as W
from starflate_amd import Compressor, StarflateError, synth

pytestmark = pytest.mark.gpu

SEG = 32768
OK, ERROR = 0, 1
NOT_INDEXABLE = -8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


def _data(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "text":
        return synth.gen_text(n, seed=seed)
    if kind == "noise":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "mixed":
        return synth.gen_mixed(n, seed=seed, stripe=3 * SEG + 1000)
    # noise-head chunks: every 32 KiB chunk starts with 8 KiB of noise, then text
    d = synth.gen_text(n, seed=seed)
    for c0 in range(0, n, SEG):
        m = min(8192, n - c0)
        d[c0:c0 + m] = rng.integers(0, 256, m, dtype=np.uint8)
    return d


def _recover(comp, stream, n, container):
    t = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
    ix, dep = comp.recover_index(t, n, container)
    return ix.cpu().numpy().astype(np.uint64), dep.cpu().numpy()


def _check_written(comp, data, container="raw", **kw):
    n = data.size
    stream = comp.compress(data, container=container, **kw)
    want = comp.last_index()
    bb = comp.last_block_bytes()
    ix, dep = _recover(comp, stream, n, container)
    assert np.array_equal(ix, want), "recovered index differs from the compressing call's"
    sps = bb // SEG
    assert not dep[::sps].any(), "a strip start depends on the segment before it"
    out, st = comp.decompress_any(stream, n, container)
    assert st == OK and out == data.tobytes()
    return stream


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
@pytest.mark.parametrize("n", [0, 1, 32767, 32768, 32769, (3 << 20) + 1])
def test_sizes_containers(comp, container, n):
    _check_written(comp, _data("mixed", n, n + 1), container)


@pytest.mark.parametrize("effort", ["default", "fastest", "thorough", "recent_all", "best"])
@pytest.mark.parametrize("block_bytes", [32768, 256 << 10, 0])
def test_efforts_strips(comp, effort, block_bytes):
    _check_written(comp, _data("text", (2 << 20) + 5, 7), block_bytes=block_bytes, effort=effort)


@pytest.mark.parametrize("strategy", ["auto", "stored", "fixed", "dynamic"])
@pytest.mark.parametrize("kind", ["text", "noise", "mixed", "zeros", "noisehead"])
def test_strategies_inputs(comp, strategy, kind):
    _check_written(comp, _data(kind, (1 << 20) + 3 * SEG + 11, 3), strategy=strategy, block_bytes=128 << 10)


def test_final_stream_concatenation(comp):
    a, b = _data("text", 5 * SEG, 1), _data("noise", 3 * SEG + 9, 2)
    sa = comp.compress(a, final_stream=False, block_bytes=64 << 10)
    ia = comp.last_index()
    sb = comp.compress(b, block_bytes=64 << 10)
    ib = comp.last_index()
    stream = sa + sb
    want = np.concatenate([ia[:-1], ib + np.uint64(len(sa))])
    ix, _ = _recover(comp, stream, a.size + b.size, "raw")
    assert np.array_equal(ix, want)
    out, st = comp.decompress_any(stream, a.size + b.size)
    assert st == OK and out == a.tobytes() + b.tobytes()


def test_adversarial_stored_payloads(comp):
    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, 64 * SEG + 77, dtype=np.uint8)
    for off in range(123, data.size - 8, 300):
        data[off:off + 4] = (0, 0, 0xFF, 0xFF)
    for off in range(250, data.size - 8, 700):
        data[off:off + 5] = (rng.integers(0, 2), 0, 0x80, 0xFF, 0x7F)
    stream = _check_written(comp, data, strategy="stored")
    assert comp.last_recover_stats()["nodes"] > 64 * 100
    _check_written(comp, data)


def test_tar_of_flushed_streams(comp):
    # pieces that are themselves zlib streams flushed every 32 KiB, inside a stream of this library
    parts = []
    for k in range(12):
        d = _data("text", 50000 + 3000 * k, k).tobytes()
        parts.append(struct.pack("<I", k) * 128 + W.zlib_flushed(d, 6, zlib.Z_SYNC_FLUSH, -15, True, 4096))
    data = np.frombuffer(b"".join(parts), np.uint8).copy()
    _check_written(comp, data)
    _check_written(comp, data, strategy="stored")


@pytest.mark.parametrize("container", ["raw", "zlib", "gzip"])
@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("flush", [zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH])
@pytest.mark.parametrize("finish_block", [True, False])
def test_foreign_zlib(comp, container, level, flush, finish_block):
    data = _data("mixed", 9 * SEG + 321, level).tobytes()
    stream = W.zlib_flushed(data, level, flush, WBITS[container], finish_block)
    ix, _ = _recover(comp, stream, len(data), container)
    assert ix.tolist() == W.recover_index(stream, len(data), container)
    out, st = comp.decompress_any(stream, len(data), container)
    assert st == OK and out == data


@pytest.mark.parametrize("name", ["starfleet.html.dynamic.flushed", "starfleet.html.fixed.flushed"])
def test_golden(comp, name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        stream = f.read()
    with open(os.path.join(GOLDEN, "starfleet.html"), "rb") as f:
        data = f.read()
    want = np.fromfile(os.path.join(GOLDEN, name + ".index"), dtype="<u8")
    ix, _ = _recover(comp, stream, len(data), "raw")
    assert np.array_equal(ix, want)
    assert starflate_amd.decompress(stream, len(data)) == data


def _never_wrong(comp, stream, n, container="raw"):
    try:
        out, st = comp.decompress_any(stream, n, container)
    except StarflateError as e:
        assert e.code == NOT_INDEXABLE
        return "not-indexable"
    if st == OK:
        d = zlib.decompressobj(WBITS[container])
        try:
            want = d.decompress(stream)[:n]
        except zlib.error:
            want = None
        assert out == want, "Success with bytes zlib does not give"
        return "ok"
    return "status"


def test_unflushed_not_indexable(comp):
    data = _data("text", 4 * SEG + 5, 2).tobytes()
    for container, wbits in WBITS.items():
        c = zlib.compressobj(6, zlib.DEFLATED, wbits)
        stream = c.compress(data) + c.flush()
        with pytest.raises(StarflateError) as e:
            comp.decompress_any(stream, len(data), container)
        assert e.value.code == NOT_INDEXABLE


def test_damage_never_wrong_bytes(comp):
    rng = np.random.default_rng(2024)
    data = _data("mixed", 6 * SEG + 99, 4)
    seen = {}
    sources = [comp.compress(data, block_bytes=64 << 10), comp.compress(data, container="zlib"),
               W.zlib_flushed(data.tobytes(), 6, zlib.Z_SYNC_FLUSH, -15, True)]
    for case in range(200):
        src = sources[case % 3]
        container = "zlib" if case % 3 == 1 else "raw"
        b = bytearray(src)
        kind = case % 5
        if kind == 0:  # bit flips
            for _ in range(1 + case % 3):
                p = int(rng.integers(0, len(b)))
                b[p] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:  # byte edits
            p = int(rng.integers(0, len(b)))
            b[p] = int(rng.integers(0, 256))
        elif kind == 2:  # plant a marker
            p = int(rng.integers(4, len(b) - 8))
            b[p:p + 4] = b"\x00\x00\xff\xff"
        elif kind == 3:  # remove one
            hits = [i for i in range(len(b) - 4) if b[i:i + 4] == b"\x00\x00\xff\xff"]
            if hits:
                p = hits[int(rng.integers(0, len(hits)))]
                b[p + 3] ^= 0x10
        else:  # truncation
            b = b[:int(rng.integers(1, len(b)))]
        r = _never_wrong(comp, bytes(b), data.size, container)
        seen[r] = seen.get(r, 0) + 1
    assert sum(seen.values()) == 200


@pytest.mark.parametrize("flags", [0x08, 0x04 | 0x08 | 0x10, 0x02 | 0x10])
def test_gzip_header_fields_isize(comp, flags):
    data = _data("text", 5 * SEG + 17, 9).tobytes()
    body = W.zlib_flushed(data, 6, zlib.Z_FULL_FLUSH, -15, True)
    hdr = bytearray(b"\x1f\x8b\x08" + bytes([flags]) + b"\x00\x00\x00\x00\x00\xff")
    if flags & 0x04:
        hdr += struct.pack("<H", 6) + b"xtra!!"
    if flags & 0x08:
        hdr += b"name.txt\x00"
    if flags & 0x10:
        hdr += b"a comment\x00"
    if flags & 0x02:
        hdr += struct.pack("<H", zlib.crc32(bytes(hdr)) & 0xFFFF)
    stream = bytes(hdr) + body + struct.pack("<II", zlib.crc32(data), len(data))
    assert gzip.decompress(stream) == data
    out, st = comp.decompress_any(stream, None, "gzip")
    assert st == OK and out == data
    t = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
    o, st = comp.decompress_any_tensor(t, None, "gzip")
    assert st == OK and o.cpu().numpy().tobytes() == data
    bad = stream[:-8] + struct.pack("<II", zlib.crc32(data) ^ 1, len(data))
    assert comp.decompress_any(bad, None, "gzip")[1] == ERROR


def test_zlib_bad_adler(comp):
    data = _data("text", 3 * SEG + 5, 1)
    stream = comp.compress(data, container="zlib")
    bad = stream[:-1] + bytes([stream[-1] ^ 0x40])
    assert comp.decompress_any(bad, data.size, "zlib")[1] == ERROR
    assert comp.decompress_any(stream, data.size, "zlib") == (data.tobytes(), OK)


def test_cpp_fallback(tmp_path, comp):
    """compressor::decompress(src, dst, Container) returns container.hpp's status (and bytes) on intact, unflushed and
    damaged streams; compressor::recover_index gives the writer's index."""
    import subprocess

    from conftest import ROOT
    from starflate_amd import build

    rng = np.random.default_rng(77)
    data = _data("mixed", 5 * SEG + 1234, 8)
    lines = []

    def case(name, stream, kind, n, ix=None):
        (tmp_path / name).write_bytes(stream)
        if ix is not None:
            np.asarray(ix, dtype="<u8").tofile(str(tmp_path / (name + ".ix")))
        lines.append(f"{name} {kind} {n} {name + '.ix' if ix is not None else '-'}")

    for kind, cont in enumerate(("raw", "zlib", "gzip")):
        s = comp.compress(data, container=cont, block_bytes=64 << 10)
        case(f"lib{kind}", s, kind, data.size, comp.last_index())
        c = zlib.compressobj(6, zlib.DEFLATED, WBITS[cont])
        case(f"unflushed{kind}", c.compress(data.tobytes()) + c.flush(), kind, data.size)
        case(f"flushed{kind}", W.zlib_flushed(data.tobytes(), 6, zlib.Z_SYNC_FLUSH, WBITS[cont]), kind, data.size)
        for j in range(10):
            b = bytearray(s)
            p = int(rng.integers(0, len(b)))
            if j % 2:
                b[p] ^= 1 << int(rng.integers(0, 8))
            else:
                b[p:p + 4] = b"\x00\x00\xff\xff"
            case(f"damaged{kind}_{j}", bytes(b), kind, data.size)
        case(f"truncated{kind}", s[: len(s) // 2], kind, data.size)
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    lib = build.build()
    exe = tmp_path / "decompress_any"
    clang = "/opt/rocm/llvm/bin/clang++"
    subprocess.check_call([clang, "-O2", "-std=c++23", "-fno-exceptions", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "decompress_any.cpp"),
                           "-L" + os.path.dirname(lib), "-lstarflate_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", str(exe)])
    out = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failed" in out.stdout
