"""Batched compression (sfh_compress_batch / sfh_compress_batch_device_async): every item's stream is byte-identical to the
single call's on that item with the same options, and to the encoder specification's (the oracle); every stream decodes
with zlib and with the oracle's decoder."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import oracle_lib as O
from conftest import GOLDEN, ROOT
from starflate_amd import Compressor, _capi, synth

pytestmark = pytest.mark.gpu

CHUNK = 32768
# effort -> the specification's parameters for it
EFFORTS = {"default": {}, "fast": dict(depth=1), "fastest": dict(depth=1, use_near=0), "thorough": dict(stride2=0, step=512),
           "max": dict(stride2=0, step=512, hash_bits=12, long_hash_bytes=7), "chain4": dict(chain_depth=4),
           "recent_all": dict(recent=1, near_depth=1, link_steps=1, stride2=0, step=512)}


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


def _content(kind, n, seed):
    if kind == "text":
        return synth.gen_text(n, seed=seed)
    if kind == "noise":
        return synth.gen_random(n, seed=seed)
    if kind == "six":  # six bits of entropy per byte
        return (np.random.default_rng(seed).integers(0, 64, n, dtype=np.uint8) + 32).astype(np.uint8)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    return synth.gen_mixed(n, seed=seed)


KINDS = ("text", "noise", "six", "zeros", "mixed")
SIZES = (0, 1, 31, 32767, 32768, 32769, 100 << 10, (1 << 20) + 17, 5 << 20)


def _items(sizes, seed=0):
    return [_content(KINDS[(i + seed) % len(KINDS)], n, seed * 100 + i) for i, n in enumerate(sizes)]


def _oracle_params(strategy="auto", final_stream=True, lazy=3, stored_fast_path=True, block_bytes=0, effort="default"):
    return O.default_params(strategy=_capi.STRATEGY[strategy], final_stream=int(final_stream), lazy=3 if lazy is True else int(lazy),
                            fast_skip=int(stored_fast_path), strip_bytes=block_bytes, **EFFORTS[effort])


def _unwrap(stream, container):
    hdr, tr = {"raw": (0, 0), "zlib": (2, 4), "gzip": (10, 8)}[container]
    return stream[hdr: len(stream) - tr]


def _check(comp, items, streams, oracle=True, **opt):
    """each batch stream == the single call's == the oracle's (raw body); it decodes with zlib and the oracle's decoder"""
    container = opt.get("container", "raw")
    for i, (data, got) in enumerate(zip(items, streams)):
        got = bytes(got)
        single = comp.compress(data, **opt)
        assert got == single, (i, data.size, opt)
        body = np.frombuffer(_unwrap(got, container), np.uint8)
        if oracle:
            oo = {k: v for k, v in opt.items() if k != "container"}
            want = O.compress(data, _oracle_params(**oo))
            assert np.array_equal(body, want), (i, data.size, opt)
        if opt.get("final_stream", True):
            wbits = {"raw": -15, "zlib": 15, "gzip": 31}[container]
            assert zlib.decompress(got, wbits) == data.tobytes(), (i, data.size)
        else:  # non-final: a final empty block closes it for the decoder
            body = np.concatenate([body, np.array([3, 0], np.uint8)])
        st, w, back = O.decompress(body, data.size)
        assert st == 0 and w == data.size and np.array_equal(back, data), (i, data.size, st)


def _device_batch(comp, items, stream=None, **opt):
    import torch

    srcs = [torch.from_numpy(d).cuda() if d.size else torch.empty(0, dtype=torch.uint8, device="cuda") for d in items]
    outs, sizes = comp.compress_batch_tensors(srcs, stream=stream, **opt)
    torch.cuda.synchronize()
    sz = sizes.cpu().tolist()
    return [o[:n].cpu().numpy().tobytes() for o, n in zip(outs, sz)]


def test_mixed_sizes_host_and_device(comp):
    items = _items(SIZES)
    _check(comp, items, comp.compress_batch(items))
    _check(comp, items, _device_batch(comp, items), oracle=False)


@pytest.mark.parametrize("effort", list(EFFORTS))
def test_every_effort(comp, effort):
    items = _items((0, 1, 31, 32769, 100 << 10, 300 << 10), seed=3)
    _check(comp, items, comp.compress_batch(items, effort=effort), effort=effort)


def test_strategies_lazy_fast_path_block_bytes(comp):
    items = _items((1, 32767, 32769, 100 << 10, (1 << 20) + 17, 5 << 20), seed=5)
    combos = []
    for k, strategy in enumerate(("auto", "stored", "fixed", "dynamic")):
        for j, bb in enumerate((0, 32768, 262144, 1 << 20)):
            combos.append(dict(strategy=strategy, lazy=(0, 3)[(k + j) % 2], stored_fast_path=bool((k + j // 2) % 2), block_bytes=bb))
    for opt in combos:
        _check(comp, items, comp.compress_batch(items, **opt), **opt)


@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_containers(comp, container):
    items = _items((0, 1, 32768, 32769, 100 << 10, (1 << 20) + 17), seed=7)
    streams = comp.compress_batch(items, container=container)
    _check(comp, items, streams, container=container)
    _check(comp, items, _device_batch(comp, items, container=container), oracle=False, container=container)
    for data, s in zip(items, streams):  # the trailer's checksum is the item's own
        if container == "zlib":
            assert int.from_bytes(s[-4:], "big") == zlib.adler32(data.tobytes())
        else:
            assert int.from_bytes(s[-8:-4], "little") == zlib.crc32(data.tobytes()) and int.from_bytes(s[-4:], "little") == data.size


def test_non_final_streams(comp):
    items = _items((0, 1, 32769, 100 << 10), seed=9)
    streams = comp.compress_batch(items, final_stream=False)
    _check(comp, items, streams, final_stream=False)
    for data, s in zip(items, streams):  # non-final: a final empty stored block closes it for zlib
        assert zlib.decompress(s + b"\x03\x00", -15) == data.tobytes()


@pytest.mark.parametrize("bb", [0, 262144])
def test_launch_batches(monkeypatch, bb):
    """SFH_BATCH_CHUNKS=4: items straddle the cut, one item spans several launch batches (with bb = 256 KiB its strips
    are wider than a launch batch), and one call runs many launch batches."""
    monkeypatch.setenv("SFH_BATCH_CHUNKS", "4")
    c = Compressor(0)
    monkeypatch.delenv("SFH_BATCH_CHUNKS")
    try:
        sizes = (3 * CHUNK + 5, 2 * CHUNK, 1, 0, 20 * CHUNK + 999, CHUNK, 5 * CHUNK, 7, 4 * CHUNK, 3 * CHUNK - 1)
        items = _items(sizes, seed=11)
        for container in ("raw", "gzip"):
            _check(c, items, c.compress_batch(items, block_bytes=bb, container=container), block_bytes=bb, container=container)
            _check(c, items, _device_batch(c, items, block_bytes=bb, container=container), oracle=False, block_bytes=bb,
                   container=container)
    finally:
        c.close()


def test_many_tiny_items(comp):
    rng = np.random.default_rng(13)
    text = synth.gen_text(1 << 22, seed=13)
    sizes = rng.integers(0, 4097, 10_000)
    starts = rng.integers(0, text.size - 4096, 10_000)
    items = [text[s: s + n].copy() if i % 5 else _content("six", int(n), i) for i, (s, n) in enumerate(zip(starts, sizes))]
    streams = comp.compress_batch(items)
    assert len(streams) == len(items)
    p = _oracle_params()
    for i, (data, s) in enumerate(zip(items, streams)):
        assert np.array_equal(np.frombuffer(s, np.uint8), O.compress(data, p)), i
    for i in range(0, len(items), 97):
        assert zlib.decompress(streams[i], -15) == items[i].tobytes()


def test_async_back_to_back_on_a_caller_stream(comp):
    """two async calls in a row whose descriptor tables differ: the second's must not overwrite the first's before they
    were uploaded; sizes come from the device tensor"""
    import torch

    a = _items((1, 32769, 100 << 10, 3 << 20), seed=15)
    b = _items((200 << 10, 0, 31, 32768, 77, 600 << 10, 5), seed=16)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ta = [torch.from_numpy(d).cuda() if d.size else torch.empty(0, dtype=torch.uint8, device="cuda") for d in a]
        tb = [torch.from_numpy(d).cuda() if d.size else torch.empty(0, dtype=torch.uint8, device="cuda") for d in b]
        oa, sa = comp.compress_batch_tensors(ta, stream=s.cuda_stream, container="zlib")
        ob, sb = comp.compress_batch_tensors(tb, stream=s.cuda_stream)
    s.synchronize()
    assert sa.dtype == torch.int64 and sa.is_cuda
    got_a = [o[:n].cpu().numpy().tobytes() for o, n in zip(oa, sa.cpu().tolist())]
    got_b = [o[:n].cpu().numpy().tobytes() for o, n in zip(ob, sb.cpu().tolist())]
    _check(comp, a, got_a, oracle=False, container="zlib")
    _check(comp, b, got_b)


def test_single_batch_single_and_index_state(comp):
    data = synth.gen_text(5 * CHUNK + 1234, seed=2)
    fresh = Compressor(0)
    try:
        want = fresh.compress(data, block_bytes=65536)
        want_idx = fresh.last_index()
        assert comp.compress(data, block_bytes=65536) == want and np.array_equal(comp.last_index(), want_idx)
        items = _items((1, 100 << 10, 32769), seed=17)
        streams = comp.compress_batch(items)
        L, h = comp._lib, comp._h
        assert L.sfh_index_entries(h) == 0 and L.sfh_last_block_bytes(h) == 0
        idx = np.zeros(7, np.uint64)
        assert L.sfh_copy_index(h, idx.ctypes.data, 7, 0, None) == -1
        sub = np.zeros(6 * 64, np.uint32)
        assert L.sfh_copy_subindex(h, sub.ctypes.data, 6 * 64, 0, None) == -1
        with pytest.raises(Exception):
            comp.last_index()
        comp.set_profiling(True)
        comp.compress_batch(items)
        ms = comp.stage_ms()
        comp.set_profiling(False)
        assert ms["k_lz77"] > 0 and ms["k_emit"] > 0
        _check(comp, items, streams, oracle=False)  # (single calls on the items: the index is theirs again)
        assert comp.compress(data, block_bytes=65536) == want and np.array_equal(comp.last_index(), want_idx)
        assert comp.last_block_bytes() == 65536
    finally:
        fresh.close()


def test_refusals_write_nothing(comp):
    import torch

    L, h = comp._lib, comp._h
    srcs = [torch.from_numpy(synth.gen_text(n, seed=n)).cuda() for n in (1000, 40000, 5)]
    caps = [comp.compress_bound(t.numel()) for t in srcs]
    arena = torch.full((sum(caps) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    sizes = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def call(src_ptrs, dst_ptrs, capv, opt=None):
        k = len(src_ptrs)
        o = opt or _capi.make_options()
        return L.sfh_compress_batch_device_async(h, k, (C.c_void_p * k)(*src_ptrs), (C.c_uint64 * k)(*[t.numel() for t in srcs]),
                                                 (C.c_void_p * k)(*dst_ptrs), (C.c_uint64 * k)(*capv),
                                                 C.c_void_p(sizes.data_ptr()), C.byref(o), None)

    base = arena.data_ptr()
    sp = [t.data_ptr() for t in srcs]
    dp = [base, base + caps[0], base + caps[0] + caps[1]]
    assert call(sp, dp, [caps[0], caps[1] - 1, caps[2]]) == -2           # one destination below the bound
    assert call([sp[0], sp[1] + 1, sp[2]], dp, caps) == -1                 # a misaligned source
    assert call(sp, [dp[0], dp[1] + 2, dp[2] + 4], caps) == -1             # a misaligned destination
    assert call(sp, [dp[0], dp[0] + caps[0] - 4, dp[2]], caps) == -1       # overlapping destinations
    assert call(sp, dp, caps, _capi.make_options(container="gzip", final_stream=False)) == -1  # a container needs a final stream
    assert L.sfh_compress_batch_device_async(h, 3, None, None, None, None, None, None, None) == -1
    assert L.sfh_compress_batch_device_async(h, 0, None, None, None, None, None, None, None) == 0  # nothing to do
    torch.cuda.synchronize()
    assert bool((arena == 0xA5).all()) and bool((sizes == -1).all())
    # the host-buffer entry point refuses alike
    with pytest.raises(Exception):
        comp.compress_batch([b"abc", b"d"], container="zlib", final_stream=False)
    assert comp.compress_batch([]) == []


def test_cpp_compress_batch(tmp_path):
    from starflate_amd import build

    lib = build.build()
    exe = tmp_path / "compress_batch"
    libdir = os.path.dirname(lib)
    clang = "/opt/rocm/llvm/bin/clang++"
    flags = ["-std=c++23", "-fno-exceptions", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror", "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call([clang, "-O2"] + flags + [os.path.join(ROOT, "tests", "cpp", "compress_batch.cpp"), "-L" + libdir,
                                                   "-lstarflate_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = subprocess.run([str(exe), GOLDEN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
