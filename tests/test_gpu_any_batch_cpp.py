"""compressor::decompress_batch(srcs, dsts, Container, statuses) (include/starflate/compress.hpp): one GPU call over streams
given alone, the serial decoder behind every item the GPU did not decode -- intact, unflushed, damaged and truncated items in
one batch per container, each with the status and bytes of container.hpp's decompress(); compressor::recover_index_batch
gives the writer's indexes (tests/cpp/decompress_any_batch.cpp)."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import unindexed_walk as W
from conftest import ROOT
from starflate_amd import Compressor, build, synth

pytestmark = pytest.mark.gpu

SEG = 32768
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}
CLANG = "/opt/rocm/llvm/bin/clang++"


def test_cpp_decompress_batch(tmp_path):
    rng = np.random.default_rng(78)
    datas = [synth.gen_mixed(5 * SEG + 1234, seed=8, stripe=3 * SEG + 1000), synth.gen_text(SEG - 5, seed=2), np.zeros(0, np.uint8)]
    lines = []

    def case(name, stream, kind, n, ix=None):
        (tmp_path / name).write_bytes(stream)
        if ix is not None:
            np.asarray(ix, dtype="<u8").tofile(str(tmp_path / (name + ".ix")))
        lines.append(f"{name} {kind} {n} {name + '.ix' if ix is not None else '-'}")

    comp = Compressor(0)
    try:
        for kind, cont in enumerate(("raw", "zlib", "gzip")):
            streams = comp.compress_batch(datas, container=cont, block_bytes=64 << 10)
            flat, _, _ = comp.last_batch_index()
            at = 0
            for j, (d, s) in enumerate(zip(datas, streams)):
                n = max(1, -(-d.size // SEG)) + 1
                case(f"lib{kind}_{j}", s, kind, d.size, flat[at:at + n])
                at += n
            big, s = datas[0], streams[0]
            c = zlib.compressobj(6, zlib.DEFLATED, WBITS[cont])
            case(f"unflushed{kind}", c.compress(big.tobytes()) + c.flush(), kind, big.size)
            case(f"flushed{kind}", W.zlib_flushed(big.tobytes(), 6, zlib.Z_SYNC_FLUSH, WBITS[cont]), kind, big.size)
            for j in range(6):
                b = bytearray(s)
                p = int(rng.integers(0, len(b)))
                if j % 2:
                    b[p] ^= 1 << int(rng.integers(0, 8))
                else:
                    b[p:p + 4] = b"\x00\x00\xff\xff"
                case(f"damaged{kind}_{j}", bytes(b), kind, big.size)
            case(f"truncated{kind}", s[: len(s) // 2], kind, big.size)
            case(f"again{kind}", s, kind, big.size, flat[:max(1, -(-big.size // SEG)) + 1])
    finally:
        comp.close()
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    lib = build.build()
    exe = tmp_path / "decompress_any_batch"
    subprocess.check_call([CLANG, "-O2", "-std=c++23", "-fno-exceptions", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "decompress_any_batch.cpp"),
                           "-L" + os.path.dirname(lib), "-lstarflate_hip", "-Wl,-rpath," + os.path.dirname(lib), "-o", str(exe)])
    out = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failed" in out.stdout
    assert "12 indexes recovered" in out.stdout  # (4 per container)
    assert " 0 not indexable" not in out.stdout  # the unflushed items took the serial decoder
