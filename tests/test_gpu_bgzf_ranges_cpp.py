"""Compiles and runs the C++23 BGZF random-access test (tests/cpp/bgzf_ranges.cpp: compressor::decompress_bgzf_range and
decompress_bgzf_ranges, starflate::bgzf_voffsets_to_offsets and bgzf_offsets_to_voffsets) with AMD clang -std=c++23, as
tests/test_gpu_bgzf_cpp.py runs its program.  The file of 65280-byte members is written here with Python's zlib."""
import os
import subprocess

import pytest

import bgzf_files as BZ
from conftest import GOLDEN, ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
FLAGS = ["-std=c++23", "-fno-exceptions", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror",
         "-I" + os.path.join(ROOT, "include")]


@pytest.mark.gpu
def test_bgzf_ranges_cpp(tmp_path):
    from starflate_amd import build

    lib = build.build()
    exe = tmp_path / "bgzf_ranges"
    libdir = os.path.dirname(lib)
    subprocess.check_call([CLANG, "-O2"] + FLAGS + [os.path.join(ROOT, "tests", "cpp", "bgzf_ranges.cpp"),
                                                   "-L" + libdir, "-lstarflate_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
    data = BZ.text(3 * 65280, seed=2)
    blob = BZ.write(data, [65280] * 3)[0]
    (tmp_path / "wide.gz").write_bytes(blob)
    (tmp_path / "wide.bin").write_bytes(data)
    out = subprocess.run([str(exe), GOLDEN, str(tmp_path / "wide.gz"), str(tmp_path / "wide.bin")], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
