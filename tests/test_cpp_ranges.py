"""Compiles and runs the C++23 random-access test (tests/cpp/decompress_ranges.cpp: compressor::decompress_range and
compressor::decompress_ranges) with AMD clang -std=c++23, as tests/test_cpp_host_api.py runs its programs."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
FLAGS = ["-std=c++23", "-fno-exceptions", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror",
         "-I" + os.path.join(ROOT, "include")]


@pytest.mark.gpu
def test_decompress_ranges_cpp(tmp_path):
    from starflate_amd import build

    lib = build.build()
    exe = tmp_path / "decompress_ranges"
    libdir = os.path.dirname(lib)
    subprocess.check_call([CLANG, "-O2"] + FLAGS + [os.path.join(ROOT, "tests", "cpp", "decompress_ranges.cpp"),
                                                   "-L" + libdir, "-lstarflate_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = subprocess.run([str(exe), GOLDEN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
