"""Compiles and runs the C++23 seekable-gzip test (tests/cpp/dictzip_roundtrip.cpp: Container::Dictzip, starflate::dz_read_index,
compressor::decompress_dz and decompress_dz_range) with AMD clang -std=c++23, as tests/test_cpp_ranges.py runs its program."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
FLAGS = ["-std=c++23", "-fno-exceptions", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror",
         "-I" + os.path.join(ROOT, "include")]


@pytest.mark.gpu
def test_dictzip_cpp(tmp_path):
    from starflate_amd import build

    lib = build.build()
    exe = tmp_path / "dictzip_roundtrip"
    libdir = os.path.dirname(lib)
    subprocess.check_call([CLANG, "-O2"] + FLAGS + [os.path.join(ROOT, "tests", "cpp", "dictzip_roundtrip.cpp"),
                                                   "-L" + libdir, "-lstarflate_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = subprocess.run([str(exe), GOLDEN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
