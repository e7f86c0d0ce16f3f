"""Compiles and runs the C++23 BGZF test (tests/cpp/bgzf_roundtrip.cpp: compressor::compress_bgzf and decompress_bgzf,
starflate::bgzf_bound and bgzf_read_index) with AMD clang -std=c++23, as tests/test_gpu_dictzip_cpp.py runs its program."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
FLAGS = ["-std=c++23", "-fno-exceptions", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror",
         "-I" + os.path.join(ROOT, "include")]


@pytest.mark.gpu
def test_bgzf_cpp(tmp_path):
    from starflate_amd import build

    lib = build.build()
    exe = tmp_path / "bgzf_roundtrip"
    libdir = os.path.dirname(lib)
    subprocess.check_call([CLANG, "-O2"] + FLAGS + [os.path.join(ROOT, "tests", "cpp", "bgzf_roundtrip.cpp"),
                                                   "-L" + libdir, "-lstarflate_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
    out = subprocess.run([str(exe), GOLDEN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
