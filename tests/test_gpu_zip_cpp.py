"""Compiles and runs the C++23 ZIP test (tests/cpp/zip_roundtrip.cpp: compressor::compress_zip and decompress_zip,
starflate::zip_bound and zip_read_index) with AMD clang -std=c++23, as tests/test_gpu_bgzf_cpp.py runs its program; the test
writes one archive with zipfile, and every entry's bytes beside it, for the program to read."""
import os
import subprocess
import zipfile

import pytest

import zip_files as Z
from conftest import GOLDEN, ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
FLAGS = ["-std=c++23", "-fno-exceptions", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror",
         "-I" + os.path.join(ROOT, "include")]


@pytest.mark.gpu
def test_zip_cpp(tmp_path):
    from starflate_amd import build

    lib = build.build()
    exe = tmp_path / "zip_roundtrip"
    libdir = os.path.dirname(lib)
    subprocess.check_call([CLANG, "-O2"] + FLAGS + [os.path.join(ROOT, "tests", "cpp", "zip_roundtrip.cpp"),
                                                   "-L" + libdir, "-lstarflate_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
    foreign = tmp_path / "foreign.zip"
    datas = [Z.text(100000, 1), Z.text(5000, 2), b"", Z.text(40000, 3)]
    with zipfile.ZipFile(foreign, "w") as z:
        z.writestr("deflated6.txt", datas[0], compress_type=zipfile.ZIP_DEFLATED, compresslevel=6)
        z.writestr("stored.bin", datas[1], compress_type=zipfile.ZIP_STORED)
        z.writestr("empty", datas[2], compress_type=zipfile.ZIP_STORED)
        z.writestr("deflated1.txt", datas[3], compress_type=zipfile.ZIP_DEFLATED, compresslevel=1)
    for i, d in enumerate(datas):
        with open(f"{foreign}.{i}", "wb") as f:
            f.write(d)
    out = subprocess.run([str(exe), GOLDEN, str(foreign)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
