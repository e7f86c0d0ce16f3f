"""The index-free batch decoder's cut into launch batches (starflate_amd/csrc/sf_any_plan.h: whole items, at most `cap`
segments per batch, a larger item alone) as a stand-alone host program (tests/cpp/any_plan_host.cpp), compiled with every
warning an error and run plain and under AddressSanitizer + UBSan: an item exactly at the cap, one a segment over it, empty
items, a cap of 1, items that take no part, and random calls against the rule's properties."""
import os
import subprocess

import pytest

from conftest import ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_any_plan_host(tmp_path, san):
    exe = tmp_path / "any_plan_host"
    subprocess.check_call([CLANG, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror"] + san +
                          [os.path.join(ROOT, "tests", "cpp", "any_plan_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failed" in out.stdout
