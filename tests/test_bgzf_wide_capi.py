"""CPU-side checks of sfh_decompress_bgzf_wide_device: exported, declared, listed and bound in Python; refusals before any
device is touched."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import starflate_amd
from conftest import ROOT
from starflate_amd import _capi


def test_symbol_exported_declared_listed():
    lib = _capi.lib()
    name = "sfh_decompress_bgzf_wide_device"
    assert hasattr(lib, name) and name in _capi.EXPORTS
    with open(os.path.join(ROOT, "include", "starflate_hip.h")) as f:
        header = f.read()
    decl = re.search(r"int sfh_decompress_bgzf_wide_device\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    narrow = re.search(r"int sfh_decompress_bgzf_device\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert decl and narrow and " ".join(decl.group(1).split()) == " ".join(narrow.group(1).split())  # the same arguments
    assert lib.sfh_decompress_bgzf_wide_device.argtypes == lib.sfh_decompress_bgzf_device.argtypes
    assert "decompress_bgzf_wide_tensor" in dir(starflate_amd.Compressor)
    sig = inspect.signature(starflate_amd.Compressor.decompress_bgzf_wide_tensor)
    assert list(sig.parameters) == ["self", "src", "total_n", "out", "stream"]
    assert sig == inspect.signature(starflate_amd.Compressor.decompress_bgzf_tensor)
    with open(os.path.join(ROOT, "starflate_amd", "csrc", "sf_device.h")) as f:
        assert "constexpr uint32_t kWideRow = 65536;" in f.read()


def test_null_context_and_null_arguments_are_refused():
    lib = _capi.lib()
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    n64, st = C.c_uint64(7), C.c_uint32(7)
    assert lib.sfh_decompress_bgzf_wide_device(None, p, 64, p + 128, 64, C.byref(n64), C.byref(st), None) == -1
    assert lib.sfh_decompress_bgzf_wide_device(None, None, 0, None, 0, C.byref(n64), C.byref(st), None) == -1
    assert lib.sfh_decompress_bgzf_wide_device(None, p, 64, p + 128, 64, None, None, None) == -1
    assert (n64.value, st.value) == (7, 7) and not buf.any()
