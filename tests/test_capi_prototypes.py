"""The Python binding against its parent commit and against the header, without a device:
- tests/golden/capi_prototypes_parent.json: restype and argtypes of every sfh_* function as the parent's _capi.lib() set them
  (tests and tools call comp._lib.sfh_* with ints, ctypes arrays and byrefs that rely on them), and every argtypes list against
  the parameter count include/starflate_hip.h declares;
- tests/golden/python_api_parent.json: signature and docstring of every public function of the package and of every public
  method of Compressor;
- the marshalling helpers of starflate_amd/compressor.py at their seams.
Both files are written once, from the parent, by `python tests/test_capi_prototypes.py`."""
import ctypes as C
import hashlib
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import starflate_amd
from starflate_amd import _capi, compressor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _header():
    with open(os.path.join(ROOT, "include", "starflate_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)  # (the comment stripper of test_capi_symbols.py)


def _declared_params():
    """{symbol: parameter count} of every sfh_* declaration in the header"""
    out = {}
    for name, params in re.findall(r"\b(sfh_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header()):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def _type_name(t):
    return "None" if t is None else t.__name__


def prototype_snapshot():
    lib = _capi.lib()
    return {name: {"restype": _type_name(getattr(lib, name).restype), "argtypes": [_type_name(t) for t in getattr(lib, name).argtypes]}
            for name in sorted(_declared_params())}


def _entry(f):
    return {"signature": str(inspect.signature(f)), "doc_sha256": hashlib.sha256((f.__doc__ or "").encode()).hexdigest()}


def api_snapshot():
    funcs = {n: _entry(getattr(starflate_amd, n)) for n in starflate_amd.__all__ if inspect.isfunction(getattr(starflate_amd, n))}
    methods = {n: _entry(getattr(starflate_amd.Compressor, n)) for n, v in vars(starflate_amd.Compressor).items()
               if (not n.startswith("_") or n == "__init__") and callable(getattr(starflate_amd.Compressor, n))}
    return {"__all__": sorted(starflate_amd.__all__), "functions": funcs, "Compressor": methods}


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_prototypes_are_the_parents():
    want, got = _golden("capi_prototypes_parent.json"), prototype_snapshot()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    # ... and they are what lib() applied from the one table, which names every symbol once
    assert sorted(_capi.PROTOTYPES) == sorted(want) and _capi.EXPORTS == list(_capi.PROTOTYPES)
    lib = _capi.lib()
    for name, (restype, argtypes) in _capi.PROTOTYPES.items():
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == list(argtypes), name


def test_argtypes_count_the_headers_parameters():
    declared = _declared_params()
    assert len(declared) > 80 and declared["sfh_device_count"] == 0 and declared["sfh_decompress_ranges_device_async"] == 14
    lib = _capi.lib()
    wrong = {n: (len(getattr(lib, n).argtypes), k) for n, k in declared.items() if len(getattr(lib, n).argtypes) != k}
    assert not wrong, wrong


def test_array_lengths_are_the_headers():
    defines = {k: int(v) for k, v in re.findall(r"#define\s+SFH_(\w*N(?:STAGES|COUNTS))\s+(\d+)", _header())}
    assert defines == {"STREAM_NSTAGES": _capi.STREAM_NSTAGES, "STREAM_NCOUNTS": _capi.STREAM_NCOUNTS, "NSTAGES": _capi.NSTAGES,
                       "INFLATE_NSTAGES": _capi.INFLATE_NSTAGES}, defines


def test_python_api_is_the_parents():
    want, got = _golden("python_api_parent.json"), api_snapshot()
    assert got["__all__"] == want["__all__"]
    for group in ("functions", "Compressor"):
        assert sorted(got[group]) == sorted(want[group]), group
        for name in want[group]:
            assert got[group][name] == want[group][name], (group, name)


def _parent_bytes(data):
    """the expression the parent's entry points spelled inline"""
    return np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).ravel()


@pytest.mark.parametrize("data", [
    b"starflate", bytearray(b"starflate"), memoryview(b"starflate"), b"",
    np.arange(40, dtype=np.uint8), np.arange(40, dtype=np.uint8)[3::2], np.arange(40, dtype=np.uint8).reshape(5, 8),
    np.arange(40, dtype=np.uint8).reshape(5, 8)[:, 1:4], np.array([1, 2, 255, 0], dtype=np.int32), np.zeros(0, dtype=np.uint8),
], ids=["bytes", "bytearray", "memoryview", "empty", "uint8", "strided", "2d", "2d-strided", "int32", "empty-array"])
def test_as_bytes(data):
    a = compressor._as_bytes(data)
    assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 1 and a.flags["C_CONTIGUOUS"]
    assert np.array_equal(a, _parent_bytes(data))
    assert a.tobytes() == (bytes(data) if not isinstance(data, np.ndarray) else np.asarray(data).astype(np.uint8).tobytes())


def test_pointer_helpers():
    full, empty = np.arange(4, dtype=np.uint8), np.zeros(0, dtype=np.uint8)
    assert compressor._ptr(full) == full.ctypes.data and compressor._ptr(empty) is None
    p = compressor._ptrs([full, empty, full[1:]])
    assert isinstance(p, C.c_void_p * 3) and list(p) == [full.ctypes.data, None, full.ctypes.data + 1]
    assert len(compressor._ptrs([])) == 0 and isinstance(compressor._ptrs([]), C.c_void_p * 0)
    assert compressor._ptr(None) is None and list(compressor._ptrs([None, full])) == [None, full.ctypes.data]
    assert compressor._addr(None) is None and compressor._addr(empty) == empty.ctypes.data and compressor._addr(full) == full.ctypes.data
    # tensors: an empty one's data_ptr() is 0, a view of no elements included, and a void* of 0 is null
    import torch

    t = torch.arange(8, dtype=torch.uint8)
    assert torch.empty(0, dtype=torch.uint8).data_ptr() == 0 and t[3:3].data_ptr() == 0 and t[3:].data_ptr() == t.data_ptr() + 3
    d = compressor._dptrs([t, t[3:3], None, t[3:]])
    assert isinstance(d, C.c_void_p * 4) and list(d) == [t.data_ptr(), None, None, t.data_ptr() + 3]
    assert isinstance(compressor._dptrs([]), C.c_void_p * 0)
    u = compressor._u64s([])
    assert isinstance(u, C.c_uint64 * 0) and len(u) == 0
    u = compressor._u64s([0, 5, (1 << 64) - 1])
    assert isinstance(u, C.c_uint64 * 3) and list(u) == [0, 5, (1 << 64) - 1]
    assert list(compressor._u64s(a.size for a in (full, empty))) == [4, 0]


@pytest.mark.parametrize("call, what", [
    # (decompress_batch, decompress_range(s) and read_ranges have their texts in test_batch_inflate_capi.py, test_range_capi.py
    #  and test_dictzip_capi.py; the two calls below are there without them)
    (lambda: starflate_amd.decompress_stream_batch([b"a", b"b"], [1, 2, 3]), "2 streams but 3 sizes"),
    (lambda: starflate_amd.decompress_stream_batch(b"ab"), "a sequence of bytes-like streams"),
    (lambda: starflate_amd.decompress_stream_batch([b"a"], [-1]), r"sizes must lie in \[0, 2\^44\]"),
    (lambda: starflate_amd.decompress_stream_batch([b"a"], container="lz4"), "container must be one of"),
    (lambda: starflate_amd.decompress_any_batch([b"a", b"b"], [1]), "2 streams but 1 sizes"),
    (lambda: starflate_amd.decompress_any_batch([b"a"]), "sizes is required unless container='gzip'"),
    (lambda: starflate_amd.decompress_any_batch([b"a"], [1 << 45]), r"sizes must lie in \[0, 2\^44\]"),
    (lambda: starflate_amd.decompress_batch([b"a"], [1, 2]), "1 streams but 2 sizes"),
    (lambda: starflate_amd.decompress_ranges(b"x", [0, 1], 1, [0], [1, 1], block_bytes=32768), "1 offsets but 2 lengths"),
    (lambda: starflate_amd.decompress_range(b"x", [0, 1], 1, 1, 1, block_bytes=32768), "does not lie inside"),
])
def test_module_level_checks_raise_without_a_device(monkeypatch, call, what):
    def no_context(*a, **k):
        raise AssertionError("a context was asked for before the arguments were checked")

    monkeypatch.setattr(compressor, "Compressor", no_context)
    monkeypatch.setattr(compressor, "_DEFAULT", {})
    with pytest.raises(ValueError, match=what):
        call()


def test_torch_stays_a_lazy_import():
    """A fresh interpreter: importing the package imports no torch, and a host-buffer call (which loads the library, torch
    first) leaves torch's GPU state untouched."""
    import subprocess

    code = ("import sys; sys.path.insert(0, sys.argv[1]); import starflate_amd; assert 'torch' not in sys.modules\n"
            "from starflate_amd import compressor\n"
            "assert compressor._as_bytes(b'ab').tolist() == [97, 98] and 'torch' not in sys.modules\n"
            "try:\n    starflate_amd.bgzf_index(b'')\nexcept starflate_amd.StarflateError:\n    pass\n"
            "assert starflate_amd.zip_bound([], []) == 98\n"
            "t = sys.modules.get('torch'); assert t is None or not t.cuda.is_initialized()\n")
    subprocess.run([sys.executable, "-c", code, ROOT], check=True, timeout=120)


if __name__ == "__main__":  # writes the two snapshots: run at the parent commit only
    for name, snap in (("capi_prototypes_parent.json", prototype_snapshot()), ("python_api_parent.json", api_snapshot())):
        with open(os.path.join(GOLDEN, name), "w") as f:
            json.dump(snap, f, indent=1, sort_keys=True)
            f.write("\n")
