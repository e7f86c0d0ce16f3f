"""Virtual offsets (sfh_bgzf_voffsets_to_offsets, sfh_bgzf_offsets_to_voffsets: host arithmetic, no device) against a
ten-line Python model, on the files of tests/bgzf_files.py."""
import ctypes as C

import numpy as np
import pytest

import bgzf_files as BZ
import starflate_amd as sa
from starflate_amd import _capi

NONE = (1 << 64) - 1


def model_to_offset(moff, ooff, v):
    c, u = v >> 16, v & 0xFFFF
    m = len(moff) - 1
    if c == moff[m]:
        return ooff[m] if u == 0 else NONE
    for i in range(m):
        if moff[i] == c:
            return ooff[i] + u if u <= ooff[i + 1] - ooff[i] else NONE
    return NONE


def model_to_voffset(moff, ooff, o):
    m = len(moff) - 1
    if o > ooff[m]:
        return NONE
    if o == ooff[m]:
        return moff[m] << 16
    i = min(i for i in range(m) if ooff[i + 1] > o)  # the member that holds byte o: never an empty one
    return moff[i] << 16 | (o - ooff[i])


@pytest.fixture(scope="module")
def files():
    return BZ.good_files()


def test_both_directions_against_the_model(files):
    for name, (data, blob, moff, ooff, _) in files.items():
        total = len(data)
        offs = sorted({o + d for o in ooff for d in (-1, 0, 1) if 0 <= o + d <= total + 1} | {total // 2})
        got_v = [int(v) for v in sa.bgzf_offsets_to_voffsets(moff, ooff, offs)]
        assert got_v == [model_to_voffset(moff, ooff, o) for o in offs], name
        vs = [v for v in got_v if v != NONE]
        vs += [m << 16 for m in moff] + [m << 16 | (b - a) for m, a, b in zip(moff, ooff, ooff[1:])]  # uoffset == out_n is valid
        assert [int(o) for o in sa.bgzf_voffsets_to_offsets(moff, ooff, vs)] == [model_to_offset(moff, ooff, v) for v in vs], name


def test_round_trip_over_every_offset(files):
    for name, (data, blob, moff, ooff, _) in files.items():
        if len(data) > 140000:  # (the small files; the 65280-byte members have their boundaries in the test above)
            continue
        offs = np.arange(len(data) + 1, dtype=np.uint64)
        back = sa.bgzf_voffsets_to_offsets(moff, ooff, sa.bgzf_offsets_to_voffsets(moff, ooff, offs))
        assert np.array_equal(back, offs), name


def test_a_voffset_never_names_an_empty_member_for_a_byte_that_exists(files):
    data, blob, moff, ooff, _ = files["sizes eof=True"]  # members [0, 1, 100, 32768, 31, 0] + EOF
    v = [int(x) for x in sa.bgzf_offsets_to_voffsets(moff, ooff, [0, 1, 101])]
    assert v == [moff[1] << 16, moff[2] << 16, moff[3] << 16]
    assert int(sa.bgzf_offsets_to_voffsets(moff, ooff, [len(data)])[0]) == moff[-1] << 16


def test_invalid_voffsets(files):
    data, blob, moff, ooff, _ = files["sizes eof=True"]
    out_n = ooff[3] - ooff[2]
    bad = [(moff[2] + 1) << 16,            # a coffset inside a member
           moff[2] << 16 | (out_n + 1),    # uoffset = out_n + 1
           (moff[-1] + 28) << 16,          # a coffset past the file
           moff[-1] << 16 | 1]             # the file's end with a uoffset
    assert [int(o) for o in sa.bgzf_voffsets_to_offsets(moff, ooff, bad)] == [NONE] * 4
    assert int(sa.bgzf_offsets_to_voffsets(moff, ooff, [len(data) + 1])[0]) == NONE
    assert len(sa.bgzf_voffsets_to_offsets(moff, ooff, [])) == 0


def test_null_arguments_are_refused():
    L = _capi.lib()
    a = np.zeros(2, np.uint64)
    v = np.zeros(1, np.uint64)
    for fn in (L.sfh_bgzf_voffsets_to_offsets, L.sfh_bgzf_offsets_to_voffsets):
        assert fn(None, a.ctypes.data, 1, 1, v.ctypes.data, v.ctypes.data) == -1
        assert fn(a.ctypes.data, None, 1, 1, v.ctypes.data, v.ctypes.data) == -1
        assert fn(a.ctypes.data, a.ctypes.data, 1, 1, None, v.ctypes.data) == -1
        assert fn(a.ctypes.data, a.ctypes.data, 1, 1, v.ctypes.data, None) == -1
        assert fn(a.ctypes.data, a.ctypes.data, 1, 0, None, None) == 0
