"""The ZIP plan (starflate_amd/csrc/sf_zip_plan.h: the end records, the directory walk, the local headers, the writer's
arithmetic) compiled for the host with every warning an error and compared, field by field, with zipfile and with the pure
Python walker of tests/zip_files.py -- on archives zipfile and numpy wrote, on the damage catalogue, and on what the writer's
own records assemble to.  The same enumeration runs once more in a stand-alone program built with AddressSanitizer + UBSan,
every archive in a heap block of exactly its size, with every truncation and byte corruption of one small archive."""
import ctypes as C
import io
import os
import struct
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

import zip_files as Z
from conftest import ROOT

CLANG = "/opt/rocm/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "zip_index_host.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]


class Info(C.Structure):
    _fields_ = [("entries", C.c_uint64), ("cd_off", C.c_uint64), ("cd_size", C.c_uint64), ("total_out", C.c_uint64),
                ("zip64", C.c_uint32), ("status", C.c_uint32)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = tmp_path_factory.mktemp("sfz") / "libsfz.so"
    subprocess.check_call([CLANG, "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", str(so)])
    L = C.CDLL(str(so))
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.sfz_digest.argtypes = [C.c_char_p, u64]
    L.sfz_digest.restype = u64
    L.sfz_read_index.argtypes = [C.c_char_p, u64, C.POINTER(Info), vp, u64]
    L.sfz_read_index.restype = C.c_int
    L.sfz_find_eocd.argtypes = [C.c_char_p, u64]
    L.sfz_find_eocd.restype = u64
    L.sfz_write_local.argtypes = [vp, C.c_char_p, u32, u32, u32, u32]
    L.sfz_write_central.argtypes = [vp, C.c_char_p, u32, u32, u32, u32, u32]
    L.sfz_write_end.argtypes = [vp, u64, u64, u64]
    L.sfz_end_bytes.argtypes = [u64]
    for f in (L.sfz_write_local, L.sfz_write_central, L.sfz_write_end, L.sfz_end_bytes):
        f.restype = u32
    L.sfz_bound.argtypes = [u64, vp, vp]
    L.sfz_bound.restype = u64
    return L


def read_index(L, data):
    """(rc, info, entries as a structured array): the count call, then the table"""
    info = Info()
    rc = L.sfz_read_index(data, len(data), C.byref(info), None, 0)
    if info.status or info.entries == 0:
        assert rc == 0
        return rc, info, np.zeros(0, Z.ENTRY_DTYPE)
    assert rc == -2  # SFH_E_DST_TOO_SMALL, with the counts filled
    ents = np.zeros(info.entries, Z.ENTRY_DTYPE)
    rc = L.sfz_read_index(data, len(data), C.byref(info), ents.ctypes.data, info.entries)
    return rc, info, ents


def check_against_walker(L, data):
    st, winfo, went = Z.walk(data)
    rc, info, ents = read_index(L, data)
    assert rc == 0 and info.status == st
    if st:
        assert (info.entries, info.cd_off, info.cd_size, info.total_out, info.zip64) == (0, 0, 0, 0, 0)
        return ents
    assert {k: getattr(info, k) for k in winfo} == winfo
    assert len(ents) == len(went)
    for e, w in zip(ents, went):
        for k in ("local_off", "data_off", "csize", "usize", "out_off", "name_off", "crc32", "status", "method", "flags", "name_len"):
            assert int(e[k]) == w[k], (k, w)
        assert int(e["pad"]) == 0
    return ents


ARCHIVES = Z.foreign_archives()


@pytest.mark.parametrize("name", sorted(ARCHIVES))
def test_foreign_archives_field_by_field(plan, name):
    data = ARCHIVES[name]
    ents = check_against_walker(plan, data)
    zf = zipfile.ZipFile(io.BytesIO(data))
    infos = zf.infolist()
    assert len(infos) == len(ents)
    for zi, e in zip(infos, ents):
        assert int(e["status"]) == 0
        assert (int(e["local_off"]), int(e["csize"]), int(e["usize"]), int(e["crc32"])) == (zi.header_offset, zi.compress_size, zi.file_size, zi.CRC)
        assert (int(e["method"]), int(e["flags"])) == (zi.compress_type, zi.flag_bits)
        nm = data[int(e["name_off"]): int(e["name_off"]) + int(e["name_len"])]
        assert nm.decode("utf-8" if zi.flag_bits & 0x800 else "cp437") == zi.orig_filename
        body = data[int(e["data_off"]): int(e["data_off"]) + int(e["csize"])]
        assert (body if zi.compress_type == 0 else zlib.decompress(body, -15)) == zf.read(zi)
    # every entry starts 16-byte aligned in the packed layout
    assert all(int(e["out_off"]) % 16 == 0 for e in ents)


def test_stored_entries_at_every_residue(plan):
    data = Z.residue_archive((0, 1, 17))
    ents = check_against_walker(plan, data)
    for n in (0, 1, 17):
        assert {int(e["data_off"]) % 16 for e in ents if int(e["usize"]) == n} == set(range(16))
    # the name lengths 1 to 17, a 255-byte name and a non-ASCII one
    names = check_against_walker(plan, ARCHIVES["names"])
    assert {int(e["name_len"]) for e in names} >= set(range(1, 18)) | {255}
    assert any(int(e["flags"]) & 0x800 for e in names)


def test_65536_empty_entries_have_the_zip64_end_record(plan):
    data = Z.many_empty(65536)
    rc, info, ents = read_index(plan, data)
    assert rc == 0 and info.status == 0 and info.zip64 == 1 and info.entries == 65536 and info.total_out == 0
    infos = zipfile.ZipFile(io.BytesIO(data)).infolist()
    assert [int(v) for v in ents["local_off"]] == [zi.header_offset for zi in infos]
    assert not ents["status"].any() and not ents["usize"].any()
    # 65535 entries: the classic record alone, its count at the saturation value and no locator
    data = Z.many_empty(65535)
    rc, info, ents = read_index(plan, data)
    assert rc == 0 and info.status == 0 and info.zip64 == 0 and info.entries == 65535


CATALOGUE = Z.damage_catalogue()


@pytest.mark.parametrize("name", sorted(CATALOGUE))
def test_damage_catalogue(plan, name):
    data, want_index, want_entries = CATALOGUE[name]
    ents = check_against_walker(plan, data)
    rc, info, _ = read_index(plan, data)
    assert info.status == want_index
    for i, e in enumerate(ents):
        assert int(e["status"]) == want_entries.get(i, 0), (name, i)


def test_the_end_record_is_the_last_one_whose_comment_ends_the_file(plan):
    good = ARCHIVES["levels"]
    q = plan.sfz_find_eocd(good, len(good))
    assert good[q:q + 4] == b"PK\5\6" and q == len(good) - 22
    # a signature inside the comment that does not end the file is passed over; one that does is taken (the highest counts)
    c = b"xxPK\5\6" + bytes(16) + b"yy"
    withc = good[:q + 20] + struct.pack("<H", len(c)) + c
    assert plan.sfz_find_eocd(withc, len(withc)) == q
    c2 = b"xxPK\5\6" + bytes(16) + struct.pack("<H", 2) + b"yy"
    withc2 = good[:q + 20] + struct.pack("<H", len(c2)) + c2
    assert plan.sfz_find_eocd(withc2, len(withc2)) == q + 22 + 2
    assert plan.sfz_find_eocd(good[:21], 21) == (1 << 64) - 1


def build_with_plan(L, names, bodies, datas):
    out, cd = bytearray(), bytearray()
    buf = C.create_string_buffer(46 + 65535 + 200)
    for name, body, data in zip(names, bodies, datas):
        crc = zlib.crc32(data)
        n = L.sfz_write_central(buf, name, len(name), crc, len(body), len(data), len(out))
        cd += buf.raw[:n]
        n = L.sfz_write_local(buf, name, len(name), crc, len(body), len(data))
        out += buf.raw[:n]
        out += body
    cd_off = len(out)
    n = L.sfz_write_end(buf, len(names), cd_off, len(cd))
    assert n == L.sfz_end_bytes(len(names))
    return bytes(out + cd + buf.raw[:n])


@pytest.mark.parametrize("count", [0, 1, 65535, 65536])
def test_writer_records_assemble_to_an_archive_zipfile_reads(plan, count):
    names = Z.test_names(count)
    if count <= 1:
        datas = [Z.text(70000, 3)] * count
        bodies = [zlib.compress(d, 6)[2:-4] for d in datas]
    else:
        datas, bodies = [b""] * count, [b"\3\0"] * count
    got = build_with_plan(plan, names, bodies, datas)
    assert got == Z.assemble(names, bodies, datas)
    assert len(got) <= Z.zip_bound([len(d) for d in datas], [len(n) for n in names])
    zf = zipfile.ZipFile(io.BytesIO(got))
    assert zf.testzip() is None
    assert [zi.filename.encode("utf-8") for zi in zf.infolist()] == names
    for nm, d in list(zip(names, datas))[:: max(1, count // 50)]:
        assert zf.read(nm.decode("utf-8")) == d
    rc, info, ents = read_index(plan, got)
    assert rc == 0 and info.status == 0 and info.entries == count and info.zip64 == (1 if count > 65535 else 0)
    assert not ents["status"].any()
    if count == 0:
        assert got == b"PK\5\6" + bytes(18)


def test_bound_against_its_restatement(plan):
    for sizes, lens in (([], []), ([0], [1]), ([1, 32768, 32769, 10 ** 9], [1, 17, 255, 65535]), ([5] * 1000, [9] * 1000)):
        a, b = np.array(sizes, np.uint64), np.array(lens, np.uint32)
        assert plan.sfz_bound(len(sizes), a.ctypes.data if sizes else None, b.ctypes.data if sizes else None) == Z.zip_bound(sizes, lens)
    assert Z.zip_bound([], []) == 98


def test_same_enumeration_under_asan_ubsan(plan, tmp_path):
    cases = [ARCHIVES["comments"]] + [ARCHIVES[k] for k in sorted(ARCHIVES)] + [CATALOGUE[k][0] for k in sorted(CATALOGUE)]
    cases += [Z.many_empty(65536), b"", b"PK\5\6"]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for c in cases:
            f.write(struct.pack("<Q", len(c)) + c)
    exe = tmp_path / "zip_index_host"
    subprocess.check_call([CLANG, "-O1", "-g"] + WARN + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", str(exe)])
    out = subprocess.run([str(exe), str(path), "sweep"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == f"{len(cases)} cases"
    for c, line in zip(cases, lines):
        assert int(line) == plan.sfz_digest(c, len(c))
    # the sweep ended in a status or an index every time, and both builds agree on all of it
    assert lines[len(cases)].startswith("sweep ")
