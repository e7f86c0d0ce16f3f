"""The inputs of tests/test_gpu_walk_scale.py, held on the CPU: every generated file has the node count, the member count, the
seam position and the length class that the GPU test relies on, and the pure-Python walkers and the host parsers agree on
it.  Nothing here runs a kernel; what the kernels split on is stated beside each check."""
import zlib

import numpy as np
import pytest

import bgzf_files as BZ
import dictzip_files as DZ
import starflate_amd
import unindexed_walk as W
from bgzf_range_cases import scale_ranges

SEG = 32768


# ---- the BGZF member walk: 256 nodes per workgroup, 1024 lanes in k_bgzf_finish, 8192 bytes per scan workgroup ----
def _host_index(blob):
    moff, ooff, info = starflate_amd.bgzf_index(blob)
    return [int(v) for v in moff], [int(v) for v in ooff], info


def _check_bgzf(data, blob, moff, ooff, nodes):
    wm, wo, widest, eof = BZ.walk(blob)
    assert (wm, wo) == (moff, ooff) and wo[-1] == len(data)
    hm, ho, info = _host_index(blob)
    assert (hm, ho) == (wm, wo) and info == {"total_n": len(data), "members": len(wm) - 1, "max_isize": widest, "has_eof": eof}
    assert BZ.parse_nodes(blob) == nodes
    # every member inflates alone to its slice of the data
    assert b"".join(zlib.decompress(blob[moff[k]: moff[k + 1]], wbits=31) for k in range(len(moff) - 1)) == data


def test_bgzf_chain_files_have_exactly_their_nodes():
    data, members, sizes = BZ.tiny_members()
    assert len(members) == 5055 and min(sizes) == 0 and max(sizes) == 79 and 300 << 10 < sum(map(len, members)) < 340 << 10
    assert BZ.CHAIN_NODES == (1, 2, 3, 4, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 5000)
    for nodes in BZ.CHAIN_NODES:
        data, blob, moff, ooff = BZ.chain_file(nodes)
        assert len(moff) - 1 == nodes and BZ.walk(blob)[3]  # the EOF member included; no node but the members
        _check_bgzf(data, blob, moff, ooff, nodes)
        assert BZ.node_positions(blob) == moff[:-1]


def test_bgzf_decoy_files():
    data, blob, moff, ooff, nodes = BZ.decoy_file((1500, 1500))
    assert len(moff) - 1 == 4 and nodes == 3000 + 4 + 1  # the decoys, the members, the fake head in an extra field
    _check_bgzf(data, blob, moff, ooff, nodes)
    pos = BZ.node_positions(blob)
    for m, count in ((0, 1500), (1, 1500)):
        first = moff[m] + BZ.HEAD + 5
        decoys = [first + 18 * k for k in range(count)]
        assert set(decoys) <= set(pos)
        size = [BZ.parse_at(blob, p)[0] for p in decoys]
        # each lands on the decoy two ahead: two chains of 750, either one's last decoy on the next true member's first byte
        assert all(decoys[k] + size[k] == decoys[k + 2] for k in range(count - 2))
        assert decoys[-2] + size[-2] == moff[m + 1] == decoys[-1] + size[-1]
    # the fake head in the text member's own extra field lands on the member behind it
    fake = moff[2] + 16
    assert fake in pos and blob[moff[2] + 12: moff[2] + 14] == b"XY" and fake + BZ.parse_at(blob, fake)[0] == moff[3]
    assert len(pos) == nodes and sorted(set(pos) - set(moff)) == sorted(
        [moff[m] + BZ.HEAD + 5 + 18 * k for m in (0, 1) for k in range(1500)] + [fake])
    for want in (256, 1024):  # the sentinel in the next workgroup, the second lane run of k_bgzf_finish untouched: < 10 members
        data, blob, moff, ooff, nodes = BZ.decoy_file_of(want)
        assert nodes == want and len(moff) - 1 == 3
        _check_bgzf(data, blob, moff, ooff, want)


def test_bgzf_seam_files():
    starts = BZ.seam_starts()
    assert len(starts) == 2 * 71
    assert {s for w, s in starts if w == 1} == set(range(8192 - 35, 8192 + 36))
    assert {s for w, s in starts if w == 2} == set(range(16384 - 35, 16384 + 36))
    assert {s % 32 for w, s in starts if w == 1} == set(range(32))  # every lane residue of the scan
    for which, start in starts:
        data, blob, moff, ooff = BZ.seam_file(which, start)
        assert moff[which] == start and len(moff) - 1 == 4
        _check_bgzf(data, blob, moff, ooff, 4)
    # the head's four shape bytes and the rest of the header on either side of the boundary, and the shape bytes across it
    for seam, which in zip(BZ.SEAMS, (1, 2)):
        got = {s - seam for w, s in starts if w == which}
        assert {-4, -3, -2, -1, 0, -18, -12} <= got


def test_bgzf_files_without_eof_member_and_cuts():
    files = BZ.no_eof_files()
    assert sorted(len(blob) % 4 for _, blob in files) == [0, 1, 2, 3]
    for data, blob in files:
        wm, wo, _, eof = BZ.walk(blob)
        assert not eof and len(wm) - 1 == 2 and wo[-1] == len(data) and BZ.parse_nodes(blob) == 2
        assert _host_index(blob)[2]["has_eof"] is False
    cuts = BZ.cut_files()
    assert [k for k, _, _ in cuts] == list(range(1, 13)) + [16, 17, 18]
    for k, blob, st in cuts:
        assert st == BZ.SRC_TOO_SMALL, k
        with pytest.raises(starflate_amd.StarflateError) as e:
            starflate_amd.bgzf_index(blob)
        assert e.value.code == st, k
        assert BZ.parse_nodes(blob) == 1  # the first member alone


def test_bgzf_tile_file():
    data, blob, moff, ooff = BZ.tile_file()
    assert len(moff) - 1 == 301 and len(blob) > 1024 * 8192  # the scan's counts fill more than one tile of the u32 scan
    assert -(-len(blob) // 8192) == 1202
    wm, wo, widest, eof = BZ.walk(blob)
    assert (wm, wo, widest, eof) == (moff, ooff, SEG, True)
    assert BZ.parse_nodes(blob) == 301
    assert _host_index(blob)[:2] == (wm, wo)


def test_bgzf_range_sets():
    data, blob, moff, ooff = BZ.chain_file(5000)
    for count in (3000, 1024, 1025):
        ranges = scale_ranges(ooff, len(data), count, seed=count)
        assert len(ranges) == count and all(0 <= o and o + n <= len(data) and n <= 200 for o, n in ranges)
        edges = set(ooff[2500: 2550])
        near = [r for r in ranges if any(abs(r[0] - b) <= 2 or abs(r[0] + r[1] - b) <= 2 for b in edges)]
        assert len(near) >= (1000 if count == 3000 else 500) and {0, 1, 3, 4, 5, 200} <= {n for _, n in near}


# ---- the flush-point walk: 256 nodes per workgroup, 1024 entries per scan tile, 8192 bytes per wave, 256 per round ----
def _check_stream(data, stream, index, container="raw"):
    assert zlib.decompressobj(W.WBITS[container]).decompress(stream) == data
    assert W.recover_index(stream, len(data), container) == index


def test_flush_chain_streams_have_exactly_their_nodes():
    assert W.CHAIN_NODES == (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097)
    for nodes in W.CHAIN_NODES:
        for container in ("raw", "zlib", "gzip") if nodes in W.WRAPPED_NODES else ("raw",):
            data, stream = W.chain_stream(nodes, container)
            b0, e = W.body_range(stream, container)
            assert len(data) == (nodes - 1) * SEG and W.scan_nodes(stream, b0, e) == nodes, (nodes, container)
            ix = W.recover_index(stream, len(data), container)
            assert len(ix) == nodes and ix[0] == b0 and ix[-1] == e
            if nodes <= 513:
                assert zlib.decompressobj(W.WBITS[container]).decompress(stream) == data
    assert len(W.WRAPPED_NODES) == 3 and set(W.WRAPPED_NODES) <= set(W.CHAIN_NODES)


def test_flush_rows_stream():
    data, stream = W.rows_stream()
    assert len(data) == 1300 * SEG and zlib.decompressobj(-15).decompress(stream) == data
    ix = W.recover_index(stream, len(data))
    assert len(ix) == 1301 and W.scan_nodes(stream, 0, len(stream)) == 1301
    rows = W.independent_segments(stream, ix)
    # segment 0, and every segment behind a full flush: more rows than one workgroup of k_any_rows_*, segments over two tiles
    assert rows == 1 + len([k for k in range(1299) if k % 7 == 0]) == 187


def test_flush_decoy_streams():
    for kind, per_segment in (("markers", 8192), ("headers", 6553)):
        data, stream, index = W.decoy_stream(kind)
        _check_stream(data, stream, index)
        assert len(index) - 1 == 21
        nodes = W.scan_nodes(stream, 0, len(stream))
        # b0, one marker behind each of the 11 coded segments, and the decoys; the stored segments' own headers stand where a
        # coded segment's marker ends
        assert nodes == 1 + 11 + 10 * per_segment, kind
        assert nodes > (80000 if kind == "markers" else 65000) and nodes.bit_length() == 17  # 17 rounds of the jump
    data, stream, index = W.decoy_stream("markers")
    assert stream[index[2] - 4: index[2]] == W.MARK  # a stored payload's last marker ends on the next segment's first byte


def test_flush_alternating_stream():
    data, stream, index = W.alternating_stream()
    _check_stream(data, stream, index)
    assert len(index) - 1 == 600
    assert W.scan_nodes(stream, 0, len(stream)) == 301  # the stored headers and the last marker: coded starts are no nodes
    for k in (0, 2, 254, 256, 258, 598):
        assert W.is_stored_header(stream, index[k], len(stream)) and W.landing(stream, index[k], len(stream)) == index[k + 1]
        assert not W.is_stored_header(stream, index[k + 1], len(stream)) and stream[index[k + 1] - 4: index[k + 1]] != W.MARK


def test_flush_seam_streams():
    cases = W.seam_cases()
    assert len(cases) == 2 * 2 * 9
    seen = set()
    for what, mod, d, name in cases:
        data, stream, index = W.seam_stream(name)
        _check_stream(data, stream, index, "gzip")
        b0, e = W.body_range(stream, "gzip")
        assert index[0] == b0 and index[-1] == e
        at = index[2] if what == "H" else index[4]
        assert (at - d) % mod == 0 and (mod == 8192 or (at - d) % 8192 != 0), (what, mod, d)
        if what == "H":  # a stored header no marker ends at
            assert W.is_stored_header(stream, at, e) and stream[at - 4: at] != W.MARK
        else:  # the end of a marker where no stored block starts
            assert stream[at - 4: at] == W.MARK and not W.is_stored_header(stream, at, e)
        assert W.scan_nodes(stream, b0, e) == 5  # b0, segments 1 (marker and header), 2 (header), 4 and the last marker
        seen.add((what, mod, d, b0 % 4))
    assert {(w, m, d) for w, m, d, _ in seen} == {(w, m, d) for w in "HM" for m in (8192, 256) for d in range(-4, 5)}
    assert {r for _, _, _, r in seen} == {0, 1, 2, 3}


def test_flush_markers_at_the_body_start():
    data, stream = W.marker_at_b0_stream()
    b0, e = W.body_range(stream, "gzip")
    assert stream[b0 - 4: b0] == W.MARK and zlib.decompress(stream, wbits=31) == data
    ix = W.recover_index(stream, len(data), "gzip")
    assert len(ix) == 4 and W.scan_nodes(stream, b0, e) == 4  # b0 and three markers behind it
    data, stream = W.marker_across_b0_stream()
    b0, e = W.body_range(stream, "gzip")
    assert stream[b0 - 1: b0 + 3] == W.MARK and zlib.decompress(stream, wbits=31) == data and len(data) == 4 * SEG
    ix = W.recover_index(stream, len(data), "gzip")  # the Python walk's outcome: an index, without b0 + 3
    assert len(ix) == 5 and ix[0] == b0 and ix[1] > b0 + 65535 and W.scan_nodes(stream, b0, e) == 4


def test_flush_many_items():
    items = W.many_items()
    assert len(items) == 700 and len(W.MANY_BAD) == 10
    kinds = {"one": 0, "few": 0, "long": 0, "bad": 0}
    for i, (n, stream) in enumerate(items):
        nseg = max(1, -(-n // SEG))
        try:
            ix = W.recover_index(stream, n)
            assert len(ix) == nseg + 1 and i not in W.MANY_BAD
            kinds["one" if nseg == 1 else "long" if nseg == 600 else "few"] += 1
            assert nseg in (1, 2, 3, 4, 5, 600)
        except W.NotIndexable:
            assert i in W.MANY_BAD and 2 <= nseg <= 5
            kinds["bad"] += 1
    assert kinds["bad"] == 10 and kinds["long"] == 2 and kinds["one"] > 200 and kinds["few"] > 400
    assert sum(1 for n, _ in items if n > SEG) > 256  # k_any_ranges on more than one workgroup of scanned items
    assert all(0 < i < 699 and i - 1 not in W.MANY_BAD and i + 1 not in W.MANY_BAD for i in W.MANY_BAD)


# ---- the dictzip table: one workgroup of 1024 lanes, a run of sizes per lane ----
def test_dictzip_scale_files():
    assert DZ.SCALE_CHUNKS == (1023, 1024, 1025, 2048, 2049, 4100)
    for chunks in DZ.SCALE_CHUNKS:
        blob, index = DZ.scale_file(chunks)
        assert len(index) == chunks + 1 and index[-1] == len(blob) - 8
        host, total_n = starflate_amd.dictzip_index(blob)
        assert [int(v) for v in host] == index and total_n == chunks * SEG
        for k in (0, chunks // 2, chunks - 1):
            assert zlib.decompressobj(-15).decompress(blob[index[k]: index[k + 1]]) == bytes(SEG)


def test_dictzip_limit_file():
    blob, index = DZ.limit_file()
    assert DZ.MAX_CHUNKS == 32762 and len(index) == 32763 and index[-1] == len(blob) - 8
    sizes = np.diff(np.asarray(index))
    assert sizes.min() == 20 and sizes.max() == 60 and int.from_bytes(blob[-4:], "little") == 32762 * SEG
    host, total_n = starflate_amd.dictzip_index(blob)
    assert [int(v) for v in host] == index and total_n == 32762 * SEG
