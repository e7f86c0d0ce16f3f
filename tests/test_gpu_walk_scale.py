"""The index walks and their scans beyond one workgroup and at their seams: the BGZF member walk (k_bgzf_* of sf_bgzf.hip), the
flush-point walk (k_any_* of sf_unindexed.hip), the shared u32 scan (k_scan_*) and the dictzip table reader (k_dz_index), at
node counts of 2^k - 1, 2^k and 2^k + 1 around every unit a kernel splits on, with thousands of nodes nobody reaches, and with
a pattern placed on every lane, round, wave and workgroup seam of the scans.  Every comparison is exact equality with the
pure-Python walkers (bgzf_files.walk, unindexed_walk.recover_index, dictzip_files) and the host parsers; the inputs themselves
are held by tests/test_walk_scale_inputs.py without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import bgzf_files as BZ
import dictzip_files as DZ
import starflate_amd
import unindexed_walk as W
from bgzf_range_cases import scale_ranges
from starflate_amd import Compressor, StarflateError, _capi

pytestmark = pytest.mark.gpu

SEG = 32768
NOT_INDEXABLE, DST_TOO_SMALL = -8, -2
ITEM_NOT_INDEXABLE = starflate_amd.ITEM_NOT_INDEXABLE


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


def _cuda(data):
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda() if len(data) else torch.empty(0, dtype=torch.uint8, device="cuda")


def _same(t, data):
    """a device tensor against host bytes, compared on the device"""
    return t.numel() == len(data) and bool(torch.equal(t, _cuda(data)))


# ---- the BGZF member walk ----
def _bgzf_index(comp, blob):
    moff, ooff, info = comp.bgzf_index_tensor(_cuda(blob))
    return [int(v) for v in moff.cpu()], [int(v) for v in ooff.cpu()], info


def _check_bgzf_index(comp, blob, data, key):
    wm, wo, widest, eof = BZ.walk(blob)
    hm, ho, hinfo = starflate_amd.bgzf_index(blob)
    want = {"total_n": len(data), "members": len(wm) - 1, "max_isize": widest, "has_eof": eof}
    assert ([int(v) for v in hm], [int(v) for v in ho], hinfo) == (wm, wo, want), key
    assert _bgzf_index(comp, blob) == (wm, wo, want), key


def _check_bgzf_decode(comp, blob, data, key):
    out, got, st = comp.decompress_bgzf_tensor(_cuda(blob), len(data))
    assert (got, st) == (len(data), 0) and _same(out[:got], data), key


@pytest.mark.parametrize("nodes", BZ.CHAIN_NODES)
def test_bgzf_chain_lengths(comp, nodes):
    """one node short of, at and behind every power of two the jump loop counts by, 256 nodes per workgroup and 1024 lanes of
    k_bgzf_finish; the chain's tail is marked only if the last round runs"""
    data, blob, moff, ooff = BZ.chain_file(nodes)
    _check_bgzf_index(comp, blob, data, nodes)
    if nodes in (257, 1025, 5000):  # k_bgzf_rows, k_bgzf_first and the fold over more than 1024 members
        _check_bgzf_decode(comp, blob, data, nodes)


def test_bgzf_index_arrays_one_entry_short(comp):
    data, blob, moff, ooff = BZ.chain_file(1025)
    src = _cuda(blob)
    m = len(moff) - 1
    arrays = torch.full((2, m + 1), -1, dtype=torch.int64, device="cuda")
    info = _capi.BgzfInfo()
    call = _capi.lib().sfh_bgzf_read_index_device
    assert call(comp._h, src.data_ptr(), src.numel(), C.byref(info), arrays[0].data_ptr(), arrays[1].data_ptr(), m, None) == DST_TOO_SMALL
    assert info.members == m == 1025 and bool((arrays == -1).all())
    assert call(comp._h, src.data_ptr(), src.numel(), C.byref(info), arrays[0].data_ptr(), arrays[1].data_ptr(), m + 1, None) == 0
    assert [int(v) for v in arrays[0].cpu()] == moff and [int(v) for v in arrays[1].cpu()] == ooff


@pytest.mark.parametrize("which", ["two chains of 750 twice", "256 nodes", "1024 nodes"])
def test_bgzf_decoys_at_scale(comp, which):
    """fake heads in stored payloads and in a member's own extra field: thousands of nodes in chains that end on true members
    and that the chain from byte 0 never enters; 256 and 1024 nodes put the sentinel into a workgroup of its own"""
    counts, want = {"two chains of 750 twice": ((1500, 1500), 3005), "256 nodes": ((252,), 256), "1024 nodes": ((1020,), 1024)}[which]
    data, blob, moff, ooff, nodes = BZ.decoy_file(counts)
    assert len(moff) - 1 < 10 and nodes == want
    _check_bgzf_index(comp, blob, data, which)
    _check_bgzf_decode(comp, blob, data, which)


def test_bgzf_member_heads_on_the_scan_seams(comp):
    """a member's first byte on every position within 35 bytes of the scan's first two workgroup boundaries: every lane
    residue, the head's shape bytes and the rest of the header in different workgroups"""
    for which, start in BZ.seam_starts():
        data, blob, moff, ooff = BZ.seam_file(which, start)
        _check_bgzf_index(comp, blob, data, (which, start))
    data, blob, _, _ = BZ.seam_file(1, 8192 - 2)
    _check_bgzf_decode(comp, blob, data, "decode")


def test_bgzf_file_ends(comp):
    """files without an EOF member of every length mod 4 (the scan's last dword), and a file cut 1 .. 18 bytes into a member"""
    for data, blob in BZ.no_eof_files():
        _check_bgzf_index(comp, blob, data, len(blob) % 4)
        _check_bgzf_decode(comp, blob, data, len(blob) % 4)
    for k, blob, st in BZ.cut_files():
        with pytest.raises(StarflateError) as e:
            _bgzf_index(comp, blob)
        assert e.value.code == st, k


def test_bgzf_more_than_one_scan_tile(comp):
    """1202 workgroups of k_bgzf_scan: the second tile of the count scan, k_scan_add with an addend that is not 0"""
    data, blob, moff, ooff = BZ.tile_file()
    _check_bgzf_index(comp, blob, data, "tile")
    _check_bgzf_decode(comp, blob, data, "tile")


@pytest.mark.parametrize("count", [3000, 1024, 1025])
def test_bgzf_range_calls(comp, count):
    """more ranges than one workgroup of k_bgzf_range_spans and one tile of the row scan hold, on a file of 4999 small members"""
    data, blob, moff, ooff = BZ.chain_file(5000)
    ranges = scale_ranges(ooff, len(data), count, seed=count)
    src = _cuda(blob)
    dm, do, info = comp.bgzf_index_tensor(src)
    pos = np.concatenate([[0], np.cumsum([ln for _, ln in ranges])])
    buf = torch.full((int(pos[-1]) + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = [buf[int(pos[i]): int(pos[i + 1])] for i in range(count)]
    _, status = comp.read_bgzf_ranges_tensor(src, dm, do, info, [o for o, _ in ranges], [ln for _, ln in ranges], outs=outs)
    assert not bool(status.any())
    want = b"".join(data[o: o + ln] for o, ln in ranges) + b"\xa5"
    assert _same(buf, want)


# ---- the flush-point walk ----
def _recover(comp, stream, n, container="raw"):
    ix, dep = comp.recover_index(_cuda(stream), n, container)
    return [int(v) for v in ix.cpu()], dep.cpu().numpy()


def _check_walk(comp, data, stream, container="raw", decode=True):
    """the recovered index against the Python walk, the scan's node count against the scan rule, the decode against the data"""
    want = W.recover_index(stream, len(data), container)
    ix, _ = _recover(comp, stream, len(data), container)
    assert ix == want
    b0, e = W.body_range(stream, container)
    # sfh_last_recover_stats counts the scan's nodes without the end sentinel each scanned item's list is closed by
    assert comp.last_recover_stats()["nodes"] == W.scan_nodes(stream, b0, e)
    if decode:
        out, st = comp.decompress_any_tensor(_cuda(stream), len(data), container)
        assert st == 0 and _same(out, data)
    return want


@pytest.mark.parametrize("nodes, container", [(n, "raw") for n in W.CHAIN_NODES] + [(n, c) for n in W.WRAPPED_NODES for c in ("zlib", "gzip")])
def test_flush_chain_lengths(comp, nodes, container):
    """an item of exactly 2^k nodes gets exactly k jump rounds: one too few leaves the chain's tail unmarked"""
    data, stream = W.chain_stream(nodes, container)
    want = _check_walk(comp, data, stream, container, decode=nodes - 1 <= 1025)
    assert len(want) == nodes


def test_flush_rows_beyond_one_workgroup_and_one_tile(comp):
    data, stream = W.rows_stream()
    want = _check_walk(comp, data, stream)
    assert comp.last_recover_stats()["rows"] == W.independent_segments(stream, want) == 187


@pytest.mark.parametrize("kind", ["markers", "headers"])
def test_flush_decoys_at_scale(comp, kind):
    """tens of thousands of markers / stored headers inside stored payloads: over 300 workgroups, 17 jump rounds"""
    data, stream, index = W.decoy_stream(kind)
    assert _check_walk(comp, data, stream) == index
    assert comp.last_recover_stats()["nodes"] > 65000


def test_flush_stored_run_over_the_scan_tile(comp):
    """300 stored segments from the compressor's stored fast path: over 1024 scan waves, one edge of the walk"""
    data = np.random.default_rng(61).integers(0, 256, 300 * SEG, dtype=np.uint8)
    stream = comp.compress(data)
    index = [int(v) for v in comp.last_index()]
    assert len(stream) > 300 * SEG and len(stream) > 1024 * 8192
    assert _check_walk(comp, data.tobytes(), stream) == index


def test_flush_two_segment_edges_across_workgroups(comp):
    data, stream, index = W.alternating_stream()
    assert _check_walk(comp, data, stream) == index
    assert comp.last_recover_stats()["nodes"] == 301


def test_flush_patterns_on_the_scan_seams(comp):
    """a stored header's first byte and a marker's end on every offset within 4 bytes of a wave's piece (8192) and of a round
    (256) of k_any_scan, counted from the stream's first byte; b0 of every residue mod 4"""
    cases = W.seam_cases()
    streams = {name: W.seam_stream(name) for _, _, _, name in cases}
    for name, (data, stream, index) in streams.items():
        assert _check_walk(comp, data, stream, "gzip") == index, name
    # ... and all of them as the items of one call
    names = sorted(streams)
    ix, st = comp.recover_index_batch([_cuda(streams[k][1]) for k in names], [len(streams[k][0]) for k in names], "gzip")
    assert st == [0] * len(names) and [int(v) for v in ix.cpu()] == [v for k in names for v in streams[k][2]]


def test_flush_marker_over_the_body_start(comp):
    """a marker that ends inside [b0, b0 + 4) is no node"""
    data, stream = W.marker_at_b0_stream()
    _check_walk(comp, data, stream, "gzip")
    # the second stream's first block is no segment of 32 KiB: the walk alone (no depends flags, no decode)
    data, stream = W.marker_across_b0_stream()
    want = W.recover_index(stream, len(data), "gzip")
    src = _cuda(stream)
    index = torch.full((len(want),), -1, dtype=torch.int64, device="cuda")
    rc = _capi.lib().sfh_recover_index_device(comp._h, src.data_ptr(), src.numel(), 2, len(data), index.data_ptr(), len(want) - 1, None, None)
    assert rc == 0 and [int(v) for v in index.cpu()] == want
    assert comp.last_recover_stats()["nodes"] == W.scan_nodes(stream, *W.body_range(stream, "gzip")) == 4


def test_flush_many_items_in_one_call(comp):
    """700 items: node lists that straddle workgroups, k_any_ranges and k_any_single on more than 256 items, ten items that
    are not indexable between good neighbours"""
    items = W.many_items()
    want, bad = [], []
    for i, (n, stream) in enumerate(items):
        try:
            want += W.recover_index(stream, n)
        except W.NotIndexable:
            want += [0] * (max(1, -(-n // SEG)) + 1)
            bad.append(i)
    assert bad == list(W.MANY_BAD)
    ix, st = comp.recover_index_batch([_cuda(s) for _, s in items], [n for n, _ in items])
    assert st == [ITEM_NOT_INDEXABLE if i in W.MANY_BAD else 0 for i in range(len(items))]
    assert [int(v) for v in ix.cpu()] == want
    assert comp.last_recover_stats()["nodes"] == sum(W.scan_nodes(s, 0, len(s)) for n, s in items if n > SEG)


# ---- the dictzip table ----
def _dz_index(comp, blob, cap=None):
    src = _cuda(blob)
    index = torch.full((_capi.DZ_MAX_CHUNKS + 1,), -1, dtype=torch.int64, device="cuda")
    info = _capi.DzInfo()
    rc = _capi.lib().sfh_dz_read_index_device(comp._h, src.data_ptr(), src.numel(), C.byref(info), index.data_ptr(),
                                              index.numel() if cap is None else cap, None)
    return rc, info, index.cpu().numpy()


@pytest.mark.parametrize("chunks", DZ.SCALE_CHUNKS)
def test_dictzip_tables_beyond_one_size_per_lane(comp, chunks):
    blob, want = DZ.scale_file(chunks)
    host, total_n = starflate_amd.dictzip_index(blob)
    assert [int(v) for v in host] == want and total_n == chunks * SEG
    rc, info, got = _dz_index(comp, blob)
    assert (rc, info.status, info.nseg, info.total_n, info.header_bytes) == (0, 0, chunks, chunks * SEG, want[0])
    assert got[: chunks + 1].tolist() == want and (got[chunks + 1:] == -1).all()
    if chunks == 1025:
        out, st = comp.decompress_dictzip(blob)
        assert st == 0 and out == bytes(chunks * SEG)


def test_dictzip_table_at_the_formats_limit(comp):
    blob, want = DZ.limit_file()
    host, total_n = starflate_amd.dictzip_index(blob)
    assert [int(v) for v in host] == want and total_n == DZ.MAX_CHUNKS * SEG
    rc, info, got = _dz_index(comp, blob)
    assert (rc, info.status, info.nseg, info.total_n) == (0, 0, DZ.MAX_CHUNKS, DZ.MAX_CHUNKS * SEG)
    assert got.tolist() == want
    rc, info, got = _dz_index(comp, blob, cap=DZ.MAX_CHUNKS)  # one entry short
    assert rc == DST_TOO_SMALL and (got == -1).all()
