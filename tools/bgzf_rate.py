"""BGZF (sfh_compress_bgzf*, sfh_bgzf_read_index_device, sfh_decompress_bgzf*) against the paths it extends, on --total bytes of
synthetic text resident in HBM (device buffers, HIP events around a synchronised call, median and spread of --repeats after a
warm-up):

  compress  sfh_compress_bgzf_device_async against sfh_compress_device_async with SFH_GZIP at block_bytes = 32768 on the same
            bytes, the file's size against that stream's, and the stage times of one profiled call each
  walk      sfh_bgzf_read_index_device (every member found by pointer jumping) with its member count, against
            sfh_dz_read_index_device on the dictzip file of the same input (a table in one header)
  decode    sfh_decompress_bgzf_device against sfh_decompress_batch_device_async without an index on the same members as
            separate, 16-byte aligned items
  fallback  sfh_decompress_bgzf (host buffers, wall clock) on a file of 65280-byte members made with zlib, --fallback-total
            bytes, against sfh_inflate_stream_batch on those members as items

usage: python tools/bgzf_rate.py OUT.json [--total BYTES] [--fallback-total BYTES] [--repeats N]"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from starflate_amd import Compressor, _capi, build, synth  # noqa: E402

MiB = 1 << 20
SEG = 32768


def timed(fn, repeats):
    """(median, min, max) milliseconds of fn() between two HIP events, the device idle before each repeat"""
    fn()  # warm-up (scratch, pinned tables, kernels loaded)
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def wall(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def rate(n, t):
    ms, lo, hi = t
    return {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "MiB_s": round(n / MiB / (ms / 1e3), 1)}


def zlib_member(payload):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    body = c.compress(payload) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(body) + 8 - 1) + body +
            struct.pack("<II", zlib.crc32(payload), len(payload)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--total", type=int, default=256 * MiB)
    ap.add_argument("--fallback-total", type=int, default=64 * MiB)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    comp = Compressor(0)
    L, h = comp._lib, comp._h
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    total = args.total
    members = -(-total // SEG) + 1
    flat = synth.gen_text_torch(total, seed=3)
    out = torch.empty(L.sfh_bgzf_bound(total), dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int64, device="cuda")
    res, files = {}, {}

    # compress: the BGZF call against the gzip stream at block_bytes = 32768
    calls = {"gzip": lambda: comp.compress_tensor_async(flat, out, size, container="gzip", block_bytes=SEG),
             "dictzip": lambda: comp.compress_tensor_async(flat, out, size, container="dictzip", block_bytes=SEG),
             "bgzf": lambda: comp.compress_bgzf_tensor_async(flat, out, size)}
    for name, call in calls.items():
        t = timed(call, args.repeats)
        n = int(size.item())
        files[name] = out[:n].clone()
        comp.set_profiling(True)
        call()
        torch.cuda.synchronize()
        stages = comp.stage_ms()
        comp.set_profiling(False)
        res[f"compress_{name}"] = dict(rate(total, t), stream_bytes=n, stage_ms={k: round(v, 4) for k, v in stages.items()})
    res["compress_bgzf_over_gzip"] = round(res["compress_bgzf"]["ms"] / res["compress_gzip"]["ms"], 4)
    res["bgzf_bytes_over_gzip_bytes"] = round(res["compress_bgzf"]["stream_bytes"] / res["compress_gzip"]["stream_bytes"], 5)
    del out
    torch.cuda.empty_cache()

    # walk: the members found on the device against a dictzip table read
    blob = files["bgzf"]
    moff = torch.empty(members + 1, dtype=torch.int64, device="cuda")
    ooff = torch.empty(members + 1, dtype=torch.int64, device="cuda")
    info = _capi.BgzfInfo()
    dz = files["dictzip"]
    idx_dz = torch.empty(members + 1, dtype=torch.int64, device="cuda")
    dzinfo = _capi.DzInfo()

    def walk():
        comp._check(L.sfh_bgzf_read_index_device(h, blob.data_ptr(), blob.numel(), C.byref(info), moff.data_ptr(), ooff.data_ptr(),
                                                 members + 1, s))

    def read_dz():
        comp._check(L.sfh_dz_read_index_device(h, dz.data_ptr(), dz.numel(), C.byref(dzinfo), idx_dz.data_ptr(), members + 1, s))

    t_walk = timed(walk, args.repeats)
    assert (info.total_n, info.members, info.max_isize, info.has_eof, info.status) == (total, members, min(total, SEG), 1, 0)
    res["walk_bgzf"] = dict(rate(blob.numel(), t_walk), members=members)
    if total <= _capi.DZ_MAX_CHUNKS * SEG:
        res["index_dz_read"] = rate(dz.numel(), timed(read_dz, args.repeats))

    # decode: the file against its members as separate aligned items of the batch decoder
    back = torch.empty(total, dtype=torch.uint8, device="cuda")
    got, st = C.c_uint64(0), C.c_uint32(0)

    def decode_bgzf():
        comp._check(L.sfh_decompress_bgzf_device(h, blob.data_ptr(), blob.numel(), back.data_ptr(), total, C.byref(got), C.byref(st), s))

    back.zero_()
    t_dec = timed(decode_bgzf, args.repeats)
    assert st.value == 0 and got.value == total and torch.equal(back, flat)
    res["decode_bgzf"] = rate(total, t_dec)
    m_host = moff.cpu().numpy()
    starts = np.zeros(members + 1, np.int64)
    for i in range(members):
        starts[i + 1] = (starts[i] + (m_host[i + 1] - m_host[i]) + 15) // 16 * 16
    packed = torch.zeros(int(starts[-1]) + 16, dtype=torch.uint8, device="cuda")
    items, outs, sizes = [], [], []
    for i in range(members - 1):  # (the EOF member holds nothing)
        n_i = int(m_host[i + 1] - m_host[i])
        packed[int(starts[i]): int(starts[i]) + n_i] = blob[int(m_host[i]): int(m_host[i + 1])]
        items.append(packed[int(starts[i]): int(starts[i]) + n_i])
        sizes.append(min(SEG, total - i * SEG))
        outs.append(back[i * SEG: i * SEG + sizes[-1]])
    status = {}

    def decode_batch():
        status["st"] = comp.decompress_batch_tensors(items, sizes, container="gzip", outs=outs)[1]

    back.zero_()
    t_batch = timed(decode_batch, args.repeats)
    assert int(status["st"].abs().sum().item()) == 0 and torch.equal(back, flat)
    res["decode_batch_items"] = rate(total, t_batch)
    res["decode_bgzf_over_batch_items"] = round(t_dec[0] / t_batch[0], 3)
    del packed, back, items, outs
    torch.cuda.empty_cache()

    # the host fallback: members of 65280 bytes, as bgzip writes them
    ft = args.fallback_total
    data = synth.gen_text(ft, seed=5).tobytes()
    parts = [zlib_member(data[k: k + 65280]) for k in range(0, ft, 65280)] + [zlib_member(b"")]
    big = b"".join(parts)
    res["fallback_bgzf"] = dict(rate(ft, wall(lambda: comp.decompress_bgzf(big), 3)), members=len(parts), file_bytes=len(big))
    assert comp.decompress_bgzf(big) == (data, 0)
    caps = [min(65280, ft - k) for k in range(0, ft, 65280)] + [0]
    res["fallback_stream_batch_items"] = rate(ft, wall(lambda: comp.decompress_stream_batch(parts, caps, "gzip"), 3))

    res = dict({"tool": "bgzf_rate", "device": torch.cuda.get_device_name(0), "total_bytes": total, "members": members,
                "repeats": args.repeats, "source": build.source_stamp(), "ratio": round(total / blob.numel(), 4)}, **res)
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
