"""ZIP archives (sfh_compress_zip*, sfh_zip_read_index_device, sfh_decompress_zip_device) against the paths they extend, on
--items items of --item-bytes of synthetic text resident in HBM (device buffers, HIP events around a synchronised call, median
and spread of --repeats after a warm-up):

  write     sfh_compress_zip_device_async against sfh_compress_batch_device_async (raw) on the same items, in the same run: the
            difference is the pack, the CRC-32 and the headers
  read_own  sfh_decompress_zip_device on that archive against sfh_decompress_any_batch_device on the same bodies as separate,
            16-byte aligned items
  read_zlib sfh_decompress_zip_device on a zipfile level-6 archive of the same items against sfh_inflate_stream_batch_device on
            its bodies as separate items
  stored    sfh_decompress_zip_device on a stored archive of the same items against a device-to-device hipMemcpyAsync of the
            same bytes plus sfh_checksum_device over them
  index     sfh_zip_read_index_device on an archive of --index-entries empty entries (host walk, copies, k_zip_locals), and the
            host walk (sfh_zip_read_index) alone, wall clock

usage: python tools/zip_rate.py OUT.json [--items N] [--item-bytes BYTES] [--index-entries N] [--repeats N]"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time
import zipfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import starflate_amd  # noqa: E402
from starflate_amd import Compressor, _capi, build, synth  # noqa: E402

MiB = 1 << 20


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


def aligned_items(blob, ents):
    """every entry's body as a 16-byte aligned tensor of its own (what the batch decoders take)"""
    host = np.frombuffer(blob, np.uint8)
    offs = np.concatenate([[0], np.cumsum((ents["csize"].astype(np.int64) + 15) & ~15)])
    pool = torch.zeros(int(offs[-1]) + 16, dtype=torch.uint8, device="cuda")
    packed = np.zeros(int(offs[-1]) + 16, np.uint8)
    for o, e in zip(offs, ents):
        packed[int(o): int(o) + int(e["csize"])] = host[int(e["data_off"]): int(e["data_off"]) + int(e["csize"])]
    pool.copy_(torch.from_numpy(packed))
    return pool, [pool[int(o): int(o) + int(e["csize"])] for o, e in zip(offs, ents)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--item-bytes", type=int, default=65536)
    ap.add_argument("--index-entries", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    comp = Compressor(0)
    L, h = comp._lib, comp._h
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    k, n = args.items, args.item_bytes
    total = k * n
    flat = synth.gen_text_torch(total, seed=3)
    srcs = [flat[i * n: (i + 1) * n] for i in range(k)]
    names = [b"item%06d.txt" % i for i in range(k)]
    res = {}

    # write: the archive against the raw batch on the same items
    cap = starflate_amd.zip_bound([n] * k, [len(b) for b in names])
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    outs = [torch.empty(comp.compress_bound(n), dtype=torch.uint8, device="cuda") for _ in range(k)]
    size = {}

    def write_zip():
        size["zip"] = comp.compress_zip_tensors(names, srcs, out=out)[1]

    def write_batch():
        size["batch"] = comp.compress_batch_tensors(srcs, outs=outs)[1]

    t_batch = timed(write_batch, args.repeats)
    t_zip = timed(write_zip, args.repeats)
    zip_n = int(size["zip"].item())
    res["write_batch_raw"] = dict(rate(total, t_batch), stream_bytes=int(size["batch"].sum().item()))
    res["write_zip"] = dict(rate(total, t_zip), archive_bytes=zip_n)
    res["write_zip_over_batch"] = round(t_zip[0] / t_batch[0], 4)
    own = out[:zip_n].clone()
    own_host = own.cpu().numpy().tobytes()
    assert zipfile.ZipFile(io.BytesIO(own_host)).testzip() is None
    del out, outs
    torch.cuda.empty_cache()

    # read: the archive against its bodies as separate aligned items, own and zlib-made
    back = torch.empty(k * ((n + 15) & ~15), dtype=torch.uint8, device="cuda")
    dsts = [back[i * n: (i + 1) * n] for i in range(k)]
    host_items = flat.cpu().numpy().tobytes()
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=6) as z:
        for i in range(k):
            z.writestr(names[i].decode(), host_items[i * n: (i + 1) * n])
    f0 = io.BytesIO()
    with zipfile.ZipFile(f0, "w", compression=zipfile.ZIP_STORED) as z:
        for i in range(k):
            z.writestr(names[i].decode(), host_items[i * n: (i + 1) * n])
    for label, blob, other in (("own", own_host, "any"), ("zlib6", f.getvalue(), "stream"), ("stored", f0.getvalue(), "memcpy")):
        dev = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
        info, ents = comp.zip_index_tensor(dev)
        assert info["status"] == 0 and info["entries"] == k
        st = {"zip": np.zeros(k, np.uint32)}
        # (the C call itself, its arguments marshalled once: 4096 tensors through the Python wrapper cost more than the decode)
        rows = np.ascontiguousarray(ents)
        dp = (C.c_void_p * k)(*[t.data_ptr() for t in dsts])
        caps = (C.c_uint64 * k)(*[n] * k)

        def read_zip():
            comp._check(L.sfh_decompress_zip_device(h, dev.data_ptr(), dev.numel(), C.c_void_p(rows.ctypes.data), k, dp, caps,
                                                    C.c_void_p(st["zip"].ctypes.data), s))

        back.zero_()
        t = timed(read_zip, args.repeats)
        assert not st["zip"].any() and back[: total].equal(flat)
        res[f"read_{label}_zip"] = dict(rate(total, t), archive_bytes=len(blob),
                                        recover_rows=int(comp.last_recover_stats()["rows"]), stream_chunks=int(comp.last_stream_stats()["confirmed"]))
        if other == "memcpy":
            crc = C.c_uint32(0)

            def copy_and_check():
                back[:total].copy_(dev[int(ents["data_off"][0]): int(ents["data_off"][0]) + total], non_blocking=True)
                comp._check(L.sfh_checksum_device(h, back.data_ptr(), total, 2, C.byref(crc), s))

            res["read_stored_memcpy_crc"] = rate(total, timed(copy_and_check, args.repeats))
            continue
        pool, items = aligned_items(blob, ents)

        sp = (C.c_void_p * k)(*[t.data_ptr() for t in items])
        sn = (C.c_uint64 * k)(*[t.numel() for t in items])
        got, ost = (C.c_uint64 * k)(), (C.c_uint32 * k)()
        st["other"] = ost

        def read_items():
            if other == "any":
                comp._check(L.sfh_decompress_any_batch_device(h, k, sp, sn, 0, dp, caps, caps, got, ost, s))
            else:
                comp._check(L.sfh_inflate_stream_batch_device(h, k, sp, sn, 0, dp, caps, got, ost, s))

        back.zero_()
        t = timed(read_items, args.repeats)
        assert not any(st["other"]) and all(int(g) == n for g in got) and back[: total].equal(flat)
        res[f"read_{label}_{other}_batch"] = rate(total, t)
        res[f"read_{label}_zip_over_{other}"] = round(res[f"read_{label}_zip"]["ms"] / res[f"read_{label}_{other}_batch"]["ms"], 4)
        del pool, items, dev
        torch.cuda.empty_cache()

    # index: an archive of many empty entries
    m = args.index_entries
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w") as z:
        for i in range(m):
            z.writestr("e%07d" % i, b"")
    blob = f.getvalue()
    dev = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    info = _capi.ZipInfo()
    ents = np.zeros(m, starflate_amd.ZIP_ENTRY_DTYPE)

    def index_device():
        comp._check(L.sfh_zip_read_index_device(h, dev.data_ptr(), dev.numel(), C.byref(info), C.c_void_p(ents.ctypes.data), m, s))

    def index_host():
        assert L.sfh_zip_read_index(blob, len(blob), C.byref(info), C.c_void_p(ents.ctypes.data), m) == 0

    res["index_device"] = dict(rate(len(blob), wall(index_device, args.repeats)), entries=m, wall_clock=True)
    assert info.entries == m and info.status == 0 and not ents["status"].any()
    res["index_host_walk"] = dict(rate(len(blob), wall(index_host, args.repeats)), entries=m, wall_clock=True)

    props = _capi.device_props(0)
    doc = {"tool": "zip_rate", "device": props["name"], "items": k, "item_bytes": n, "total_bytes": total, "repeats": args.repeats,
           "source": build.source_stamp(), **res}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
