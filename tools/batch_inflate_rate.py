"""Batched decompression against a per-item loop and one large call (device buffers, HIP events around a synchronised
call, median of --repeats after a warm-up).  For items of 4 KiB, 64 KiB and 1 MiB of synthetic text (--total bytes in all),
compressed with compress_batch (block_bytes 0: 32 KiB strips below 8 MiB items), rates in MiB/s of decoded output:

  batch       one sfh_decompress_batch_device_async over every item, with the batch index
  batch_sub   the same with the batch sub-index
  loop        sfh_decompress_device once per item (a timed subset when the loop would be slow: `items_timed` says how many)
  single_32k  one sfh_decompress_device over the same bytes compressed as one call with block_bytes = 32768
  zlib_pages  index-free zlib -6 pages of 4 KiB (container zlib: wrapper and Adler-32 checked on the GPU)

usage: python tools/batch_inflate_rate.py OUT.json [--total BYTES] [--repeats N] [--loop-items N]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from starflate_amd import Compressor, build, synth  # noqa: E402

MiB = 1 << 20


def timed(fn, repeats):
    """median milliseconds of fn() between two HIP events, the device idle before each repeat"""
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
    return statistics.median(ts)


def rate(n, ms):
    return {"ms": round(ms, 3), "MiB_s": round(n / MiB / (ms / 1e3), 1)}


def packed(streams):
    """the streams back to back in one device buffer, 16-byte aligned -> (buffer, device pointers, sizes)"""
    offs, at = [], 0
    for s in streams:
        offs.append(at)
        at = (at + len(s) + 15) // 16 * 16
    host = np.zeros(max(at, 16), np.uint8)
    for o, s in zip(offs, streams):
        host[o: o + len(s)] = np.frombuffer(s, np.uint8)
    buf = torch.from_numpy(host).cuda()
    return buf, [buf.data_ptr() + o for o in offs], [len(s) for s in streams]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--total", type=int, default=1 << 30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-items", type=int, default=2048, help="items the per-item loop times at most")
    args = ap.parse_args()
    comp = Compressor(0)
    L, h = comp._lib, comp._h
    text_np = synth.gen_text(args.total, seed=3)
    rows = []
    s = torch.cuda.current_stream().cuda_stream
    for item in (4096, 65536, MiB):
        k = args.total // item
        n = k * item
        streams = comp.compress_batch([text_np[i * item:(i + 1) * item] for i in range(k)])
        idx, sub, bb = comp.last_batch_index()
        buf, sptr, sn = packed(streams)
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        status = torch.empty(k, dtype=torch.int32, device="cuda")
        d_idx = torch.from_numpy(idx.astype(np.int64)).cuda()
        d_sub = torch.from_numpy(sub.view(np.int32)).cuda()
        sp = (C.c_void_p * k)(*sptr)
        dp = (C.c_void_p * k)(*[out.data_ptr() + i * item for i in range(k)])
        nn, dn = (C.c_uint64 * k)(*sn), (C.c_uint64 * k)(*([item] * k))
        bbs = np.ascontiguousarray(bb, np.uint32)

        def batch(sub_ptr):
            comp._check(L.sfh_decompress_batch_device_async(h, k, sp, nn, C.c_void_p(d_idx.data_ptr()), sub_ptr, dp, dn,
                                                            bbs.ctypes.data, 0, C.c_void_p(status.data_ptr()), C.c_void_p(s)))

        ms_b = timed(lambda: batch(None), args.repeats)
        assert int(status.abs().sum()) == 0 and torch.equal(out.cpu(), torch.from_numpy(text_np[:n]))
        ms_bs = timed(lambda: batch(C.c_void_p(d_sub.data_ptr())), args.repeats)
        assert int(status.abs().sum()) == 0
        kl = min(k, args.loop_items)
        per_item = []
        e = 0
        for i in range(kl):
            ns = max(1, -(-item // 32768))
            per_item.append((torch.from_numpy(np.frombuffer(streams[i], np.uint8).copy()).cuda(), d_idx[e: e + ns + 1].clone(),
                             int(bb[i])))
            e += ns + 1

        def loop():
            for i in range(kl):
                comp.decompress_tensor(per_item[i][0], per_item[i][1], item, out=out[i * item:(i + 1) * item], block_bytes=per_item[i][2])

        ms_l = timed(loop, args.repeats) * k / kl
        flat = torch.from_numpy(text_np[:n]).cuda()
        one, one_n = comp.compress_tensor(flat, block_bytes=32768)
        one = one[:one_n].clone()
        one_idx = comp.last_index(device="cuda")
        del flat

        def single():
            comp.decompress_tensor(one, one_idx, n, out=out, block_bytes=32768)

        ms_s = timed(single, args.repeats)
        row = {"item_bytes": item, "items": k, "bytes": n, "batch": rate(n, ms_b), "batch_sub": rate(n, ms_bs),
               "loop": dict(rate(n, ms_l), items_timed=kl,
                            note="per-item sfh_decompress_device; time scaled from the timed subset" if kl < k else "every item"),
               "single_32k": rate(n, ms_s)}
        row["batch_vs_single"] = round(row["batch"]["MiB_s"] / row["single_32k"]["MiB_s"], 3)
        row["batch_sub_vs_single"] = round(row["batch_sub"]["MiB_s"] / row["single_32k"]["MiB_s"], 3)
        row["batch_vs_loop"] = round(row["batch"]["MiB_s"] / row["loop"]["MiB_s"], 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del buf, out, one, one_idx, per_item, d_idx, d_sub
        torch.cuda.empty_cache()
    # index-free zlib -6 pages of 4 KiB (a quarter of --total at most: zlib on the host writes them)
    k = min(args.total, 256 * MiB) // 4096
    pages = [zlib.compress(text_np[i * 4096:(i + 1) * 4096].tobytes(), 6) for i in range(k)]
    buf, sptr, sn = packed(pages)
    out = torch.empty(k * 4096, dtype=torch.uint8, device="cuda")
    status = torch.empty(k, dtype=torch.int32, device="cuda")
    sp = (C.c_void_p * k)(*sptr)
    dp = (C.c_void_p * k)(*[out.data_ptr() + i * 4096 for i in range(k)])
    nn, dn = (C.c_uint64 * k)(*sn), (C.c_uint64 * k)(*([4096] * k))

    def zpages():
        comp._check(L.sfh_decompress_batch_device_async(h, k, sp, nn, None, None, dp, dn, None, 1, C.c_void_p(status.data_ptr()),
                                                        C.c_void_p(s)))

    ms_z = timed(zpages, args.repeats)
    assert int(status.abs().sum()) == 0 and torch.equal(out.cpu(), torch.from_numpy(text_np[: k * 4096]))
    zrow = {"item_bytes": 4096, "items": k, "bytes": k * 4096, "zlib_pages": rate(k * 4096, ms_z),
            "ratio": round(k * 4096 / sum(sn), 4)}
    print(json.dumps(zrow), flush=True)
    res = {"tool": "batch_inflate_rate", "device": torch.cuda.get_device_name(0), "total_bytes": args.total,
           "repeats": args.repeats, "source": build.source_stamp(), "rows": rows, "zlib_pages": zrow}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
