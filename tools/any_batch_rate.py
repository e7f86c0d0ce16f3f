"""Batched index-free decompression (sfh_decompress_any_batch_device) against the three other ways to read the same streams
back (device buffers; a host clock around calls that end in a device synchronise; after a warm-up of every call, the four are
timed in turn, --repeats rounds; median, minimum and maximum are reported).  --total bytes of synthetic text, cut into items of
64 KiB, 256 KiB, 1 MiB, 16 MiB and 256 MiB and written by compress_batch (raw streams); rates in MiB/s of decoded output:

  any_batch      one sfh_decompress_any_batch_device over every item: nothing but the streams and their sizes
  loop           sfh_decompress_any_device once per item (a timed subset when the loop would be slow: `items_timed`)
  stream_batch   one sfh_inflate_stream_batch_device: the decoder that needs no flush points
  indexed_batch  one sfh_decompress_batch_device_async with the writer's index and strips: the ceiling

`recover` holds sfh_last_recover_stats of one more any_batch call with profiling on: the scan and walk times, the share of the gap
to indexed_batch they account for.

usage: python tools/any_batch_rate.py OUT.json [--total BYTES] [--repeats N] [--loop-items N] [--items BYTES ...]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from starflate_amd import Compressor, build, synth  # noqa: E402

MiB = 1 << 20
SEG = 32768


def timed_in_turn(fns, repeats):
    """{name: [ms, ...]}: every fn once as a warm-up, then `repeats` rounds in which each runs once, the device idle before"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    return ts


def rate(n, ms, scale=1.0):
    ms = [t * scale for t in ms]
    med = statistics.median(ms)
    return {"ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "MiB_s": round(n / MiB / (med / 1e3), 1)}


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
    ap.add_argument("--loop-items", type=int, default=1024, help="items the per-item loop times at most")
    ap.add_argument("--items", type=int, nargs="*", default=[64 << 10, 256 << 10, MiB, 16 * MiB, 256 * MiB])
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least 5")
    comp = Compressor(0)
    L, h = comp._lib, comp._h
    text_np = synth.gen_text(args.total, seed=3)
    flat = torch.from_numpy(text_np).cuda()
    rows = []
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for item in args.items:
        k = args.total // item
        if k == 0:
            continue
        n = k * item
        streams = comp.compress_batch([text_np[i * item:(i + 1) * item] for i in range(k)])
        idx, _, bb = comp.last_batch_index()
        buf, sptr, sn = packed(streams)
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_status = torch.empty(k, dtype=torch.int32, device="cuda")
        d_idx = torch.from_numpy(idx.astype(np.int64)).cuda()
        sp = (C.c_void_p * k)(*sptr)
        dp = (C.c_void_p * k)(*[out.data_ptr() + i * item for i in range(k)])
        nn, dn = (C.c_uint64 * k)(*sn), (C.c_uint64 * k)(*([item] * k))
        out_n, st = (C.c_uint64 * k)(), (C.c_uint32 * k)()
        bbs = np.ascontiguousarray(bb, np.uint32)
        kl = min(k, args.loop_items)
        one = C.c_uint32(0)

        def any_batch():
            comp._check(L.sfh_decompress_any_batch_device(h, k, sp, nn, 0, dp, dn, dn, out_n, st, s))

        def loop():
            for i in range(kl):
                comp._check(L.sfh_decompress_any_device(h, sp[i], sn[i], 0, dp[i], item, C.byref(one), s))

        def stream_batch():
            comp._check(L.sfh_inflate_stream_batch_device(h, k, sp, nn, 0, dp, dn, out_n, st, s))

        def indexed_batch():
            comp._check(L.sfh_decompress_batch_device_async(h, k, sp, nn, C.c_void_p(d_idx.data_ptr()), None, dp, dn,
                                                            bbs.ctypes.data, 0, C.c_void_p(d_status.data_ptr()), s))

        # what each call decodes, checked once before anything is timed
        for fn in (indexed_batch, stream_batch, any_batch):
            out.zero_()
            fn()
            torch.cuda.synchronize()
            assert torch.equal(out, flat[:n]), fn.__name__
        assert not any(st) and int(d_status.abs().sum()) == 0
        ts = timed_in_turn({"any_batch": any_batch, "loop": loop, "stream_batch": stream_batch, "indexed_batch": indexed_batch},
                           args.repeats)
        comp.set_profiling(True)
        any_batch()
        torch.cuda.synchronize()
        rec = comp.last_recover_stats()
        inf = comp.inflate_ms()
        comp.set_profiling(False)
        row = {"item_bytes": item, "items": k, "bytes": n, "ratio": round(n / sum(sn), 4),
               "any_batch": rate(n, ts["any_batch"]),
               "loop": dict(rate(n, ts["loop"], k / kl), items_timed=kl,
                            note="per-item sfh_decompress_any_device; time scaled from the timed subset" if kl < k else "every item"),
               "stream_batch": rate(n, ts["stream_batch"]), "indexed_batch": rate(n, ts["indexed_batch"]),
               "recover": {"scan_ms": round(rec["scan_ms"], 3), "walk_ms": round(rec["walk_ms"], 3), "nodes": int(rec["nodes"]),
                           "rows": int(rec["rows"]), "inflate_ms": {a: round(b, 3) for a, b in inf.items()}}}
        a, b, d = row["any_batch"], row["loop"], row["indexed_batch"]
        row["any_vs_loop"] = round(b["ms"] / a["ms"], 2)
        row["spread_ms"] = round((a["max_ms"] - a["min_ms"]) + (b["max_ms"] - b["min_ms"]), 3)
        row["loop_minus_any_ms"] = round(b["ms"] - a["ms"], 3)
        gap = a["ms"] - d["ms"]
        row["gap_to_indexed_ms"] = round(gap, 3)
        row["recovery_share_of_gap"] = round((rec["scan_ms"] + rec["walk_ms"]) / gap, 3) if gap > 0 else None
        rows.append(row)
        print(json.dumps(row), flush=True)
        del buf, out, d_idx, d_status
        torch.cuda.empty_cache()
    res = {"tool": "any_batch_rate", "device": torch.cuda.get_device_name(0), "total_bytes": args.total, "repeats": args.repeats,
           "source": build.source_stamp(), "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
