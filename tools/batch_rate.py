"""Batched compression against a per-item loop and one large call (device buffers, HIP events around a synchronised
call, median of --repeats after a warm-up).  For items of 4 KiB, 64 KiB and 1 MiB of synthetic text (--total bytes in all):

  batch   one sfh_compress_batch_device_async over every item
  loop    sfh_compress_device once per item (a timed subset when the loop would be slow: `items_timed` says how many)
  single  one sfh_compress_device over the concatenation with block_bytes = 32768 -- the per-byte reference (for
          64 KiB items the batch does the same strip work)

usage: python tools/batch_rate.py OUT.json [--total BYTES] [--repeats N] [--loop-items N]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from starflate_amd import Compressor, _capi, build, synth  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--total", type=int, default=1 << 30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-items", type=int, default=2048, help="items the per-item loop times at most")
    args = ap.parse_args()
    comp = Compressor(0)
    text = synth.gen_text_torch(args.total, seed=3)
    torch.cuda.synchronize()
    rows = []
    for item in (4096, 65536, MiB):
        k = args.total // item
        cap = comp.compress_bound(item)
        arena = torch.empty(k * cap, dtype=torch.uint8, device="cuda")  # item i's stream at i * cap
        sizes = torch.empty(k, dtype=torch.int64, device="cuda")
        # the host arrays are built once: the timed call is the C-ABI call itself
        sp = (C.c_void_p * k)(*[text.data_ptr() + i * item for i in range(k)])
        dp = (C.c_void_p * k)(*[arena.data_ptr() + i * cap for i in range(k)])
        nn, cc = (C.c_uint64 * k)(*([item] * k)), (C.c_uint64 * k)(*([cap] * k))
        opt = _capi.make_options()
        s = torch.cuda.current_stream().cuda_stream
        L, h = comp._lib, comp._h

        def batch():
            comp._check(L.sfh_compress_batch_device_async(h, k, sp, nn, dp, cc, C.c_void_p(sizes.data_ptr()), C.byref(opt), C.c_void_p(s)))

        ms_b = timed(batch, args.repeats)
        out_b = int(sizes.sum())
        box = {}
        srcs = [text[i * item:(i + 1) * item] for i in range(min(k, args.loop_items))]
        outs = [arena[i * cap:(i + 1) * cap] for i in range(len(srcs))]
        kl = min(k, args.loop_items)

        def loop():
            for i in range(kl):
                comp.compress_tensor(srcs[i], outs[i])

        ms_l = timed(loop, args.repeats) * k / kl
        flat = text[: k * item]
        one = torch.empty(comp.compress_bound(flat.numel()), dtype=torch.uint8, device="cuda")

        def single():
            box["n"] = comp.compress_tensor(flat, one, block_bytes=32768)[1]

        ms_s = timed(single, args.repeats)
        n = k * item
        row = {"item_bytes": item, "items": k, "bytes": n,
               "batch": {"ms": round(ms_b, 3), "MiB_s": round(n / MiB / (ms_b / 1e3), 1), "ratio": round(n / out_b, 4)},
               "loop": {"ms": round(ms_l, 3), "MiB_s": round(n / MiB / (ms_l / 1e3), 1), "items_timed": kl,
                        "note": "per-item sfh_compress_device; time scaled from the timed subset" if kl < k else "every item"},
               "single_32k": {"ms": round(ms_s, 3), "MiB_s": round(n / MiB / (ms_s / 1e3), 1), "ratio": round(n / box["n"], 4)}}
        row["batch_vs_single"] = round(row["batch"]["MiB_s"] / row["single_32k"]["MiB_s"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del srcs, outs, one, arena
        torch.cuda.empty_cache()
    res = {"tool": "batch_rate", "device": torch.cuda.get_device_name(0), "total_bytes": args.total, "repeats": args.repeats,
           "source": build.source_stamp(), "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
