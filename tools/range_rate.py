"""Random access against the whole-stream decoders (device buffers, HIP events around a synchronised call, median and spread
of --repeats after a warm-up).  --total bytes of synthetic text, resident in HBM, compressed with block_bytes = 32768 and with
the default strip size; for each, batches of random byte ranges (any offset) of 4 KiB, 64 KiB and 1 MiB, delivered packed back
to back, rates in MiB/s:

  ranges / ranges_sub   one sfh_decompress_ranges_device_async over every range, with the index / with the sub-index as well:
                        `delivered` counts the bytes of the ranges, `span` the bytes of the segments in their decode spans
                        (what the token and byte stages walked)
  batch / batch_sub     sfh_decompress_batch_device_async over as many single-segment items as the decode spans hold
                        segments -- the same segment numbers, taken from the block_bytes = 32768 stream, each written whole to
                        a 32 KiB slot: the existing path doing the same token and byte work without clipping
  full / full_sub       sfh_decompress_device of the whole stream

usage: python tools/range_rate.py OUT.json [--total BYTES] [--repeats N] [--deliver BYTES]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from starflate_amd import Compressor, build, synth  # noqa: E402

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


def rate(n, t):
    ms, lo, hi = t
    return {"ms": round(ms, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "MiB_s": round(n / MiB / (ms / 1e3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--total", type=int, default=1 << 30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--deliver", type=int, default=256 * MiB, help="bytes a batch of ranges delivers at most (4 KiB ranges: a quarter)")
    args = ap.parse_args()
    comp = Compressor(0)
    L, h = comp._lib, comp._h
    s = torch.cuda.current_stream().cuda_stream
    total = args.total
    flat = synth.gen_text_torch(total, seed=3)
    nseg = max(1, -(-total // SEG))
    streams = {}
    for bb in (32768, 0):
        st, n = comp.compress_tensor(flat, block_bytes=bb)
        streams[bb] = dict(stream=st[:n].clone(), idx=comp.last_index(device="cuda"), sub=comp.last_subindex(device="cuda").reshape(-1),
                           bb=comp.last_block_bytes(), ratio=round(total / n, 4))
        del st
    torch.cuda.empty_cache()
    s32 = streams[32768]
    idx32 = s32["idx"].cpu().numpy().astype(np.uint64)
    slots = torch.empty(0, dtype=torch.uint8, device="cuda")
    rows = []
    for bb_asked in (32768, 0):
        S = streams[bb_asked]
        bb, sps = S["bb"], S["bb"] // SEG
        out_full = torch.empty(total, dtype=torch.uint8, device="cuda")
        full = timed(lambda: comp.decompress_tensor(S["stream"], S["idx"], total, out=out_full, block_bytes=bb), args.repeats)
        assert torch.equal(out_full, flat)
        full_sub = timed(lambda: comp.decompress_tensor(S["stream"], S["idx"], total, out=out_full, block_bytes=bb, subindex=S["sub"]),
                         args.repeats)
        del out_full
        torch.cuda.empty_cache()
        for size in (4096, 65536, MiB):
            k = max(1, min(args.deliver // (4 if size == 4096 else 1), total // 2) // size)
            rng = np.random.default_rng(size + bb)
            offs = rng.integers(0, total - size + 1, k).astype(np.uint64)
            first = offs // SEG // sps * sps
            last = (offs + np.uint64(size - 1)) // SEG
            span_segs = int((last - first + 1).sum())
            delivered = k * size
            out = torch.empty(delivered + 3, dtype=torch.uint8, device="cuda")
            status = torch.empty(k, dtype=torch.int32, device="cuda")
            co, cl = (C.c_uint64 * k)(*offs.tolist()), (C.c_uint64 * k)(*([size] * k))
            dp = (C.c_void_p * k)(*[out.data_ptr() + 3 + i * size for i in range(k)])  # packed, at odd addresses

            def ranges(sub_ptr):
                comp._check(L.sfh_decompress_ranges_device_async(h, S["stream"].data_ptr(), S["stream"].numel(), S["idx"].data_ptr(),
                                                                 sub_ptr, nseg, total, bb, k, co, cl, dp,
                                                                 C.c_void_p(status.data_ptr()), C.c_void_p(s)))

            t_r = timed(lambda: ranges(None), args.repeats)
            assert int(status.abs().sum()) == 0
            for i in range(0, k, max(1, k // 64)):
                o = int(offs[i])
                assert torch.equal(out[3 + i * size: 3 + (i + 1) * size], flat[o: o + size]), (bb, size, i)
            scratch = comp.last_decode_scratch_bytes()
            t_rs = timed(lambda: ranges(S["sub"].data_ptr()), args.repeats)
            assert int(status.abs().sum()) == 0
            # the same number of single-segment items through the batch decoder: the spans' segment numbers in the 32 KiB-strip stream
            segs = np.concatenate([np.arange(a, b + 1, dtype=np.int64) for a, b in zip(first.tolist(), last.tolist())])
            m = segs.size
            assert m == span_segs
            if slots.numel() < m * SEG:
                del slots
                torch.cuda.empty_cache()
                slots = torch.empty(m * SEG, dtype=torch.uint8, device="cuda")
            pairs = np.empty(2 * m, np.uint64)
            pairs[0::2], pairs[1::2] = idx32[segs], idx32[segs + 1]
            d_pairs = torch.from_numpy(pairs.astype(np.int64)).cuda()
            d_bsub = s32["sub"].reshape(-1, 64)[torch.from_numpy(segs).cuda()].contiguous().reshape(-1)
            bstatus = torch.empty(m, dtype=torch.int32, device="cuda")
            src_n = s32["stream"].numel()
            sp = (C.c_void_p * m)(*([s32["stream"].data_ptr()] * m))
            bdp = (C.c_void_p * m)(*[slots.data_ptr() + i * SEG for i in range(m)])
            sizes = np.minimum(SEG, total - segs * SEG).astype(np.uint64)
            nn, dn = (C.c_uint64 * m)(*([src_n] * m)), (C.c_uint64 * m)(*sizes.tolist())

            def batch(sub_ptr):
                comp._check(L.sfh_decompress_batch_device_async(h, m, sp, nn, C.c_void_p(d_pairs.data_ptr()), sub_ptr, bdp, dn, None, 0,
                                                                C.c_void_p(bstatus.data_ptr()), C.c_void_p(s)))

            t_b = timed(lambda: batch(None), args.repeats)
            assert int(bstatus.abs().sum()) == 0
            g = int(segs[m // 2])
            assert torch.equal(slots[(m // 2) * SEG: (m // 2) * SEG + int(sizes[m // 2])], flat[g * SEG: g * SEG + int(sizes[m // 2])])
            t_bs = timed(lambda: batch(C.c_void_p(d_bsub.data_ptr())), args.repeats)
            assert int(bstatus.abs().sum()) == 0
            span_bytes = int(sizes.sum())
            row = {"block_bytes": bb, "range_bytes": size, "ranges": k, "delivered_bytes": delivered, "span_segments": span_segs,
                   "span_bytes": span_bytes, "token_scratch_bytes": scratch,
                   "ranges_delivered": rate(delivered, t_r), "ranges_span": rate(span_bytes, t_r),
                   "ranges_sub_delivered": rate(delivered, t_rs), "ranges_sub_span": rate(span_bytes, t_rs),
                   "batch_single_segment_items": dict(rate(span_bytes, t_b), items=m),
                   "batch_sub_single_segment_items": dict(rate(span_bytes, t_bs), items=m),
                   "full": rate(total, full), "full_sub": rate(total, full_sub)}
            row["ranges_vs_batch"] = round(t_b[0] / t_r[0], 3)          # > 1: the range call is the faster one
            row["ranges_sub_vs_batch_sub"] = round(t_bs[0] / t_rs[0], 3)
            row["delivered_over_span"] = round(delivered / span_bytes, 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del out, status, d_pairs, d_bsub, bstatus
            torch.cuda.empty_cache()
    res = {"tool": "range_rate", "device": torch.cuda.get_device_name(0), "total_bytes": total, "repeats": args.repeats,
           "source": build.source_stamp(), "ratio": {str(v["bb"]): v["ratio"] for v in streams.values()}, "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
