"""Batches of streams without flush points, timed (sfh_inflate_stream_batch_device): --bytes of synthetic text cut into items
of 64 KiB, 256 KiB (as gzip), 1 MiB and log-uniform 1 KiB .. 4 MiB, each item compressed by zlib -6 on the host, decoded on one
GPU.  Per item size: the median MiB/s of output of the batch call over --repeats after a warm-up; a per-item
sfh_inflate_stream_device loop timed on a prefix of --loop-items items (reported per item and as MiB/s); one stream holding
the same bytes (zlib -6 of the whole text); the batch call's stage times, chunk counts, repair rounds and scratch.  For 32 KiB
items also sfh_decompress_batch without an index (the indexed batch decoder's index-free form) against the stream batch.

usage: python tools/stream_batch_rate.py OUT.json [--bytes N] [--repeats N] [--loop-items N]"""
import argparse
import concurrent.futures as cf
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
WBITS = {"zlib": 15, "gzip": 31}


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def cut(n, kind, rng):
    if kind == "loguniform":
        sizes = []
        while sum(sizes) < n:
            sizes.append(int(np.exp(rng.uniform(np.log(1024), np.log(4 * MiB)))))
        sizes[-1] -= sum(sizes) - n
        return [s for s in sizes if s > 0]
    return [kind] * (n // kind)


def compress_all(pieces, container, pool):
    def one(p):
        c = zlib.compressobj(6, zlib.DEFLATED, WBITS[container])
        return c.compress(p) + c.flush()
    return list(pool.map(one, pieces))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-items", type=int, default=200)
    a = ap.parse_args()
    build.build()
    comp = Compressor(0)
    data = synth.gen_text(a.bytes, seed=1).tobytes()
    rng = np.random.default_rng(7)
    pool = cf.ThreadPoolExecutor(16)  # (zlib releases the GIL)
    res = {"bytes": a.bytes, "repeats": a.repeats, "loop_items": a.loop_items, "sizes": {}}
    # one stream holding the same bytes
    whole = compress_all([data], "zlib", pool)[0]
    t_whole = torch.from_numpy(np.frombuffer(whole, np.uint8).copy()).cuda()
    out_whole = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    ms_one = timed(lambda: comp.decompress_stream_tensor(t_whole, len(data), "zlib", out=out_whole), a.repeats)
    res["one_stream"] = {"ms": ms_one, "MiBps": a.bytes / MiB / (ms_one / 1e3), "stats": comp.last_stream_stats()}
    del t_whole, out_whole
    print(f"one stream: {res['one_stream']['MiBps']:.0f} MiB/s", flush=True)
    for kind, label, container in ((64 << 10, "64KiB", "zlib"), (256 << 10, "256KiB", "gzip"), (MiB, "1MiB", "zlib"),
                                   ("loguniform", "1KiB-4MiB", "zlib"), (32 << 10, "32KiB", "zlib")):
        sizes = cut(a.bytes, kind, rng)
        offs = np.concatenate([[0], np.cumsum(sizes)])
        pieces = [data[offs[i]: offs[i + 1]] for i in range(len(sizes))]
        streams = compress_all(pieces, container, pool)
        srcs = [torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda() for s in streams]
        outs = [torch.empty(max(n, 1), dtype=torch.uint8, device="cuda") for n in sizes]
        total = int(offs[-1])

        def batch():
            o, st = comp.decompress_stream_batch_tensors(srcs, sizes, container, outs=outs)
            assert all(v == 0 for v in st), st

        ms = timed(batch, a.repeats)
        comp.set_profiling(True)
        batch()
        stats = comp.last_stream_stats()
        comp.set_profiling(False)
        k = min(a.loop_items, len(srcs))

        def loop():
            for i in range(k):
                o, st = comp.decompress_stream_tensor(srcs[i], sizes[i], container, out=outs[i])
                assert st == 0

        ms_loop = timed(loop, max(1, a.repeats // 2))
        loop_bytes = int(offs[k])
        r = {"items": len(sizes), "container": container, "ms": ms, "MiBps": total / MiB / (ms / 1e3),
             "loop_ms_per_item": ms_loop / k, "loop_MiBps": loop_bytes / MiB / (ms_loop / 1e3), "stats": stats}
        r["batch_over_loop"] = r["MiBps"] / r["loop_MiBps"]
        r["batch_over_one_stream"] = r["MiBps"] / res["one_stream"]["MiBps"]
        if kind == 32 << 10:  # the indexed batch decoder without an index: every item one 32 KiB segment
            status = [None]

            def indexed():
                o, st = comp.decompress_batch_tensors(srcs, sizes, container=container, outs=outs)
                status[0] = st

            ms_ix = timed(indexed, a.repeats)
            assert int(status[0].abs().sum()) == 0
            r["decompress_batch_ms"] = ms_ix
            r["decompress_batch_MiBps"] = total / MiB / (ms_ix / 1e3)
        res["sizes"][label] = r
        print(f"{label}: batch {r['MiBps']:.0f} MiB/s, loop {r['loop_MiBps']:.0f} MiB/s ({r['loop_ms_per_item']:.3f} ms/item), "
              f"x{r['batch_over_loop']:.1f} the loop, x{r['batch_over_one_stream']:.2f} one stream", flush=True)
        del srcs, outs
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
