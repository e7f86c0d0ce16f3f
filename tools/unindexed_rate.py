"""Decoding without side information, timed: the bench's 1 GiB text stream (synth.gen_text_torch, default options) decoded
three ways -- with the index and sub-index of the compressing call, with the index only, and with the index recovered from
the stream (sfh_decompress_any_device) -- plus the recovery alone (candidate scan and walk separately, HIP events) on that
stream, on a 1 GiB noise stream (32 768 stored segments) and on an adversarial one (stored noise with a flush marker every
300 bytes and a fake stored header every 700).  Rates in MiB/s of decoded output, times in ms, median of --repeats after a
warm-up.

usage: python tools/unindexed_rate.py OUT.json [--bytes N] [--repeats N]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from starflate_amd import Compressor, build, synth  # noqa: E402

MiB = 1 << 20


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


def recovery(comp, stream, n, repeats):
    comp._lib.sfh_set_profiling(comp._h, 1)
    scan, walk = [], []
    for _ in range(repeats + 1):
        comp.recover_index(stream, n)
        s = comp.last_recover_stats()
        scan.append(s["scan_ms"])
        walk.append(s["walk_ms"])
    comp._lib.sfh_set_profiling(comp._h, 0)
    nodes = comp.last_recover_stats()["nodes"]
    return {"scan_ms": statistics.median(scan[1:]), "walk_ms": statistics.median(walk[1:]), "nodes": nodes,
            "recover_wall_ms": timed(lambda: comp.recover_index(stream, n), repeats)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    build.build()
    comp = Compressor(0)
    n = a.bytes
    res = {"bytes": n}

    src = synth.gen_text_torch(n, device="cuda")
    out, m = comp.compress_tensor(src)
    stream = out[:m].clone()
    ix, sub, bb = comp.last_index(device="cuda"), comp.last_subindex(device="cuda"), comp.last_block_bytes()
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    for name, fn in (("subindex", lambda: comp.decompress_tensor(stream, ix, n, dst, subindex=sub, block_bytes=bb)),
                     ("index", lambda: comp.decompress_tensor(stream, ix, n, dst, block_bytes=bb)),
                     ("recovered", lambda: comp.decompress_any_tensor(stream, n, out=dst))):
        ms = timed(fn, a.repeats)
        assert torch.equal(dst, src), name
        res[f"text_{name}_ms"] = ms
        res[f"text_{name}_mib_s"] = n / MiB / (ms / 1e3)
    res["text_rows"] = comp.last_recover_stats()["rows"]
    res["text_recover"] = recovery(comp, stream, n, a.repeats)
    del src, out

    g = torch.Generator(device="cuda").manual_seed(5)
    noise = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    out, m = comp.compress_tensor(noise)
    res["noise_recover"] = recovery(comp, out[:m], n, a.repeats)
    res["noise_recovered_mib_s"] = n / MiB / (timed(lambda: comp.decompress_any_tensor(out[:m], n, out=dst), a.repeats) / 1e3)
    assert torch.equal(dst, noise)
    marks = torch.tensor([0, 0, 255, 255], dtype=torch.uint8, device="cuda")
    fake = torch.tensor([0, 0, 0x80, 0xFF, 0x7F], dtype=torch.uint8, device="cuda")
    at = torch.arange(123, n - 8, 300, device="cuda")
    noise[at[:, None] + torch.arange(4, device="cuda")] = marks
    at = torch.arange(250, n - 8, 700, device="cuda")
    noise[at[:, None] + torch.arange(5, device="cuda")] = fake
    out, m = comp.compress_tensor(noise, strategy="stored")
    res["adversarial_recover"] = recovery(comp, out[:m], n, a.repeats)
    res["adversarial_recovered_mib_s"] = n / MiB / (timed(lambda: comp.decompress_any_tensor(out[:m], n, out=dst), a.repeats) / 1e3)
    assert torch.equal(dst, noise)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
