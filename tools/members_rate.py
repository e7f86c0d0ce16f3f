"""Files of gzip members, timed (sfh_inflate_stream_device with SFH_GZIP_MEMBERS) on one GPU.  Seeded text, zlib -6 members made
on the host:

  (a) --bytes-a (256 MiB) in members of 64 KiB   (b) --bytes-b (64 MiB) in members of 1 KiB, WARC-like

each decoded three ways: the joined file as container="gzip_members"; the same members as the items of one
decompress_stream_batch_tensors call, their boundaries given (what a caller had to do before); and the same data as one member,
container="gzip".  (c): that single-member file under container="gzip_members" as well.  Every leg: device-event time around the
call with the profiler off, after a warm-up call, repeated until the standard error of the mean is below 1 % (5 to 15 repeats);
mean, standard deviation, extremes and repeats are recorded, and MiB/s of output from the mean.  --stream-runs label=FILE ...
embeds tools/stream_inflate_rate.py results (the unchanged single-member path on two builds of the library, run alternately)
under "unchanged_path".  Fails without a GPU.

usage: python tools/members_rate.py OUT.json [--bytes-a N] [--bytes-b N] [--stream-runs label=FILE ...]"""
import argparse
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
HEAD = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"


def member(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return HEAD + c.compress(data) + c.flush() + zlib.crc32(data).to_bytes(4, "little") + (len(data) & 0xFFFFFFFF).to_bytes(4, "little")


def timed(fn, n):
    """fn() warmed up once, then timed by device events -> the leg's record (n: output bytes)"""
    fn()
    torch.cuda.synchronize()
    ts = []
    while len(ts) < 15:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
        if len(ts) >= 5 and statistics.stdev(ts) / len(ts) ** 0.5 < 0.01 * statistics.mean(ts):
            break
    mean = statistics.mean(ts)
    return {"mean_ms": mean, "stdev_ms": statistics.stdev(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": len(ts),
            "mib_s": n / MiB / (mean / 1e3)}


def dev(b):
    return torch.from_numpy(np.frombuffer(b + bytes(-len(b) % 16), np.uint8).copy()).cuda()


def case(comp, data, size, single=None):
    """data in members of `size` bytes -> the three legs (single: the one-member file, made once per data)"""
    n = len(data)
    parts = [member(data[i: i + size]) for i in range(0, n, size)]
    want = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    res = {"bytes": n, "member_bytes": size, "members": len(parts), "file_bytes": sum(len(p) for p in parts)}
    # the joined file
    blob = b"".join(parts)
    t = dev(blob)[: len(blob)]

    def run_members():
        _, st = comp.decompress_stream_tensor(t, n, "gzip_members", out=out)
        assert st == 0

    res["gzip_members"] = timed(run_members, n)
    assert torch.equal(out, want)
    res["gzip_members"]["stats"] = {k: v for k, v in comp.last_stream_stats().items() if not k.endswith("_ms")}
    out.zero_()
    # the members as items, boundaries given: every item at a 16-byte aligned place of one buffer
    offs, at = [], 0
    for p in parts:
        offs.append(at)
        at += len(p) + (-len(p) % 16)
    packed = dev(b"".join(p + bytes(-len(p) % 16) for p in parts))
    srcs = [packed[o: o + len(p)] for o, p in zip(offs, parts)]
    sizes = [min(size, n - i) for i in range(0, n, size)]
    outs = [out[i: i + s] for i, s in zip(range(0, n, size), sizes)]

    def run_items():
        _, sts = comp.decompress_stream_batch_tensors(srcs, sizes, "gzip", outs=outs)
        assert not any(sts)

    res["items_boundaries_given"] = timed(run_items, n)
    assert torch.equal(out, want)
    out.zero_()
    del packed, srcs
    # one member
    single = member(data) if single is None else single
    s = dev(single)[: len(single)]

    def run_single():
        _, st = comp.decompress_stream_tensor(s, n, "gzip", out=out)
        assert st == 0

    res["one_member_gzip"] = timed(run_single, n)
    assert torch.equal(out, want)
    return res, single


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--bytes-a", type=int, default=256 << 20)
    ap.add_argument("--bytes-b", type=int, default=64 << 20)
    ap.add_argument("--stream-runs", nargs="*", default=[])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("members_rate: no GPU")
    build.build()
    comp = Compressor(0)
    res = {"source": build.source_stamp(), "device": torch.cuda.get_device_name(0)}
    data = synth.gen_text(a.bytes_a, seed=1).tobytes()
    res["a_64k_members"], single = case(comp, data, 65536)
    # (c) the single-member file under both container values
    n = len(data)
    s = dev(single)[: len(single)]
    out = torch.empty(n, dtype=torch.uint8, device="cuda")

    def run_c():
        _, st = comp.decompress_stream_tensor(s, n, "gzip_members", out=out)
        assert st == 0

    res["c_single_member_file"] = {"bytes": n, "gzip": res["a_64k_members"]["one_member_gzip"], "gzip_members": timed(run_c, n)}
    del s, out
    res["b_1k_members"], _ = case(comp, data[: a.bytes_b], 1024)
    runs = {}
    for item in a.stream_runs:
        label, path = item.split("=", 1)
        with open(path) as f:
            r = json.load(f)
        runs[label] = {k: r[k] for k in ("bytes", "raw_ms", "zlib_ms", "gzip_ms", "raw_mib_s", "zlib_mib_s", "gzip_mib_s") if k in r}
        for leg in ("stored_deflate", "level0_noise", "level6_noise", "mixed6"):
            if leg in r:
                runs[label][leg + "_ms"] = r[leg]["ms"]
    if runs:
        res["unchanged_path"] = runs
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
