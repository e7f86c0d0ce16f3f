"""BGZF files of bgzip's 65280-byte members on the decoder's wide rows (sfh_decompress_bgzf_wide_device) against what read them
before and against the narrow rows, on --total bytes of the project's synthetic text and of real bytes
(starflate_amd/realbytes.py: source text, then machine code), resident in HBM.  Device legs: HIP events around a synchronised
call, median, minimum and maximum of --repeats after a warm-up.  Members are made with zlib -6, as bgzip makes them.

  wide      sfh_decompress_bgzf_wide_device on members of 65280 bytes (the member walk included)
  stream    sfh_inflate_stream_batch_device on the same members as items, 16-byte aligned: the decoder such members had before
  narrow    sfh_decompress_bgzf_device on the same bytes in members of 32768: the same kernels on narrow rows, the ceiling
  host      sfh_decompress_bgzf (host buffers, wall clock) on --host-total bytes of text in zlib -1 members of 65280, the file of
            tools/bgzf_rate.py's fallback leg

--parent-root DIR: a tree of another commit, built (the parent's).  `narrow` and `host` are then measured there as well, in a
child process of their own started before this one touches the device, and reported under "parent".

usage: python tools/bgzf_wide_rate.py OUT.json [--total BYTES] [--host-total BYTES] [--repeats N] [--parent-root DIR]"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

MiB = 1 << 20
WIDE, SEG = 65280, 32768


def _root():
    for i, a in enumerate(sys.argv):
        if a == "--package-root":
            return sys.argv[i + 1]
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


ROOT = _root()  # (--package-root: the child of --parent-root measures that tree's package)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from starflate_amd import Compressor, build, realbytes, synth  # noqa: E402


def timed(fn, repeats):
    fn()
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


def member(payload, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(payload) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(body) + 8 - 1) + body +
            struct.pack("<II", zlib.crc32(payload), len(payload)))


EOF = member(b"", 6)


def members_of(data, per, level=6):
    """the BGZF members of `data` cut every `per` bytes (zlib releases the GIL: a pool of threads)"""
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        return list(pool.map(lambda k: member(data[k: k + per], level), range(0, len(data), per)))


def real(total):
    parts = [realbytes.source(), realbytes.binary(total)]
    buf = np.concatenate([p for p in parts if p.size])
    return np.resize(buf, total).tobytes()


def device_legs(comp, name, data, legs, repeats, res):
    L, h = comp._lib, comp._h
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    total = len(data)
    want = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    back = torch.empty(total, dtype=torch.uint8, device="cuda")
    got, st = C.c_uint64(0), C.c_uint32(0)

    def decode(call, blob):
        def fn():
            comp._check(getattr(L, call)(h, blob.data_ptr(), blob.numel(), back.data_ptr(), total, C.byref(got), C.byref(st), s))
        back.zero_()
        t = timed(fn, repeats)
        assert st.value == 0 and got.value == total and torch.equal(back, want), call
        return t

    if "wide" in legs or "stream" in legs:
        parts = members_of(data, WIDE)
        file_bytes = sum(len(p) for p in parts) + len(EOF)
    if "wide" in legs:
        blob = torch.from_numpy(np.frombuffer(b"".join(parts) + EOF, np.uint8).copy()).cuda()
        res[f"{name}_wide"] = dict(rate(total, decode("sfh_decompress_bgzf_wide_device", blob)), members=len(parts) + 1, file_bytes=file_bytes)
        del blob
    if "stream" in legs:
        k = len(parts)
        starts = np.zeros(k + 1, np.int64)
        for i, p in enumerate(parts):
            starts[i + 1] = (starts[i] + len(p) + 15) // 16 * 16
        host = np.zeros(int(starts[-1]) + 16, np.uint8)
        for i, p in enumerate(parts):
            host[starts[i]: starts[i] + len(p)] = np.frombuffer(p, np.uint8)
        packed = torch.from_numpy(host).cuda()
        sp = (C.c_void_p * k)(*[packed.data_ptr() + int(starts[i]) for i in range(k)])
        sn = (C.c_uint64 * k)(*[len(p) for p in parts])
        caps = [min(WIDE, total - i * WIDE) for i in range(k)]
        dp = (C.c_void_p * k)(*[back.data_ptr() + i * WIDE for i in range(k)])
        dn = (C.c_uint64 * k)(*caps)
        out_n, stat = (C.c_uint64 * k)(), (C.c_uint32 * k)()

        def fn():
            comp._check(L.sfh_inflate_stream_batch_device(h, k, sp, sn, 2, dp, dn, out_n, stat, s))

        back.zero_()
        t = timed(fn, repeats)
        assert not any(stat) and list(out_n) == caps and torch.equal(back, want)
        res[f"{name}_stream_batch_items"] = dict(rate(total, t), items=k)
        del packed
    if "narrow" in legs:
        narrow = members_of(data, SEG)
        blob = torch.from_numpy(np.frombuffer(b"".join(narrow) + EOF, np.uint8).copy()).cuda()
        res[f"{name}_narrow"] = dict(rate(total, decode("sfh_decompress_bgzf_device", blob)), members=len(narrow) + 1,
                                     file_bytes=blob.numel())
        del blob
    del want, back
    torch.cuda.empty_cache()


def measure(args, legs):
    comp = Compressor(0)
    res = {}
    if legs & {"wide", "stream", "narrow"}:
        device_legs(comp, "text", synth.gen_text(args.total, seed=3).tobytes(), legs, args.repeats, res)
        device_legs(comp, "real", real(args.total), legs, args.repeats, res)
    if "host" in legs:
        ft = args.host_total
        data = synth.gen_text(ft, seed=5).tobytes()
        big = b"".join(members_of(data, WIDE, level=1)) + member(b"", 1)
        assert comp.decompress_bgzf(big) == (data, 0)
        res["host_text"] = dict(rate(ft, wall(lambda: comp.decompress_bgzf(big), args.repeats)), file_bytes=len(big))
    res["source"] = build.source_stamp()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--total", type=int, default=256 * MiB)
    ap.add_argument("--host-total", type=int, default=64 * MiB)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--package-root", default=None, help="(internal) measure the package of this tree")
    ap.add_argument("--legs", default="wide,stream,narrow,host")
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    res = {"tool": "bgzf_wide_rate", "total_bytes": args.total, "host_total_bytes": args.host_total, "repeats": args.repeats}
    if args.parent_root:
        tmp = args.out + ".parent"
        subprocess.check_call([sys.executable, os.path.abspath(__file__), tmp, "--package-root", os.path.abspath(args.parent_root),
                               "--legs", "narrow,host", "--total", str(args.total), "--host-total", str(args.host_total),
                               "--repeats", str(args.repeats)], env=dict(os.environ, SFH_LIB=""))
        with open(tmp) as f:
            res["parent"] = json.load(f)
        os.remove(tmp)
    res["device"] = torch.cuda.get_device_name(0)
    res.update(measure(args, legs))
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
