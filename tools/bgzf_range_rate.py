"""BGZF random access (sfh_decompress_bgzf_ranges_device) on --total bytes of the project's synthetic text as a BGZF file, in
members of 65280 bytes (bgzip's) and in members of 32768 (the library's writer's), resident in HBM, the index found once by
sfh_bgzf_read_index_device.  HIP events around a synchronised call, median, minimum and maximum of --repeats after a warm-up.
Members are made with zlib -6, as bgzip makes them.

  whole     sfh_decompress_bgzf_wide_device on the file: every member, CRC-32 verified (the member walk included)
  members   the range call with ranges that are exactly the members: the token and byte work of `whole`, minus the checksum, plus
            the planner.  Its median must not exceed `whole`'s by more than the larger of the two legs' own relative spreads
            ((max - min) / median): "members_within_margin"
  mixes     4 KiB x 16384, 64 KiB x 4096 and 1024 KiB x 256 random ranges into one packed buffer: the range call, and next to it
            sfh_decompress_ranges_device_async for the same ranges of the same bytes as a raw stream indexed every 32 KiB
            (block_bytes = 32768: a range costs the segments it touches, as it costs the members it touches here)

usage: python tools/bgzf_range_rate.py OUT.json [--total BYTES] [--repeats N]"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import zlib
from concurrent.futures import ThreadPoolExecutor

MiB = 1 << 20
SEG = 32768
MIXES = ((4096, 16384), (65536, 4096), (1024 * 1024, 256))

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from starflate_amd import Compressor, _capi, build, synth  # noqa: E402


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


def rate(n, t):
    ms, lo, hi = t
    return {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "spread": round((hi - lo) / ms, 4),
            "MiB_s": round(n / MiB / (ms / 1e3), 1)}


def member(payload, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(payload) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(body) + 8 - 1) + body +
            struct.pack("<II", zlib.crc32(payload), len(payload)))


def bgzf_file(data, per):
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        parts = list(pool.map(lambda k: member(data[k: k + per]), range(0, len(data), per)))
    return b"".join(parts) + member(b"")


def packed(lens, buf):
    at = np.concatenate([[0], np.cumsum(lens)])
    return (C.c_void_p * len(lens))(*[buf.data_ptr() + int(a) for a in at[:-1]]), at


def check_packed(buf, at, want, offs, lens, every):
    for r in range(0, len(offs), every):
        assert torch.equal(buf[int(at[r]): int(at[r]) + lens[r]], want[offs[r]: offs[r] + lens[r]]), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--total", type=int, default=256 * MiB)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    total, repeats = args.total, args.repeats
    comp = Compressor(0)
    L, h = comp._lib, comp._h
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    data = synth.gen_text(total, seed=3).tobytes()
    want = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    back = torch.empty(total, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(7)
    mixes = []
    for ln, k in MIXES:
        k = max(1, min(k, total // ln))
        mixes.append(([int(v) for v in rng.integers(0, total - ln + 1, k)], [ln] * k))
    res = {"tool": "bgzf_range_rate", "total_bytes": total, "repeats": repeats, "device": torch.cuda.get_device_name(0)}

    # the same bytes as a raw stream indexed every 32 KiB
    stream, n = comp.compress_tensor(want, block_bytes=SEG)
    stream = stream[:n].clone()
    index = comp.last_index(device=want.device)
    nseg = index.numel() - 1
    for offs, lens in mixes:
        k = len(offs)
        dp, at = packed(lens, back)
        status = torch.zeros(k, dtype=torch.int32, device="cuda")
        co, cl = (C.c_uint64 * k)(*offs), (C.c_uint64 * k)(*lens)

        def fn():
            comp._check(L.sfh_decompress_ranges_device_async(h, stream.data_ptr(), stream.numel(), index.data_ptr(), None, nseg, total, SEG,
                                                             k, co, cl, dp, status.data_ptr(), s))
        t = timed(fn, repeats)
        assert not bool(status.any())
        check_packed(back, at, want, offs, lens, max(1, k // 64))
        res[f"indexed_{lens[0] // 1024}KiB_x{k}"] = rate(sum(lens), t)
    del stream, index

    for per in (65280, SEG):
        blob = torch.from_numpy(np.frombuffer(bgzf_file(data, per), np.uint8).copy()).cuda()
        moff, ooff, info = comp.bgzf_index_tensor(blob)
        binfo = _capi.BgzfInfo(info["total_n"], info["members"], info["max_isize"], int(info["has_eof"]), 0)
        got, st = C.c_uint64(0), C.c_uint32(0)
        leg = {"members": info["members"], "file_bytes": blob.numel()}

        def whole():
            comp._check(L.sfh_decompress_bgzf_wide_device(h, blob.data_ptr(), blob.numel(), back.data_ptr(), total, C.byref(got), C.byref(st), s))

        def ranges_fn(offs, lens):
            k = len(offs)
            dp, at = packed(lens, back)
            status = torch.zeros(k, dtype=torch.int32, device="cuda")
            co, cl = (C.c_uint64 * k)(*offs), (C.c_uint64 * k)(*lens)

            def fn():
                comp._check(L.sfh_decompress_bgzf_ranges_device(h, blob.data_ptr(), blob.numel(), moff.data_ptr(), ooff.data_ptr(),
                                                                C.byref(binfo), k, co, cl, dp, status.data_ptr(), s))
            return fn, status, at

        # `whole` and `members` in turn, twice: the two legs of the margin see the same machine
        oo = [int(v) for v in ooff.cpu().numpy()]
        m_offs = [a for a, b in zip(oo, oo[1:]) if b > a]
        m_lens = [b - a for a, b in zip(oo, oo[1:]) if b > a]
        fn, status, at = ranges_fn(m_offs, m_lens)
        back.zero_()
        t_whole = timed(whole, repeats)
        assert st.value == 0 and got.value == total and torch.equal(back, want)
        back.zero_()
        t_members = timed(fn, repeats)
        assert not bool(status.any()) and torch.equal(back, want)
        leg["whole"] = rate(total, t_whole)
        leg["members_as_ranges"] = dict(rate(total, t_members), ranges=len(m_offs))
        margin = max(leg["whole"]["spread"], leg["members_as_ranges"]["spread"])
        leg["members_margin"] = margin
        leg["members_over_whole"] = round(t_members[0] / t_whole[0], 4)
        leg["members_within_margin"] = bool(t_members[0] <= t_whole[0] * (1 + margin))
        for offs, lens in mixes:
            fn, status, at = ranges_fn(offs, lens)
            t = timed(fn, repeats)
            assert not bool(status.any())
            check_packed(back, at, want, offs, lens, max(1, len(offs) // 64))
            leg[f"ranges_{lens[0] // 1024}KiB_x{len(offs)}"] = rate(sum(lens), t)
        res[f"members_{per}"] = leg
        del blob, moff, ooff
    res["source"] = build.source_stamp()
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
