"""Seekable gzip (SFH_DICTZIP) against what it replaces, on --total bytes of synthetic text resident in HBM (device buffers,
HIP events around a synchronised call, median and spread of --repeats after a warm-up):

  index     sfh_dz_read_index_device (the table in the file's own header) against sfh_recover_index_device (a scan of the
            whole stream for its flush markers) on the same file
  decode    sfh_decompress_dz_device against sfh_decompress_any_device, both verifying the gzip wrapper and the CRC-32
  compress  sfh_compress_device_async with SFH_DICTZIP against SFH_GZIP, both at block_bytes = 32768: the table costs the
            stores of two bytes per 32 KiB of input (the checksum + wrapper stage is reported by itself as well)

usage: python tools/dictzip_rate.py OUT.json [--total BYTES] [--repeats N]"""
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
    return {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "MiB_s": round(n / MiB / (ms / 1e3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--total", type=int, default=256 * MiB)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    comp = Compressor(0)
    L, h = comp._lib, comp._h
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    total = args.total
    nseg = max(1, -(-total // SEG))
    flat = synth.gen_text_torch(total, seed=3)
    out = torch.empty(L.sfh_compress_bound_container(total, SEG, _capi.COMPRESS_CONTAINER["dictzip"]), dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int64, device="cuda")

    # compress: both containers at block_bytes = 32768, the stage times of one profiled call each
    res = {}
    files = {}
    for container in ("gzip", "dictzip"):
        t = timed(lambda: comp.compress_tensor_async(flat, out, size, container=container, block_bytes=SEG), args.repeats)
        n = int(size.item())
        files[container] = out[:n].clone()
        comp.set_profiling(True)
        comp.compress_tensor_async(flat, out, size, container=container, block_bytes=SEG)
        torch.cuda.synchronize()
        stages = comp.stage_ms()
        comp.set_profiling(False)
        res[f"compress_{container}"] = dict(rate(total, t), stream_bytes=n, stage_ms={k: round(v, 4) for k, v in stages.items()})
    hdr = L.sfh_dz_header_bytes(total)
    assert torch.equal(files["dictzip"][hdr:], files["gzip"][10:]), "the bodies differ"
    res["compress_dictzip_over_gzip"] = round(res["compress_dictzip"]["ms"] / res["compress_gzip"]["ms"], 4)
    res["header_bytes"] = hdr
    del out
    torch.cuda.empty_cache()

    # index: the table against the scan, on the dictzip file
    stream = files["dictzip"]
    idx_dz = torch.empty(nseg + 1, dtype=torch.int64, device="cuda")
    idx_rec = torch.empty(nseg + 1, dtype=torch.int64, device="cuda")
    info = _capi.DzInfo()

    def read_index():
        comp._check(L.sfh_dz_read_index_device(h, stream.data_ptr(), stream.numel(), C.byref(info), idx_dz.data_ptr(), nseg + 1, s))

    def recover_index():
        comp._check(L.sfh_recover_index_device(h, stream.data_ptr(), stream.numel(), 2, total, idx_rec.data_ptr(), nseg, None, s))

    t_dz = timed(read_index, args.repeats)
    t_rec = timed(recover_index, args.repeats)
    assert (info.total_n, info.nseg, info.status) == (total, nseg, 0) and torch.equal(idx_dz, idx_rec)
    res["index_dz_read"] = rate(total, t_dz)
    res["index_recover"] = rate(total, t_rec)
    res["index_recover_over_dz_read"] = round(t_rec[0] / t_dz[0], 2)

    # decode: the file's own table against the recovered index
    back = torch.empty(total, dtype=torch.uint8, device="cuda")
    got, st = C.c_uint64(0), C.c_uint32(0)

    def decode_dz():
        comp._check(L.sfh_decompress_dz_device(h, stream.data_ptr(), stream.numel(), back.data_ptr(), total, C.byref(got), C.byref(st), s))

    def decode_any():
        comp._check(L.sfh_decompress_any_device(h, stream.data_ptr(), stream.numel(), 2, back.data_ptr(), total, C.byref(st), s))

    back.zero_()
    t_ddz = timed(decode_dz, args.repeats)
    assert st.value == 0 and got.value == total and torch.equal(back, flat)
    back.zero_()
    t_any = timed(decode_any, args.repeats)
    assert st.value == 0 and torch.equal(back, flat)
    res["decode_dz"] = rate(total, t_ddz)
    res["decode_any"] = rate(total, t_any)
    res["decode_any_over_dz"] = round(t_any[0] / t_ddz[0], 3)

    res = dict({"tool": "dictzip_rate", "device": torch.cuda.get_device_name(0), "total_bytes": total, "segments": nseg,
                "repeats": args.repeats, "source": build.source_stamp(), "ratio": round(total / stream.numel(), 4)}, **res)
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
