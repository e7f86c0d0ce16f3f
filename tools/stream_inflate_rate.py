"""Streams without flush points, timed (sfh_inflate_stream_device): --bytes of synthetic text compressed by zlib -6 on the host
(raw, zlib and gzip wrappers of the same body), decoded on one GPU.  Reports the median MiB/s of output over --repeats after a
warm-up, the per-stage ms (HIP events, profiling on), chunks / candidates / confirmed / repair rounds / scratch; and for
comparison the serial decoder on one core (the oracle's sfo_decompress, zlib's inflate and container.hpp's decompress(), sampled
on a --sample byte prefix stream) and decompress_any on a Z_SYNC_FLUSH-every-32-KiB stream of the same data; and the repair
worst case, stored blocks full of DEFLATE data (--stored-bytes of the text as zlib -6 streams, packed again by zlib -6); and
three legs of --stored-leg-bytes each whose streams are made of stored blocks: level0_noise (zlib -0 of noise, blocks of 65535
bytes), level6_noise (zlib -6 of noise, which stores it in blocks of about 16 KiB) and mixed6 (zlib -6 of alternating 1 MiB
pieces of text and noise), each with its stage ms.  All inputs are seeded.

usage: python tools/stream_inflate_rate.py OUT.json [--bytes N] [--repeats N] [--sample N] [--stored-bytes N]
                                                    [--stored-leg-bytes N]"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
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


def zlib_flushed(data, every=32768):
    c = zlib.compressobj(6, zlib.DEFLATED, 15)
    out = [c.compress(data[k:k + every]) + c.flush(zlib.Z_SYNC_FLUSH) for k in range(0, len(data), every)]
    return b"".join(out) + c.flush()


def stored_leg(comp, plain, level, repeats):
    """zlib -`level` of `plain`, decoded: bytes, median ms and MiB/s, the chunk counts, and the stage ms of a profiled pass"""
    m = len(plain)
    st = torch.from_numpy(np.frombuffer(zlib.compress(plain, level), np.uint8).copy()).cuda()
    out = torch.empty(m, dtype=torch.uint8, device="cuda")
    ms = timed(lambda: comp.decompress_stream_tensor(st, m, "zlib", out=out), repeats)
    _, status = comp.decompress_stream_tensor(st, m, "zlib", out=out)
    assert status == 0 and out.cpu().numpy().tobytes() == plain
    s = comp.last_stream_stats()
    leg = {"bytes": m, "stream_bytes": st.numel(), "ms": ms, "mib_s": m / MiB / (ms / 1e3),
           **{q: s[q] for q in ("chunks", "candidates", "confirmed", "repair_rounds", "longest_chunk")}}
    comp.set_profiling(True)
    stages = []
    for _ in range(repeats):
        comp.decompress_stream_tensor(st, m, "zlib", out=out)
        stages.append(comp.last_stream_stats())
    comp.set_profiling(False)
    leg.update({q: statistics.median(x[q] for x in stages) for q in stages[0] if q.endswith("_ms")})
    return leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=32 << 20)
    ap.add_argument("--stored-bytes", type=int, default=256 << 20)
    ap.add_argument("--stored-leg-bytes", type=int, default=256 << 20)
    a = ap.parse_args()
    build.build()
    comp = Compressor(0)
    n = a.bytes
    data = synth.gen_text(n, seed=1).tobytes()
    res = {"bytes": n}
    t0 = time.perf_counter()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    res["host_zlib6_compress_s"] = time.perf_counter() - t0
    res["stream_bytes"] = len(body)
    want = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    wraps = {"raw": body, "zlib": b"\x78\x9c" + body + zlib.adler32(data).to_bytes(4, "big"),
             "gzip": b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + body + (zlib.crc32(data).to_bytes(4, "little")
                                                                           + (n & 0xFFFFFFFF).to_bytes(4, "little"))}
    for name, stream in wraps.items():
        t = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
        ms = timed(lambda: comp.decompress_stream_tensor(t, n, name, out=dst), a.repeats)
        out, st = comp.decompress_stream_tensor(t, n, name, out=dst)
        assert st == 0 and torch.equal(dst, want), name
        res[f"{name}_ms"] = ms
        res[f"{name}_mib_s"] = n / MiB / (ms / 1e3)
        del t
    t = torch.from_numpy(np.frombuffer(wraps["zlib"], np.uint8).copy()).cuda()
    comp.set_profiling(True)
    stages = []
    for _ in range(a.repeats):
        comp.decompress_stream_tensor(t, n, "zlib", out=dst)
        stages.append(comp.last_stream_stats())
    comp.set_profiling(False)
    res["stats"] = {k: statistics.median(s[k] for s in stages) for k in stages[0]}
    res["scratch_bytes_per_output_byte"] = res["stats"]["scratch_bytes"] / n
    del t
    # the serial decoder on one core, on a prefix stream
    m = min(a.sample, n)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    sample = c.compress(data[:m]) + c.flush()
    t0 = time.perf_counter()
    zlib.decompressobj(-15).decompress(sample)
    res["serial_zlib_mib_s"] = m / MiB / (time.perf_counter() - t0)
    try:
        import oracle_lib as O

        O.lib()
        t0 = time.perf_counter()
        st, w, _ = O.decompress(sample, m)
        assert st == 0 and w == m
        res["serial_oracle_mib_s"] = m / MiB / (time.perf_counter() - t0)
    except Exception as e:  # noqa: BLE001
        res["serial_oracle_error"] = str(e)[:200]
    try:
        import stream_host as H

        t0 = time.perf_counter()
        st, w, _ = H.serial(sample, "raw", m)
        assert st == 0 and w == m
        res["serial_container_hpp_mib_s"] = m / MiB / (time.perf_counter() - t0)
    except Exception as e:  # noqa: BLE001  (no host compiler on the box: the zlib figure stands)
        res["serial_container_hpp_error"] = str(e)[:200]
    # decompress_any on a flushed stream of the same data
    fl = torch.from_numpy(np.frombuffer(zlib_flushed(data), np.uint8).copy()).cuda()
    ms = timed(lambda: comp.decompress_any_tensor(fl, n, "zlib", out=dst), a.repeats)
    assert torch.equal(dst, want)
    res["flushed_any_ms"] = ms
    res["flushed_any_mib_s"] = n / MiB / (ms / 1e3)
    res["speedup_vs_oracle"] = res["zlib_mib_s"] / res["serial_oracle_mib_s"] if "serial_oracle_mib_s" in res else None
    res["speedup_vs_container_hpp"] = (res["zlib_mib_s"] / res["serial_container_hpp_mib_s"]
                                       if "serial_container_hpp_mib_s" in res else None)
    del fl
    # the repair worst case: stored blocks full of DEFLATE data (zlib -6 streams packed again by zlib -6, which stores them)
    k = max(1, min(n, a.stored_bytes) // (4 << 20))
    inner = b"".join(zlib.compress(data[j * (4 << 20):(j + 1) * (4 << 20)], 6) for j in range(k))
    packed = zlib.compress(inner, 6)
    pt = torch.from_numpy(np.frombuffer(packed, np.uint8).copy()).cuda()
    pout = torch.empty(len(inner), dtype=torch.uint8, device="cuda")
    ms = timed(lambda: comp.decompress_stream_tensor(pt, len(inner), "zlib", out=pout), a.repeats)
    out, st = comp.decompress_stream_tensor(pt, len(inner), "zlib", out=pout)
    assert st == 0 and out.cpu().numpy().tobytes() == inner
    s = comp.last_stream_stats()
    res["stored_deflate"] = {"bytes": len(inner), "ms": ms, "mib_s": len(inner) / MiB / (ms / 1e3),
                             **{q: s[q] for q in ("chunks", "candidates", "confirmed", "repair_rounds", "longest_chunk")}}
    del pt, pout
    # streams made of stored blocks (DESIGN 3a "Stored block starts")
    m = a.stored_leg_bytes
    noise = np.random.default_rng(17).integers(0, 256, m, dtype=np.uint8).tobytes()
    piece = 1 << 20
    text = synth.gen_text((m + 1) // 2 + piece, seed=2).tobytes()  # (this leg's own: whatever --bytes is)
    mixed = b"".join(noise[j:j + piece] if (j // piece) & 1 else text[j // 2:j // 2 + piece] for j in range(0, m, piece))[:m]
    for name, plain, level in (("level0_noise", noise, 0), ("level6_noise", noise, 6), ("mixed6", mixed, 6)):
        res[name] = stored_leg(comp, plain, level, a.repeats)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
