"""BGZF random access (sfh_decompress_bgzf_ranges*): the files, the range sets and the calls of tests/test_gpu_bgzf_ranges.py.
Run as a script in a child process (`python bgzf_range_cases.py CASE`), with SFH_INFLATE_SERIAL or SFH_BATCH_CHUNKS set by the
parent, it runs one case through the device call, checks it against slices of the payload and prints a digest of the bytes
(and, for "batches", the token scratch of the call)."""
import ctypes as C
import hashlib
import sys

import numpy as np

import bgzf_files as BZ

GUARD = 0xA5
NARROW = [0, 1, 100, 32768, 31, 0]
WIDE = [65280, 65280, 7, 65536, 0, 5]


def cuda(data):
    import torch

    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda() if len(data) else torch.empty(0, dtype=torch.uint8, device="cuda")


def info_struct(info, **over):
    from starflate_amd import _capi

    d = dict(info, status=0)
    d.update(over)
    return _capi.BgzfInfo(d["total_n"], d["members"], d["max_isize"], int(d["has_eof"]), d["status"])


def device_index(comp, blob):
    """-> (member_off, out_off: int64 tensors on the device, info dict), from the device walk"""
    return comp.bgzf_index_tensor(cuda(blob))


def run_device(comp, blob, ranges, index=None, stream=None, gap=3, **over):
    """sfh_decompress_bgzf_ranges_device -> (rc, list of bytes, list of statuses, the destinations' places).  **over: fields of
    the info the call is given instead of the index's own.  The destinations lie in one buffer, `gap`
    guard bytes between them and 64 at both ends, so their addresses take every alignment; every byte of the buffer outside
    the destinations must still hold the guard value afterwards (all of it after a refused call)."""
    import torch
    from starflate_amd import _capi

    src = cuda(blob)
    moff, ooff, info = device_index(comp, blob) if index is None else index
    binfo = info_struct(info, **over)
    k = len(ranges)
    pos, at = [], 64
    for _, ln in ranges:
        pos.append(at)
        at += ln + gap
    buf = torch.full((at + 64,), GUARD, dtype=torch.uint8, device="cuda")
    status = torch.full((max(k, 1),), 77, dtype=torch.int32, device="cuda")
    dp = (C.c_void_p * max(k, 1))(*[buf.data_ptr() + p for p in pos])
    offs = (C.c_uint64 * max(k, 1))(*[r[0] for r in ranges])
    lens = (C.c_uint64 * max(k, 1))(*[r[1] for r in ranges])
    torch.cuda.synchronize()
    rc = _capi.lib().sfh_decompress_bgzf_ranges_device(comp._h, src.data_ptr(), len(blob), moff.data_ptr(), ooff.data_ptr(), C.byref(binfo),
                                                       k, offs, lens, dp, status.data_ptr(), C.c_void_p(stream) if stream else None)
    torch.cuda.synchronize()
    back = buf.cpu().numpy()
    keep = np.ones(back.size, bool)
    if rc == 0:
        for p, (_, ln) in zip(pos, ranges):
            keep[p: p + ln] = False
    assert np.all(back[keep] == GUARD), "a byte outside the destinations was written"
    return rc, [back[p: p + ln].tobytes() for p, (_, ln) in zip(pos, ranges)], [int(v) for v in status.cpu().numpy()[:k]], pos


def check_exact(data, ranges, outs, st):
    assert st == [0] * len(ranges), [(r, s) for r, s in zip(ranges, st) if s][:5]
    for (off, ln), got in zip(ranges, outs):
        assert got == data[off: off + ln], (off, ln)


def boundary_ranges(out_off, total, lengths=(0, 1, 3, 4, 5, 4096), reach=2):
    """every range of one of the lengths that starts or ends within `reach` bytes of a member boundary"""
    out = set()
    for b in out_off:
        for d in range(-reach, reach + 1):
            for ln in lengths:
                for off in (b + d, b + d - ln):  # starts there, ends there
                    if 0 <= off and off + ln <= total:
                        out.add((off, ln))
    return sorted(out)


def scale_ranges(out_off, total, count, seed=0, members=50):
    """`count` ranges of a file of many small members: boundary_ranges of `members` boundaries in its middle (the first
    `count` of them at most), the rest at random offsets with lengths 0 .. 200"""
    mid = len(out_off) // 2
    out = boundary_ranges(out_off[mid: mid + members], total, lengths=(0, 1, 3, 4, 5, 200))[:count]
    rng = np.random.default_rng(seed)
    while len(out) < count:
        ln = int(rng.integers(0, 201))
        out.append((int(rng.integers(0, total - ln + 1)), ln))
    return out


def narrow_case():
    data = BZ.text(sum(NARROW), seed=1)
    blob, moff, ooff = BZ.write(data, NARROW)
    ranges = boundary_ranges(ooff, len(data)) + [(0, len(data)), (len(data), 0)]
    return data, blob, ranges


def wide_case():
    data = BZ.text(sum(WIDE), seed=31)
    blob, moff, ooff = BZ.write(data, WIDE)  # (member()'s size assertion holds: text packs to well under 64 KiB)
    total = len(data)
    ranges = []
    for i in (0, 1, 3):  # the wide members
        b, n = ooff[i], WIDE[i]
        for edge in (32767, 32768, 32769):
            for ln in (1, 2, 3, 4, 5, 100, 20000):
                ranges += [(b + edge, ln), (b + edge - ln, ln)]  # windows that start / end at the 32 KiB mark
        ranges += [(b + 40000, 1000), (b + 32768, n - 32768), (b + 50000, n - 50000), (b, n)]  # wholly in the second 32 KiB; all
    ranges += [(ooff[1] - 3, 6), (ooff[1] - 40000, 80000), (ooff[0] + 10, ooff[4] - 10), (ooff[2] - 1, 9), (0, total), (total, 0)]
    ranges += [(ooff[3] + 32760 + a, ln) for a in range(4) for ln in (1, 2, 3, 4, 5)]  # short windows, every source alignment
    assert all(off + ln <= total for off, ln in ranges)
    return data, blob, ranges


def batches_case():
    """one range over five members, twenty single-member ranges beside it"""
    sizes = [65280] * 5 + [1000] * 20
    data = BZ.text(sum(sizes), seed=32)
    blob, moff, ooff = BZ.write(data, sizes)
    ranges = [(ooff[5 + k] + 7 * k, 500) for k in range(10)] + [(100, 5 * 65280 - 200)] + [(ooff[15 + k] + k, 900) for k in range(10)]
    return data, blob, ranges


def main(case):
    from starflate_amd import Compressor

    data, blob, ranges = {"narrow": narrow_case, "wide": wide_case, "batches": batches_case}[case]()
    comp = Compressor(0)
    rc, outs, st, pos = run_device(comp, blob, ranges)
    assert rc == 0
    check_exact(data, ranges, outs, st)
    assert len({p % 4 for p in pos}) == 4
    print(comp.last_decode_scratch_bytes(), hashlib.sha256(b"".join(outs)).hexdigest())
    comp.close()


if __name__ == "__main__":
    main(sys.argv[1])
