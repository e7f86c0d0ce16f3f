"""The single indexed decode (sfh_decompress / sfh_decompress_device) against a record made by the commit BEFORE it became a
batch of one: tests/golden/single_decode_parent.json holds, for the smallest shapes at which building a segment's geometry can
go wrong, what that commit's implicit-geometry kernels returned -- status, the sfh_last_error text of a failing decode, the
token scratch of the call, SHA-256 of the output and of the SFH_DBG_SEGINFO rows.  Every field must be equal; independently of
the record, every decode that reports success must return its input.

SF_RECORD_SINGLE=<path>: write that JSON instead of comparing (run once, on the GPU, in a checkout of the recorded commit with
this file and single_decode_cases.py added: they use nothing newer).  The JSON also holds the statuses the single call gave for the items of two batch tests
of test_gpu_batch_inflate.py (damaged_batch / first_entry_batch, single_decode_cases.py), which assert them as literals."""
import hashlib
import json
import os

import numpy as np
import pytest

from single_decode_cases import CHUNK, context_under, damaged_batch, first_entry_batch, parent_record
from starflate_amd import _capi, build, synth

pytestmark = pytest.mark.gpu

RECORD = os.environ.get("SF_RECORD_SINGLE")
FIELDS = ("status", "error", "scratch_bytes", "out_sha256", "seginfo_sha256")


def _single_statuses(comp, batch):
    sizes, _, streams, _, _, bb, per = batch
    return {str(use_sub).lower(): [comp.decompress(streams[i], per[i][0], n, subindex=per[i][1] if use_sub else None,
                                                   block_bytes=int(bb[i]))[1] for i, n in enumerate(sizes)]
            for use_sub in (False, True)}


def _decode(c, stream, index, n, sub, bb):
    out, st = c.decompress(stream, index, n, subindex=sub, block_bytes=bb)
    r = {"status": st, "scratch_bytes": c.last_decode_scratch_bytes(),
         "seginfo_sha256": hashlib.sha256(c.debug(_capi.DBG_SEGINFO, index.size - 1).tobytes()).hexdigest()}
    if st:
        r["error"] = c.last_error()
    else:
        r["out_sha256"] = hashlib.sha256(out).hexdigest()
    return r, out


@pytest.fixture(scope="module")
def results():
    """name -> (what the decode returned, its output, the input), and the single call's statuses on the batch tests' items"""
    ctxs = {"default": context_under(), "serial": context_under(SFH_INFLATE_SERIAL="1"), "cap8": context_under(SFH_BATCH_CHUNKS="8"),
            "cap2": context_under(SFH_BATCH_CHUNKS="2")}
    enc = ctxs["default"]
    res = {}

    def own(data, bb):
        stream = np.frombuffer(enc.compress(data, block_bytes=bb), np.uint8).copy()
        return stream, enc.last_index(), enc.last_subindex()

    def run(name, ctx, stream, index, n, sub, bb, want):
        r, out = _decode(ctxs[ctx], stream, index, n, sub, bb)
        res[name] = (r, out, want)

    try:
        text = synth.gen_text(7 * CHUNK, seed=61)
        for n in (0, 1, CHUNK, CHUNK + 1, 7 * CHUNK - 5):
            for bb in (CHUNK, 4 * CHUNK):
                stream, index, sub = own(text[:n], bb)
                run(f"geometry/{n}/{bb}/sub", "default", stream, index, n, sub, bb, text[:n])
                run(f"geometry/{n}/{bb}/index", "default", stream, index, n, None, bb, text[:n])
                run(f"geometry/{n}/{bb}/serial", "serial", stream, index, n, None, bb, text[:n])
        # test_decoder_batches' 23 segments: a partial last batch; a strip larger than a batch
        data = np.concatenate([synth.gen_text(9 * CHUNK + 777, seed=11), synth.gen_mixed(14 * CHUNK, seed=12)])
        for ctx, bb in (("cap8", CHUNK), ("cap8", 4 * CHUNK), ("cap2", 4 * CHUNK)):
            stream, index, sub = own(data, bb)
            run(f"batches/{ctx}/{bb}/sub", ctx, stream, index, data.size, sub, bb, data)
            run(f"batches/{ctx}/{bb}/index", ctx, stream, index, data.size, None, bb, data)
        stored = np.random.default_rng(62).integers(0, 256, 3 * CHUNK + 100, dtype=np.uint8)
        mixed = synth.gen_mixed(3 << 20, seed=4, stripe=1 << 16)[: (1 << 20) + 13]
        for name, d in (("stored", stored), ("mixed", mixed)):
            for bb in (CHUNK, 4 * CHUNK):
                stream, index, sub = own(d, bb)
                run(f"{name}/{bb}/sub", "default", stream, index, d.size, sub, bb, d)
                run(f"{name}/{bb}/index", "default", stream, index, d.size, None, bb, d)
        # a gzip stream decoded raw through its index: entry 0 = 10
        item = synth.gen_text(70000, seed=63)
        gz = enc.compress_batch([item], container="gzip")[0]
        gidx, gsub, gbb = enc.last_batch_index()
        assert int(gidx[0]) == 10
        run("entry0/sub", "default", gz, gidx, item.size, gsub.reshape(-1, 32, 2), int(gbb[0]), item)
        run("entry0/index", "default", gz, gidx, item.size, None, int(gbb[0]), item)
        # damage, on the 23 segments in strips of four
        bb = 4 * CHUNK
        stream, index, sub = own(data, bb)
        for mode, s in (("sub", sub), ("index", None)):
            bad = stream.copy()
            bad[int(index[19]) + 9] ^= 0x5A
            run(f"damage/flip19/{mode}", "default", bad, index, data.size, s, bb, data)
            ix = index.copy()
            ix[5] += np.uint64(3)
            run(f"damage/index5/{mode}", "default", stream, ix, data.size, s, bb, data)
            run(f"damage/cut20/{mode}", "default", stream[: int(index[20])], index, data.size, s, bb, data)
        sb = sub.copy()
        sb[3, 5, 0] += np.uint32(7)  # word 2 * 5 of segment 3
        run("damage/sub3/sub", "default", stream, index, data.size, sb, bb, data)
        wide, windex, wsub = own(data, 8 * CHUNK)
        run("damage/block_bytes/sub", "default", wide, windex, data.size, wsub, CHUNK, data)
        run("damage/block_bytes/index", "default", wide, windex, data.size, None, CHUNK, data)
        batch = {"damaged": _single_statuses(enc, damaged_batch(enc)), "first_entry": _single_statuses(enc, first_entry_batch(enc))}
    finally:
        for c in ctxs.values():
            c.close()
    return res, batch


def test_single_decode_equals_the_parent_record(results):
    res, batch = results
    if RECORD:
        doc = {"parent": build.source_stamp()["commit"], "dropped": [], "cases": {k: v[0] for k, v in res.items()},
               "batch_want_st": batch}
        with open(RECORD, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    rec = parent_record()
    assert sorted(rec["cases"]) == sorted(res)
    dropped = {(d["case"], d["field"]) for d in rec["dropped"]}
    assert all(c.startswith("damage/") and f == "seginfo_sha256" for c, f in dropped)
    for name, want in rec["cases"].items():
        got = res[name][0]
        for field in FIELDS:
            if (name, field) in dropped:
                continue
            assert got.get(field) == want.get(field), (name, field, got.get(field), want.get(field))
    assert batch == rec["batch_want_st"]


def test_every_success_returns_its_input(results):
    res, _ = results
    for name, (r, out, want) in res.items():
        if r["status"] == 0:
            assert out == want.tobytes(), name
        assert r["status"] == 0 or name.startswith("damage/"), name
