"""The single index-free calls (sfh_decompress_any*, sfh_recover_index*) against a record made by the commit BEFORE they became
a batch of one: tests/golden/any_single_parent.json holds, for every case of any_single_cases.py, what that commit's
single-body driver and kernels returned -- rc, status, the sfh_last_error text of a failing call, SHA-256 of the output, of the
index and of the depends flags, whether a failing call left its destination alone, the nodes and rows of
sfh_last_recover_stats and the token scratch.  Every field must be equal; independently of the record, every decode that
reports rc 0 and status 0 must return the bytes zlib decodes from the stream (for the intact streams: the input).

SF_RECORD_ANY_SINGLE=<path>: write that JSON instead of comparing (run once, on the GPU, in a checkout of the recorded commit
with this file and any_single_cases.py added: they use nothing newer)."""
import json
import os

import pytest

from any_single_cases import TRAILER, cases, contexts, parent_record, run_case, zlib_says
from starflate_amd import build

pytestmark = pytest.mark.gpu

RECORD = os.environ.get("SF_RECORD_ANY_SINGLE")
FIELDS = ("rc", "status", "error", "out_sha256", "dst_untouched", "dst_n_out", "index_sha256", "depends_sha256", "nodes", "rows",
          "scratch_bytes")


@pytest.fixture(scope="module")
def results():
    """name -> (what the call returned, the decoded bytes or None, the bytes zlib gives or None)"""
    ctxs = contexts()
    res = {}
    try:
        for name, ctx, entry, stream, container, dst_n, opt in cases(ctxs["default"]):
            assert name not in res
            r, out = run_case(ctxs[ctx], entry, stream, container, dst_n, opt)
            size = dst_n if dst_n != TRAILER else int.from_bytes(stream[-4:], "little")
            res[name] = (r, out, zlib_says(stream, size, container) if out is not None else None)
    finally:
        for c in ctxs.values():
            c.close()
    return res


def test_single_calls_equal_the_parent_record(results):
    if RECORD:
        doc = {"parent": build.source_stamp()["commit"], "cases": {k: v[0] for k, v in results.items()}}
        with open(RECORD, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    rec = parent_record()
    assert sorted(rec["cases"]) == sorted(results)
    for name, want in rec["cases"].items():
        got = results[name][0]
        for field in FIELDS:
            assert got.get(field) == want.get(field), (name, field, got.get(field), want.get(field))


def test_every_success_returns_its_input(results):
    decodes = 0
    for name, (r, out, want) in results.items():
        if out is not None and r["rc"] == 0 and r["status"] == 0:
            # (an explicit dst_n one above ISIZE is taken as it is, wrapper/above_isize: the byte behind the stream's last
            # stays unwritten, and the record holds that answer)
            assert want is not None and len(want) >= min(len(out), 1) and out[:len(want)] == want, name
            assert len(want) == len(out) or name == "wrapper/above_isize/decode", name
            decodes += 1
        if name.startswith(("geometry/", "serial/", "cap2/", "lastwave/", "stream/", "depends/", "wrapper/flags")):
            assert r["rc"] == 0 and r.get("status", 0) == 0, name
    assert decodes > 100  # (the 96 geometry decodes alone)
