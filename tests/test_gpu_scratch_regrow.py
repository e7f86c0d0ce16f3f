"""A context's scratch buffers grown and then reused (sf_scratch.h: every buffer, pinned table and event of sfh_ctx owns what it
holds), on ONE context through the Python wrapper: per family three calls in a row -- one item of 1 byte, then items of 1, 32769
and 100000 bytes (one segment, a segment boundary, several segments: the buffers grow), then the one-byte item again (the grown
buffers and the table pairs are reused by a smaller call).  A pointer taken from a buffer before a later grow of it, or a pinned
table refilled under a copy that still reads it, shows as wrong bytes here.  The expected bytes are the inputs, and zlib, gzip
and zipfile read what the writers wrote.  Then the context is closed, and a second one runs one family again."""
import gzip
import io
import zipfile
import zlib

import pytest

from starflate_amd import Compressor, synth

pytestmark = pytest.mark.gpu

SEG = 32768
SIZES = (1, 32769, 100000)
ROUNDS = ((1,), SIZES, (1,))


@pytest.fixture(scope="module")
def comp():
    c = Compressor(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def inputs():
    """size -> its bytes (the middle size: text and noise mixed, the others text)"""
    return {n: (synth.gen_mixed(n, seed=31 + i) if n == SIZES[1] else synth.gen_text(n, seed=31 + i)).tobytes() for i, n in enumerate(SIZES)}


def test_any_batch_grows_and_reuses(comp, inputs):
    flushed = {}
    for n, data in inputs.items():  # block-flushed every 32 KiB: what the index-free decoder reads
        flushed[n] = comp.compress(data, block_bytes=SEG)
        assert zlib.decompress(flushed[n], -15) == data
    for sizes in ROUNDS:
        out, st = comp.decompress_any_batch([flushed[n] for n in sizes], list(sizes))
        assert st == [0] * len(sizes), (sizes, st)
        assert out == [inputs[n] for n in sizes], sizes


def test_stream_batch_grows_and_reuses(comp, inputs):
    streams = {n: zlib.compress(data, 6) for n, data in inputs.items()}  # no flush points
    for sizes in ROUNDS:
        out, st = comp.decompress_stream_batch([streams[n] for n in sizes], list(sizes), container="zlib")
        assert st == [0] * len(sizes), (sizes, st)
        assert out == [inputs[n] for n in sizes], sizes


def test_bgzf_grows_and_reuses(comp, inputs):
    for sizes in ROUNDS:
        for n in sizes:
            f = comp.compress_bgzf(inputs[n])
            assert gzip.decompress(f) == inputs[n], n
            back, st = comp.decompress_bgzf(f)
            assert st == 0 and back == inputs[n], n


def zip_round(comp, inputs, sizes):
    items = [(f"item{k}_{n}.bin", inputs[n]) for k, n in enumerate(sizes)]
    archive = comp.compress_zip(items)
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        assert z.testzip() is None
        assert [(i.filename, z.read(i)) for i in z.infolist()] == items
    out, st = comp.decompress_zip(archive)
    assert not st.any(), (sizes, st)
    assert out == dict(items), sizes


def test_zip_grows_and_reuses(comp, inputs):
    for sizes in ROUNDS:
        zip_round(comp, inputs, sizes)


def test_second_context_after_close(comp, inputs):
    """(the module's last test) the context of the tests above is closed with every buffer grown -- each frees itself -- and a
    second one gives the same bytes for the same calls"""
    zip_round(comp, inputs, SIZES)
    comp.close()  # (the fixture's own close is then a no-op)
    second = Compressor(0)
    try:
        for sizes in ROUNDS:
            zip_round(second, inputs, sizes)
    finally:
        second.close()
