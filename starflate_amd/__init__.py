"""starflate_amd -- MI355X-native DEFLATE compressor (hand-written HIP, gfx950).

Only what the hot path needs: csrc/ (HIP kernels + C-ABI), the ctypes binding,
torch plumbing for device buffers, the multi-GPU shard/concat helper and the
synthetic corpora used by tests and bench.py.
"""
from .compressor import (CHUNK_BYTES, ITEM_NOT_INDEXABLE, Compressor, StarflateError, checksum_combine, compress, compress_batch,  # noqa: F401
                         compress_multi, decompress, decompress_any_batch, decompress_batch, decompress_range, decompress_ranges,
                         decompress_dictzip, decompress_stream, decompress_stream_batch, dictzip_index, read_ranges, wrapper_bytes,
                         bgzf_index, compress_bgzf, decompress_bgzf, read_bgzf_ranges, bgzf_voffsets_to_offsets,
                         bgzf_offsets_to_voffsets, ZIP_ENTRY_DTYPE, ZIP_ENTRY_UNSUPPORTED, compress_zip, decompress_zip, zip_bound,
                         zip_index, zip_names)

__all__ = ["Compressor", "StarflateError", "compress", "CHUNK_BYTES", "checksum_combine", "wrapper_bytes", "compress_multi", "compress_batch", "decompress", "decompress_batch", "decompress_range", "decompress_ranges", "decompress_stream",
           "decompress_stream_batch", "decompress_any_batch", "ITEM_NOT_INDEXABLE", "dictzip_index", "decompress_dictzip", "read_ranges",
           "compress_bgzf", "decompress_bgzf", "bgzf_index", "read_bgzf_ranges", "bgzf_voffsets_to_offsets", "bgzf_offsets_to_voffsets",
           "compress_zip", "decompress_zip", "zip_index", "zip_names", "zip_bound", "ZIP_ENTRY_DTYPE", "ZIP_ENTRY_UNSUPPORTED"]
