"""ctypes binding of include/starflate_hip.h (libstarflate_hip.so).

There is no CPU fallback: if the library is missing or no HIP device is present,
every compute entry point raises.
"""
import ctypes as C
import os

from . import build as _build

NSTAGES = 5
INFLATE_NSTAGES = 2
SEGMENT_BYTES = 32768
STRATEGY = {"auto": 0, "stored": 1, "fixed": 2, "dynamic": 3}
CONTAINER = {"raw": 0, "zlib": 1, "gzip": 2}  # what the decoders take (to them a dictzip file is a gzip stream)
COMPRESS_CONTAINER = dict(CONTAINER, dictzip=3)  # ... and the single-stream compress calls: SFH_DICTZIP
DZ_MAX_CHUNKS = 32762  # SFH_DZ_MAX_CHUNKS
E_NOT_INDEXABLE = -8  # SFH_E_NOT_INDEXABLE
SIZE_FROM_TRAILER = (1 << 64) - 1  # SFH_SIZE_FROM_TRAILER
ITEM_NOT_INDEXABLE = 0xFFFFFFF8  # SFH_ITEM_NOT_INDEXABLE: a per-item status of the sfh_*_any_batch* calls
DBG_NTOK, DBG_TOKENS, DBG_HIST, DBG_PLAN, DBG_LENS, DBG_OFFSETS, DBG_STAMPS = range(7)
DBG_SUBINDEX = 7
DBG_ITEMS, DBG_NITEMS = 8, 9
DBG_SEGINFO = 10
DBG_RITEM = 11
DEFAULT_BLOCK_BYTES = 262144
LARGE_BLOCK_BYTES = 1 << 19
CHAIN_BLOCK_BYTES = 1 << 20
SUBINDEX_WORDS = 64

# every symbol include/starflate_hip.h declares
EXPORTS = [
    "sfh_default_options", "sfh_device_count", "sfh_get_device_props", "sfh_create", "sfh_destroy", "sfh_last_error",
    "sfh_compress_bound", "sfh_compress_bound_container", "sfh_dz_header_bytes", "sfh_compress", "sfh_compress_multi", "sfh_compress_device", "sfh_compress_device_async",
    "sfh_compress_batch_device_async", "sfh_compress_batch", "sfh_batch_index_size", "sfh_copy_batch_index",
    "sfh_decompress_batch_device_async", "sfh_decompress_batch",
    "sfh_decompress_ranges_device_async", "sfh_decompress_range_device", "sfh_decompress_ranges",
    "sfh_dz_read_index", "sfh_dz_read_index_device", "sfh_decompress_dz_device", "sfh_decompress_dz", "sfh_decompress_dz_ranges",
    "sfh_bgzf_bound", "sfh_compress_bgzf_device_async", "sfh_compress_bgzf_device", "sfh_compress_bgzf",
    "sfh_bgzf_read_index", "sfh_bgzf_read_index_device", "sfh_decompress_bgzf_device", "sfh_decompress_bgzf",
    "sfh_decompress_bgzf_wide_device",
    "sfh_decompress_bgzf_ranges_device", "sfh_decompress_bgzf_ranges", "sfh_bgzf_voffsets_to_offsets", "sfh_bgzf_offsets_to_voffsets",
    "sfh_zip_read_index", "sfh_zip_read_index_device", "sfh_decompress_zip_device", "sfh_decompress_zip", "sfh_zip_bound",
    "sfh_compress_zip_device_async", "sfh_compress_zip_device", "sfh_compress_zip",
    "sfh_recover_index_device", "sfh_recover_index", "sfh_decompress_any_device", "sfh_decompress_any", "sfh_last_recover_stats",
    "sfh_recover_index_batch_device", "sfh_recover_index_batch", "sfh_decompress_any_batch_device", "sfh_decompress_any_batch",
    "sfh_inflate_stream_device", "sfh_inflate_stream", "sfh_inflate_stream_batch_device", "sfh_inflate_stream_batch",
    "sfh_last_stream_stats",
    "sfh_last_block_bytes", "sfh_index_entries", "sfh_copy_index", "sfh_copy_subindex", "sfh_decompress_device", "sfh_decompress", "sfh_last_inflate_ms", "sfh_last_decode_scratch_bytes",
    "sfh_inflate_stage_name", "sfh_checksum_device", "sfh_crc32_combine", "sfh_adler32_combine",
    "sfh_set_profiling", "sfh_last_stage_ms", "sfh_stage_name", "sfh_debug_read",
    "sfh_gather_offsets", "sfh_gather_streams", "sfh_comm_ranks", "sfh_lds_order_check",
]


class Options(C.Structure):
    _fields_ = [("strategy", C.c_uint32), ("final_stream", C.c_uint32), ("lazy", C.c_uint32),
                ("no_stored_fast_path", C.c_uint32), ("container", C.c_uint32), ("block_bytes", C.c_uint32),
                ("effort", C.c_uint32), ("chain_depth", C.c_uint32)]


class DzInfo(C.Structure):  # sfh_dz_info
    _fields_ = [("total_n", C.c_uint64), ("nseg", C.c_uint32), ("header_bytes", C.c_uint32), ("status", C.c_uint32),
                ("reserved", C.c_uint32)]


class BgzfInfo(C.Structure):  # sfh_bgzf_info
    _fields_ = [("total_n", C.c_uint64), ("members", C.c_uint32), ("max_isize", C.c_uint32), ("has_eof", C.c_uint32),
                ("status", C.c_uint32)]


class ZipInfo(C.Structure):  # sfh_zip_info
    _fields_ = [("entries", C.c_uint64), ("cd_off", C.c_uint64), ("cd_size", C.c_uint64), ("total_out", C.c_uint64),
                ("zip64", C.c_uint32), ("status", C.c_uint32)]


class ZipEntry(C.Structure):  # sfh_zip_entry (64 bytes)
    _fields_ = [("local_off", C.c_uint64), ("data_off", C.c_uint64), ("csize", C.c_uint64), ("usize", C.c_uint64),
                ("out_off", C.c_uint64), ("name_off", C.c_uint64), ("crc32", C.c_uint32), ("status", C.c_uint32),
                ("method", C.c_uint16), ("flags", C.c_uint16), ("name_len", C.c_uint16), ("pad", C.c_uint16)]


ZIP_ENTRY_UNSUPPORTED = 0xFFFFFFF9  # SFH_ZIP_ENTRY_UNSUPPORTED: a per-entry status of the ZIP reader


class DeviceProps(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("arch", C.c_char * 32), ("compute_units", C.c_uint32),
                ("lds_bytes_per_cu", C.c_uint32), ("l2_bytes", C.c_uint32), ("memory_clock_khz", C.c_uint32),
                ("memory_bus_bits", C.c_uint32), ("clock_khz", C.c_uint32), ("total_memory", C.c_uint64)]


_LIB = None


def lib():
    """Load libstarflate_hip.so (loudly failing if it has not been built)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _build.LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # torch ships its own libamdhip64.so.7 / libhsa-runtime64; two HIP runtimes in one
    # process cannot both see the GPU.  Import torch first so that the DT_NEEDED
    # libamdhip64.so.7 of our library binds to the copy torch has already loaded (a pure
    # C/C++ host without torch gets /opt/rocm's through the library's RUNPATH).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, sz = C.c_void_p, C.c_size_t
    L.sfh_default_options.argtypes = [C.POINTER(Options)]
    L.sfh_default_options.restype = None
    L.sfh_device_count.argtypes = []
    L.sfh_device_count.restype = C.c_int
    L.sfh_get_device_props.argtypes = [C.c_int, C.POINTER(DeviceProps)]
    L.sfh_get_device_props.restype = C.c_int
    L.sfh_create.argtypes = [C.POINTER(vp), C.c_int]
    L.sfh_create.restype = C.c_int
    L.sfh_destroy.argtypes = [vp]
    L.sfh_destroy.restype = None
    L.sfh_last_error.argtypes = [vp]
    L.sfh_last_error.restype = C.c_char_p
    L.sfh_compress_bound.argtypes = [sz, C.c_uint32]
    L.sfh_compress_bound.restype = sz
    L.sfh_compress_bound_container.argtypes = [sz, C.c_uint32, C.c_uint32]
    L.sfh_compress_bound_container.restype = sz
    L.sfh_dz_header_bytes.argtypes = [sz]
    L.sfh_dz_header_bytes.restype = sz
    L.sfh_dz_read_index.argtypes = [vp, sz, C.POINTER(DzInfo), vp, sz]
    L.sfh_dz_read_index.restype = C.c_int
    L.sfh_dz_read_index_device.argtypes = [vp, vp, sz, C.POINTER(DzInfo), vp, sz, vp]
    L.sfh_dz_read_index_device.restype = C.c_int
    L.sfh_decompress_dz_device.argtypes = [vp, vp, sz, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), vp]
    L.sfh_decompress_dz_device.restype = C.c_int
    L.sfh_decompress_dz.argtypes = [vp, vp, sz, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.sfh_decompress_dz.restype = C.c_int
    L.sfh_decompress_dz_ranges.argtypes = [vp, vp, sz, sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(vp), vp]
    L.sfh_decompress_dz_ranges.restype = C.c_int
    L.sfh_bgzf_bound.argtypes = [sz]
    L.sfh_bgzf_bound.restype = sz
    L.sfh_compress_bgzf_device_async.argtypes = [vp, vp, sz, vp, sz, vp, C.POINTER(Options), vp]
    L.sfh_compress_bgzf_device_async.restype = C.c_int
    L.sfh_compress_bgzf_device.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(Options), vp]
    L.sfh_compress_bgzf_device.restype = C.c_int
    L.sfh_compress_bgzf.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(Options)]
    L.sfh_compress_bgzf.restype = C.c_int
    L.sfh_bgzf_read_index.argtypes = [vp, sz, C.POINTER(BgzfInfo), vp, vp, sz]
    L.sfh_bgzf_read_index.restype = C.c_int
    L.sfh_bgzf_read_index_device.argtypes = [vp, vp, sz, C.POINTER(BgzfInfo), vp, vp, sz, vp]
    L.sfh_bgzf_read_index_device.restype = C.c_int
    L.sfh_decompress_bgzf_device.argtypes = [vp, vp, sz, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), vp]
    L.sfh_decompress_bgzf_device.restype = C.c_int
    L.sfh_decompress_bgzf_wide_device.argtypes = [vp, vp, sz, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), vp]
    L.sfh_decompress_bgzf_wide_device.restype = C.c_int
    L.sfh_decompress_bgzf.argtypes = [vp, vp, sz, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.sfh_decompress_bgzf.restype = C.c_int
    u64 = C.POINTER(C.c_uint64)
    L.sfh_decompress_bgzf_ranges_device.argtypes = [vp, vp, sz, vp, vp, C.POINTER(BgzfInfo), sz, u64, u64, C.POINTER(vp), vp, vp]
    L.sfh_decompress_bgzf_ranges_device.restype = C.c_int
    L.sfh_decompress_bgzf_ranges.argtypes = [vp, vp, sz, vp, vp, C.POINTER(BgzfInfo), sz, u64, u64, C.POINTER(vp), vp]
    L.sfh_decompress_bgzf_ranges.restype = C.c_int
    L.sfh_bgzf_voffsets_to_offsets.argtypes = [vp, vp, C.c_uint32, sz, vp, vp]
    L.sfh_bgzf_voffsets_to_offsets.restype = C.c_int
    L.sfh_bgzf_offsets_to_voffsets.argtypes = [vp, vp, C.c_uint32, sz, vp, vp]
    L.sfh_bgzf_offsets_to_voffsets.restype = C.c_int
    L.sfh_zip_read_index.argtypes = [vp, sz, C.POINTER(ZipInfo), vp, sz]
    L.sfh_zip_read_index.restype = C.c_int
    L.sfh_zip_read_index_device.argtypes = [vp, vp, sz, C.POINTER(ZipInfo), vp, sz, vp]
    L.sfh_zip_read_index_device.restype = C.c_int
    L.sfh_decompress_zip_device.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp, vp]
    L.sfh_decompress_zip_device.restype = C.c_int
    L.sfh_decompress_zip.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp]
    L.sfh_decompress_zip.restype = C.c_int
    L.sfh_zip_bound.argtypes = [sz, vp, vp]
    L.sfh_zip_bound.restype = sz
    L.sfh_compress_zip_device_async.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, vp, C.POINTER(Options), vp]
    L.sfh_compress_zip_device_async.restype = C.c_int
    L.sfh_compress_zip_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, C.POINTER(sz), C.POINTER(Options), vp]
    L.sfh_compress_zip_device.restype = C.c_int
    L.sfh_compress_zip.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, C.POINTER(sz), C.POINTER(Options)]
    L.sfh_compress_zip.restype = C.c_int
    L.sfh_compress.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(Options)]
    L.sfh_compress.restype = C.c_int
    L.sfh_compress_multi.argtypes = [C.POINTER(vp), C.c_int, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(Options)]
    L.sfh_compress_multi.restype = C.c_int
    L.sfh_compress_device.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(Options), vp]
    L.sfh_compress_device.restype = C.c_int
    L.sfh_compress_device_async.argtypes = [vp, vp, sz, vp, sz, vp, C.POINTER(Options), vp]
    L.sfh_compress_device_async.restype = C.c_int
    u64p = C.POINTER(C.c_uint64)
    L.sfh_compress_batch_device_async.argtypes = [vp, sz, C.POINTER(vp), u64p, C.POINTER(vp), u64p, vp, C.POINTER(Options), vp]
    L.sfh_compress_batch_device_async.restype = C.c_int
    L.sfh_compress_batch.argtypes = [vp, sz, C.POINTER(vp), u64p, C.POINTER(vp), u64p, u64p, C.POINTER(Options)]
    L.sfh_compress_batch.restype = C.c_int
    L.sfh_batch_index_size.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    L.sfh_batch_index_size.restype = C.c_int
    L.sfh_copy_batch_index.argtypes = [vp, vp, vp, vp, C.c_int, vp]
    L.sfh_copy_batch_index.restype = C.c_int
    L.sfh_decompress_batch_device_async.argtypes = [vp, sz, C.POINTER(vp), u64p, vp, vp, C.POINTER(vp), u64p, vp, C.c_uint32, vp, vp]
    L.sfh_decompress_batch_device_async.restype = C.c_int
    L.sfh_decompress_batch.argtypes = [vp, sz, C.POINTER(vp), u64p, vp, vp, C.POINTER(vp), u64p, vp, C.c_uint32, vp]
    L.sfh_decompress_batch.restype = C.c_int
    L.sfh_decompress_ranges_device_async.argtypes = [vp, vp, sz, vp, vp, sz, C.c_uint64, C.c_uint32, sz, u64p, u64p, C.POINTER(vp), vp, vp]
    L.sfh_decompress_ranges_device_async.restype = C.c_int
    L.sfh_decompress_range_device.argtypes = [vp, vp, sz, vp, vp, sz, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, vp,
                                              C.POINTER(C.c_uint32), vp]
    L.sfh_decompress_range_device.restype = C.c_int
    L.sfh_decompress_ranges.argtypes = [vp, vp, sz, vp, vp, sz, C.c_uint64, C.c_uint32, sz, u64p, u64p, C.POINTER(vp), vp]
    L.sfh_decompress_ranges.restype = C.c_int
    L.sfh_recover_index_device.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint64, vp, sz, vp, vp]
    L.sfh_recover_index_device.restype = C.c_int
    L.sfh_recover_index.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint64, vp, sz, vp]
    L.sfh_recover_index.restype = C.c_int
    L.sfh_decompress_any_device.argtypes = [vp, vp, sz, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint32), vp]
    L.sfh_decompress_any_device.restype = C.c_int
    L.sfh_decompress_any.argtypes = [vp, vp, sz, C.c_uint32, vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint32)]
    L.sfh_decompress_any.restype = C.c_int
    u32p = C.POINTER(C.c_uint32)
    L.sfh_recover_index_batch_device.argtypes = [vp, sz, C.POINTER(vp), u64p, C.c_uint32, u64p, vp, u32p, vp]
    L.sfh_recover_index_batch_device.restype = C.c_int
    L.sfh_recover_index_batch.argtypes = [vp, sz, C.POINTER(vp), u64p, C.c_uint32, u64p, vp, u32p]
    L.sfh_recover_index_batch.restype = C.c_int
    L.sfh_decompress_any_batch_device.argtypes = [vp, sz, C.POINTER(vp), u64p, C.c_uint32, C.POINTER(vp), u64p, u64p, u64p, u32p, vp]
    L.sfh_decompress_any_batch_device.restype = C.c_int
    L.sfh_decompress_any_batch.argtypes = [vp, sz, C.POINTER(vp), u64p, C.c_uint32, C.POINTER(vp), u64p, u64p, u64p, u32p]
    L.sfh_decompress_any_batch.restype = C.c_int
    L.sfh_last_recover_stats.argtypes = [vp, C.POINTER(C.c_float * 2), C.POINTER(C.c_uint64 * 2)]
    L.sfh_last_recover_stats.restype = C.c_int
    L.sfh_inflate_stream_device.argtypes = [vp, vp, sz, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), vp]
    L.sfh_inflate_stream_device.restype = C.c_int
    L.sfh_inflate_stream.argtypes = [vp, vp, sz, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.sfh_inflate_stream.restype = C.c_int
    L.sfh_inflate_stream_batch_device.argtypes = [vp, sz, C.POINTER(vp), u64p, C.c_uint32, C.POINTER(vp), u64p, u64p,
                                                  C.POINTER(C.c_uint32), vp]
    L.sfh_inflate_stream_batch_device.restype = C.c_int
    L.sfh_inflate_stream_batch.argtypes = [vp, sz, C.POINTER(vp), u64p, C.c_uint32, C.POINTER(vp), u64p, u64p, C.POINTER(C.c_uint32)]
    L.sfh_inflate_stream_batch.restype = C.c_int
    L.sfh_last_stream_stats.argtypes = [vp, C.POINTER(C.c_float * 5), C.POINTER(C.c_uint64 * 6)]
    L.sfh_last_stream_stats.restype = C.c_int
    L.sfh_gather_offsets.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sfh_gather_offsets.restype = C.c_int
    L.sfh_comm_ranks.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.sfh_comm_ranks.restype = C.c_int
    L.sfh_gather_streams.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]
    L.sfh_gather_streams.restype = C.c_int
    L.sfh_last_block_bytes.argtypes = [vp]
    L.sfh_last_block_bytes.restype = C.c_uint32
    L.sfh_last_decode_scratch_bytes.argtypes = [vp]
    L.sfh_last_decode_scratch_bytes.restype = sz
    L.sfh_index_entries.argtypes = [vp]
    L.sfh_index_entries.restype = sz
    L.sfh_copy_index.argtypes = [vp, vp, sz, C.c_int, vp]
    L.sfh_copy_index.restype = C.c_int
    L.sfh_copy_subindex.argtypes = [vp, vp, sz, C.c_int, vp]
    L.sfh_copy_subindex.restype = C.c_int
    L.sfh_decompress_device.argtypes = [vp, vp, sz, vp, vp, sz, vp, sz, C.c_uint32, C.POINTER(C.c_uint32), vp]
    L.sfh_decompress_device.restype = C.c_int
    L.sfh_decompress.argtypes = [vp, vp, sz, vp, vp, sz, vp, sz, C.c_uint32, C.POINTER(C.c_uint32)]
    L.sfh_decompress.restype = C.c_int
    L.sfh_last_inflate_ms.argtypes = [vp, C.POINTER(C.c_float * INFLATE_NSTAGES)]
    L.sfh_last_inflate_ms.restype = C.c_int
    L.sfh_inflate_stage_name.argtypes = [C.c_int]
    L.sfh_inflate_stage_name.restype = C.c_char_p
    L.sfh_checksum_device.argtypes = [vp, vp, sz, C.c_uint32, C.POINTER(C.c_uint32), vp]
    L.sfh_checksum_device.restype = C.c_int
    L.sfh_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    L.sfh_crc32_combine.restype = C.c_uint32
    L.sfh_adler32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    L.sfh_adler32_combine.restype = C.c_uint32
    L.sfh_set_profiling.argtypes = [vp, C.c_int]
    L.sfh_set_profiling.restype = None
    L.sfh_last_stage_ms.argtypes = [vp, C.POINTER(C.c_float * NSTAGES)]
    L.sfh_last_stage_ms.restype = C.c_int
    L.sfh_stage_name.argtypes = [C.c_int]
    L.sfh_stage_name.restype = C.c_char_p
    L.sfh_debug_read.argtypes = [vp, C.c_int, vp, sz]
    L.sfh_debug_read.restype = C.c_int
    L.sfh_lds_order_check.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sfh_lds_order_check.restype = C.c_int
    _LIB = L
    return L


def device_props(device=0):
    p = DeviceProps()
    rc = lib().sfh_get_device_props(int(device), C.byref(p))
    if rc:
        raise RuntimeError(f"sfh_get_device_props({device}) -> {rc}")
    return {k: (getattr(p, k).decode() if isinstance(getattr(p, k), bytes) else getattr(p, k)) for k, _ in p._fields_ if k != "reserved"}


EFFORT = {"default": 0, "fast": 1, "fastest": 2, "thorough": 3, "max": 4, "best": 5, "ultra": 6, "extreme": 7, "recent": 8, "recent_all": 9}


def make_options(strategy="auto", final_stream=True, lazy=True, stored_fast_path=True, container="raw", block_bytes=0,
                 effort="default"):
    o = Options()
    lib().sfh_default_options(C.byref(o))
    o.strategy = STRATEGY[strategy] if isinstance(strategy, str) else int(strategy)
    o.final_stream = int(bool(final_stream))
    o.lazy = 3 if lazy is True else int(lazy)
    o.no_stored_fast_path = int(not stored_fast_path)
    o.container = COMPRESS_CONTAINER[container] if isinstance(container, str) else int(container)
    o.block_bytes = int(block_bytes)
    if isinstance(effort, str) and effort.startswith("chain"):  # "chain4": exact hash chains of that depth
        o.effort, o.chain_depth = EFFORT["best"], int(effort[5:].lstrip(":") or 8)
    else:
        o.effort = EFFORT[effort] if isinstance(effort, str) else int(effort)
    return o


def resolve_block_bytes(block_bytes, n, effort="default"):
    """What sfh_options.block_bytes = 0 stands for on an input of n bytes (mirrors sf_capi.hip): up to 256 KiB, 1 MiB with
    the chain efforts."""
    if block_bytes:
        return int(block_bytes)
    if isinstance(effort, str):  # a name, "chainN", or (as make_options accepts) the enum's integer
        e = EFFORT["best"] if effort.startswith("chain") else EFFORT[effort]
    else:
        e = int(effort)
    chain = EFFORT["best"] <= e <= EFFORT["extreme"]
    b = CHAIN_BLOCK_BYTES if chain else LARGE_BLOCK_BYTES
    while b > DEFAULT_BLOCK_BYTES and n // b < (1024 if chain else 2048):
        b >>= 1
    while b > SEGMENT_BYTES and n // b < 256:
        b >>= 1
    return b
