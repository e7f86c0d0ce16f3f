"""ctypes binding of include/starflate_hip.h (libstarflate_hip.so).

There is no CPU fallback: if the library is missing or no HIP device is present,
every compute entry point raises.
"""
import ctypes as C
import os

from . import build as _build

NSTAGES = 5
INFLATE_NSTAGES = 2
STREAM_NSTAGES = 5  # SFH_STREAM_NSTAGES, SFH_STREAM_NCOUNTS: sfh_last_stream_stats' arrays
STREAM_NCOUNTS = 6
SEGMENT_BYTES = 32768
STRATEGY = {"auto": 0, "stored": 1, "fixed": 2, "dynamic": 3}
CONTAINER = {"raw": 0, "zlib": 1, "gzip": 2}  # what the decoders take (to them a dictzip file is a gzip stream)
COMPRESS_CONTAINER = dict(CONTAINER, dictzip=3)  # ... and the single-stream compress calls: SFH_DICTZIP
STREAM_CONTAINER = dict(CONTAINER, gzip_members=4)  # ... and the decompress_stream* family: SFH_GZIP_MEMBERS
DZ_MAX_CHUNKS = 32762  # SFH_DZ_MAX_CHUNKS
E_NOT_INDEXABLE = -8  # SFH_E_NOT_INDEXABLE
SIZE_FROM_TRAILER = (1 << 64) - 1  # SFH_SIZE_FROM_TRAILER
ITEM_NOT_INDEXABLE = 0xFFFFFFF8  # SFH_ITEM_NOT_INDEXABLE: a per-item status of the sfh_*_any_batch* calls
DBG_NTOK, DBG_TOKENS, DBG_HIST, DBG_PLAN, DBG_LENS, DBG_OFFSETS, DBG_STAMPS = range(7)
DBG_SUBINDEX = 7
DBG_ITEMS, DBG_NITEMS = 8, 9
DBG_SEGINFO = 10
DBG_RITEM = 11
DBG_STREAM_MEMBERS = 12
DEFAULT_BLOCK_BYTES = 262144
LARGE_BLOCK_BYTES = 1 << 19
CHAIN_BLOCK_BYTES = 1 << 20
SUBINDEX_WORDS = 64


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


def _prototypes():
    """{symbol: (restype, argtypes)} of every function include/starflate_hip.h declares, parameter for parameter.  A pointer
    is typed where callers hand over a ctypes array or a byref, and vp where they hand over an address (a context, a buffer,
    a stream, a numpy array's data): tests and tools call these functions directly and rely on which is which."""
    i, vp, sz, u32, u64 = C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64
    vpp, szp, u32p, u64p, opt = C.POINTER(vp), C.POINTER(sz), C.POINTER(u32), C.POINTER(u64), C.POINTER(Options)
    dz, bgzf, zinfo = C.POINTER(DzInfo), C.POINTER(BgzfInfo), C.POINTER(ZipInfo)
    return {
        "sfh_default_options": (None, [opt]),
        "sfh_device_count": (i, []),
        "sfh_get_device_props": (i, [i, C.POINTER(DeviceProps)]),
        "sfh_create": (i, [vpp, i]),
        "sfh_destroy": (None, [vp]),
        "sfh_last_error": (C.c_char_p, [vp]),
        "sfh_compress_bound": (sz, [sz, u32]),
        "sfh_compress_bound_container": (sz, [sz, u32, u32]),
        # seekable gzip (dictzip)
        "sfh_dz_header_bytes": (sz, [sz]),
        "sfh_dz_read_index": (i, [vp, sz, dz, vp, sz]),
        "sfh_dz_read_index_device": (i, [vp, vp, sz, dz, vp, sz, vp]),
        "sfh_decompress_dz_device": (i, [vp, vp, sz, vp, u64, u64p, u32p, vp]),
        "sfh_decompress_dz": (i, [vp, vp, sz, vp, u64, u64p, u32p]),
        "sfh_decompress_dz_ranges": (i, [vp, vp, sz, sz, u64p, u64p, vpp, vp]),
        # BGZF
        "sfh_bgzf_bound": (sz, [sz]),
        "sfh_compress_bgzf_device_async": (i, [vp, vp, sz, vp, sz, vp, opt, vp]),
        "sfh_compress_bgzf_device": (i, [vp, vp, sz, vp, sz, szp, opt, vp]),
        "sfh_compress_bgzf": (i, [vp, vp, sz, vp, sz, szp, opt]),
        "sfh_bgzf_read_index": (i, [vp, sz, bgzf, vp, vp, sz]),
        "sfh_bgzf_read_index_device": (i, [vp, vp, sz, bgzf, vp, vp, sz, vp]),
        "sfh_decompress_bgzf_device": (i, [vp, vp, sz, vp, u64, u64p, u32p, vp]),
        "sfh_decompress_bgzf_wide_device": (i, [vp, vp, sz, vp, u64, u64p, u32p, vp]),
        "sfh_decompress_bgzf": (i, [vp, vp, sz, vp, u64, u64p, u32p]),
        "sfh_decompress_bgzf_ranges_device": (i, [vp, vp, sz, vp, vp, bgzf, sz, u64p, u64p, vpp, vp, vp]),
        "sfh_decompress_bgzf_ranges": (i, [vp, vp, sz, vp, vp, bgzf, sz, u64p, u64p, vpp, vp]),
        "sfh_bgzf_voffsets_to_offsets": (i, [vp, vp, u32, sz, vp, vp]),
        "sfh_bgzf_offsets_to_voffsets": (i, [vp, vp, u32, sz, vp, vp]),
        # ZIP archives
        "sfh_zip_read_index": (i, [vp, sz, zinfo, vp, sz]),
        "sfh_zip_read_index_device": (i, [vp, vp, sz, zinfo, vp, sz, vp]),
        "sfh_decompress_zip_device": (i, [vp, vp, sz, vp, sz, vp, vp, vp, vp]),
        "sfh_decompress_zip": (i, [vp, vp, sz, vp, sz, vp, vp, vp]),
        "sfh_zip_bound": (sz, [sz, vp, vp]),
        "sfh_compress_zip_device_async": (i, [vp, sz, vp, vp, vp, vp, vp, sz, vp, opt, vp]),
        "sfh_compress_zip_device": (i, [vp, sz, vp, vp, vp, vp, vp, sz, szp, opt, vp]),
        "sfh_compress_zip": (i, [vp, sz, vp, vp, vp, vp, vp, sz, szp, opt]),
        # one stream, and many in one call
        "sfh_compress": (i, [vp, vp, sz, vp, sz, szp, opt]),
        "sfh_compress_multi": (i, [vpp, i, vp, sz, vp, sz, szp, opt]),
        "sfh_compress_device": (i, [vp, vp, sz, vp, sz, szp, opt, vp]),
        "sfh_compress_device_async": (i, [vp, vp, sz, vp, sz, vp, opt, vp]),
        "sfh_compress_batch_device_async": (i, [vp, sz, vpp, u64p, vpp, u64p, vp, opt, vp]),
        "sfh_compress_batch": (i, [vp, sz, vpp, u64p, vpp, u64p, u64p, opt]),
        "sfh_batch_index_size": (i, [vp, szp, szp]),
        "sfh_copy_batch_index": (i, [vp, vp, vp, vp, i, vp]),
        # the indexed decoder: batches and ranges
        "sfh_decompress_batch_device_async": (i, [vp, sz, vpp, u64p, vp, vp, vpp, u64p, vp, u32, vp, vp]),
        "sfh_decompress_batch": (i, [vp, sz, vpp, u64p, vp, vp, vpp, u64p, vp, u32, vp]),
        "sfh_decompress_ranges_device_async": (i, [vp, vp, sz, vp, vp, sz, u64, u32, sz, u64p, u64p, vpp, vp, vp]),
        "sfh_decompress_range_device": (i, [vp, vp, sz, vp, vp, sz, u64, u32, u64, u64, vp, u32p, vp]),
        "sfh_decompress_ranges": (i, [vp, vp, sz, vp, vp, sz, u64, u32, sz, u64p, u64p, vpp, vp]),
        # decoding without side information
        "sfh_recover_index_device": (i, [vp, vp, sz, u32, u64, vp, sz, vp, vp]),
        "sfh_recover_index": (i, [vp, vp, sz, u32, u64, vp, sz, vp]),
        "sfh_decompress_any_device": (i, [vp, vp, sz, u32, vp, u64, u32p, vp]),
        "sfh_decompress_any": (i, [vp, vp, sz, u32, vp, u64, u64, u64p, u32p]),
        "sfh_recover_index_batch_device": (i, [vp, sz, vpp, u64p, u32, u64p, vp, u32p, vp]),
        "sfh_recover_index_batch": (i, [vp, sz, vpp, u64p, u32, u64p, vp, u32p]),
        "sfh_decompress_any_batch_device": (i, [vp, sz, vpp, u64p, u32, vpp, u64p, u64p, u64p, u32p, vp]),
        "sfh_decompress_any_batch": (i, [vp, sz, vpp, u64p, u32, vpp, u64p, u64p, u64p, u32p]),
        "sfh_last_recover_stats": (i, [vp, C.POINTER(C.c_float * 2), C.POINTER(u64 * 2)]),
        "sfh_inflate_stream_device": (i, [vp, vp, sz, u32, vp, u64, u64p, u32p, vp]),
        "sfh_inflate_stream": (i, [vp, vp, sz, u32, vp, u64, u64p, u32p]),
        "sfh_inflate_stream_batch_device": (i, [vp, sz, vpp, u64p, u32, vpp, u64p, u64p, u32p, vp]),
        "sfh_inflate_stream_batch": (i, [vp, sz, vpp, u64p, u32, vpp, u64p, u64p, u32p]),
        "sfh_last_stream_stats": (i, [vp, C.POINTER(C.c_float * STREAM_NSTAGES), C.POINTER(u64 * STREAM_NCOUNTS)]),
        # multi-GPU gather
        "sfh_gather_offsets": (i, [u64p, i, u64, u64, u64p]),
        "sfh_comm_ranks": (i, [vp, C.POINTER(i), C.POINTER(i)]),
        "sfh_gather_streams": (i, [vp, vp, i, vp, vp, vp, u64, u64, u64p, u64p, vp]),
        # the last call's index, the single-stream indexed decoder, checksums, measurement
        "sfh_last_block_bytes": (u32, [vp]),
        "sfh_last_decode_scratch_bytes": (sz, [vp]),
        "sfh_index_entries": (sz, [vp]),
        "sfh_copy_index": (i, [vp, vp, sz, i, vp]),
        "sfh_copy_subindex": (i, [vp, vp, sz, i, vp]),
        "sfh_decompress_device": (i, [vp, vp, sz, vp, vp, sz, vp, sz, u32, u32p, vp]),
        "sfh_decompress": (i, [vp, vp, sz, vp, vp, sz, vp, sz, u32, u32p]),
        "sfh_last_inflate_ms": (i, [vp, C.POINTER(C.c_float * INFLATE_NSTAGES)]),
        "sfh_inflate_stage_name": (C.c_char_p, [i]),
        "sfh_checksum_device": (i, [vp, vp, sz, u32, u32p, vp]),
        "sfh_crc32_combine": (u32, [u32, u32, u64]),
        "sfh_adler32_combine": (u32, [u32, u32, u64]),
        "sfh_set_profiling": (None, [vp, i]),
        "sfh_last_stage_ms": (i, [vp, C.POINTER(C.c_float * NSTAGES)]),
        "sfh_stage_name": (C.c_char_p, [i]),
        "sfh_debug_read": (i, [vp, i, vp, sz]),
        "sfh_lds_order_check": (i, [vp, u32, u32, u32, u64p, u64p]),
    }


PROTOTYPES = _prototypes()
EXPORTS = list(PROTOTYPES)  # every symbol include/starflate_hip.h declares
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
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = argtypes
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
