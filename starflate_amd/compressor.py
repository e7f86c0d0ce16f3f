"""Host plumbing over the C-ABI: device memory and streams come from torch, the
compression itself happens only in libstarflate_hip.so (HIP kernels, gfx950).

`compress()` is the sibling of the reference's
`starflate::decompress(src, dst) -> status` (/root/reference/src/decompress.hpp:63-71):
raw RFC 1951 out (or, with container="zlib"/"gzip", the RFC 1950 / RFC 1952 wrapper the
reference's fixture tool strips, tools/deflate_compress.py:8-13), caller-owned buffers,
integer status turned into an exception.
"""
import ctypes as C

import numpy as np

from . import _capi

CHUNK_BYTES = 32768
ITEM_NOT_INDEXABLE = _capi.ITEM_NOT_INDEXABLE  # a per-item status of decompress_any_batch: not block-flushed every 32 KiB


class StarflateError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"starflate_hip error {code}: {msg}")
        self.code = code


# ---- marshalling for the C-ABI: one definition per idiom ----
def _as_bytes(data):
    """any bytes-like object or array -> a 1-D contiguous uint8 array over the same bytes (an array of another dtype is
    converted value by value)"""
    return np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).ravel()


def _ptr(a):
    """the address of a host array, null when it is empty or None (a CUDA tensor needs no such helper: an empty tensor's
    data_ptr() is 0 already)"""
    return a.ctypes.data if a is not None and a.size else None


def _addr(a):
    """the address of an optional host array or CUDA tensor: null for None only"""
    if a is None:
        return None
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def _ptrs(arrays):
    """void*[k] of host arrays' addresses: one _ptr per item"""
    p = [_ptr(a) for a in arrays]
    return (C.c_void_p * len(p))(*p)


def _dptrs(tensors):
    """void*[k] of CUDA tensors' addresses: null for an empty tensor (its data_ptr() is 0) and for None"""
    p = [None if t is None else t.data_ptr() for t in tensors]
    return (C.c_void_p * len(p))(*p)


def _u64s(seq):
    """uint64_t[k] of a sequence of ints"""
    v = list(seq)
    return (C.c_uint64 * len(v))(*v)


def _host_dsts(sizes):
    """one host destination per size, of one byte at least: its address is never null"""
    return [np.empty(max(m, 1), dtype=np.uint8) for m in sizes]


def _device_array(t, dtype):
    """is t a contiguous CUDA tensor of that dtype ("int64", "int32")?"""
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == getattr(torch, dtype) and t.is_contiguous()


class Compressor:
    """One sfh_ctx (one GPU). Not thread-safe; use one per thread / per rank."""

    def __init__(self, device=0):
        self._lib = _capi.lib()
        n = self._lib.sfh_device_count()
        if n <= 0:
            raise StarflateError(-3, "no HIP device visible; the compressor has no CPU fallback")
        h = C.c_void_p()
        rc = self._lib.sfh_create(C.byref(h), int(device))
        if rc:
            raise StarflateError(rc, f"sfh_create(device={device}) failed")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sfh_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc:
            raise StarflateError(rc, self._lib.sfh_last_error(self._h).decode())

    def _check_tensor(self, t):
        import torch

        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 1 and t.is_contiguous()):
            raise ValueError("expected a contiguous 1-D uint8 CUDA tensor")
        if t.device.index != self.device:
            raise ValueError(f"tensor is on cuda:{t.device.index}, compressor on cuda:{self.device}")

    def _check_tensors(self, ts):
        for t in ts:
            self._check_tensor(t)

    def _stream(self, stream, device=None):
        """the void* of a stream handle; None: the current stream of this context's device (which _check_tensor pins every
        tensor of a call to), or of `device`"""
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(self.device if device is None else device).cuda_stream
        return C.c_void_p(stream)

    def _new(self, n, dtype="uint8", zeros=False):
        """a new tensor of n elements on this context's device; zeros: for what a call may leave unwritten"""
        import torch

        return (torch.zeros if zeros else torch.empty)(n, dtype=getattr(torch, dtype), device=torch.device("cuda", self.device))

    def _new_bytes(self, sizes):
        """new uint8 tensors of these sizes on this context's device (a batch's outputs: torch and the device looked up once)"""
        import torch

        dev = torch.device("cuda", self.device)
        return [torch.empty(m, dtype=torch.uint8, device=dev) for m in sizes]

    def _out(self, out, n, floor=1):
        """a call's output tensor: the caller's, or a new one of n bytes (`floor` at least)"""
        if out is None:
            out = self._new(max(int(n), floor))
        self._check_tensor(out)
        return out

    def _outs(self, outs, sizes, noun, name=None):
        """a call's output tensors, one per `noun` ("item", "range", "entry"): the caller's, or new ones of sizes[i] bytes (one
        at least).  sizes: one entry per noun; where the call names that argument (`name`), the bytes each tensor must hold."""
        if outs is None:
            outs = self._new_bytes(max(m, 1) for m in sizes)
        outs = list(outs)
        if name is None:
            if len(outs) != len(sizes):
                raise ValueError(f"outs must hold one tensor per {noun}")
        elif len(outs) != len(sizes) or any(o.numel() < m for o, m in zip(outs, sizes)):
            raise ValueError(f"outs must hold one tensor of at least {name}[i] bytes per {noun}")
        self._check_tensors(outs)
        return outs

    @staticmethod
    def compress_bound(n):
        return _capi.lib().sfh_compress_bound(int(n), 0)

    @staticmethod
    def _bound(n, container, block_bytes):
        """capacity of a single-stream compress call: container="dictzip" carries its table on top of compress_bound(n)
        (ValueError for what that container refuses: a block_bytes other than 0 and 32768, an input above 32762 * 32768 bytes)"""
        if container not in ("dictzip", _capi.COMPRESS_CONTAINER["dictzip"]):
            return Compressor.compress_bound(n)
        cap = _capi.lib().sfh_compress_bound_container(int(n), int(block_bytes), _capi.COMPRESS_CONTAINER["dictzip"])
        if not cap:
            raise ValueError('container="dictzip": block_bytes must be 0 or 32768 and the input at most 32762 * 32768 bytes')
        return cap

    # ---- host buffers (PCIe inclusive) ----
    def compress(self, data, strategy="auto", final_stream=True, lazy=True, stored_fast_path=True, container="raw",
                 block_bytes=0, effort="default"):
        src = _as_bytes(data)
        cap = self._bound(src.size, container, block_bytes)
        dst = np.empty(cap, dtype=np.uint8)
        out_n = C.c_size_t(0)
        opt = _capi.make_options(strategy, final_stream, lazy, stored_fast_path, container, block_bytes, effort)
        self._check(self._lib.sfh_compress(self._h, _ptr(src), src.size, dst.ctypes.data, cap, C.byref(out_n), C.byref(opt)))
        return dst[: out_n.value].tobytes()

    # ---- device buffers (torch uint8 CUDA tensors) ----
    def compress_tensor(self, src, out=None, strategy="auto", final_stream=True, lazy=True, stream=None,
                        stored_fast_path=True, container="raw", block_bytes=0, effort="default"):
        """src: 1-D uint8 tensor on this device. Returns (out tensor, stream byte count)."""
        self._check_tensor(src)
        cap = self._bound(src.numel(), container, block_bytes)
        out = self._out(out, cap)
        out_n = C.c_size_t(0)
        opt = _capi.make_options(strategy, final_stream, lazy, stored_fast_path, container, block_bytes, effort)
        self._check(self._lib.sfh_compress_device(self._h, src.data_ptr(), src.numel(), out.data_ptr(), out.numel(), C.byref(out_n),
                                                  C.byref(opt), self._stream(stream)))
        return out, out_n.value

    def _compress_async(self, fn, src, out, size_out, stream, **options):
        """compress_tensor_async and compress_bgzf_tensor_async: the checks, then the enqueue of fn with make_options(**options)"""
        import torch

        self._check_tensor(src)
        self._check_tensor(out)
        if size_out.dtype not in (torch.int64, torch.uint64) or not size_out.is_cuda:
            raise ValueError("size_out must be a 1-element int64 CUDA tensor")
        opt = _capi.make_options(**options)
        self._check(fn(self._h, src.data_ptr(), src.numel(), out.data_ptr(), out.numel(), size_out.data_ptr(), C.byref(opt),
                       self._stream(stream)))

    def compress_tensor_async(self, src, out, size_out, strategy="auto", final_stream=True, lazy=True, stream=None,
                              container="raw", block_bytes=0, effort="default"):
        """Enqueue only. size_out: 1-element int64 CUDA tensor receiving the stream size."""
        self._compress_async(self._lib.sfh_compress_device_async, src, out, size_out, stream, strategy=strategy,
                             final_stream=final_stream, lazy=lazy, container=container, block_bytes=block_bytes, effort=effort)

    # ---- BGZF, the blocked gzip of bgzip / htslib: one member per 32 KiB of input, then the EOF member (sfh_compress_bgzf*) ----
    @staticmethod
    def bgzf_bound(n):
        return _capi.lib().sfh_bgzf_bound(int(n))

    def compress_bgzf(self, data, strategy="auto", lazy=True, stored_fast_path=True, effort="default"):
        """Host buffers: bytes-like -> the BGZF file (bytes) that `bgzip -d`, htslib and gzip.decompress read."""
        src = _as_bytes(data)
        cap = self.bgzf_bound(src.size)
        dst = np.empty(cap, dtype=np.uint8)
        out_n = C.c_size_t(0)
        opt = _capi.make_options(strategy, True, lazy, stored_fast_path, "raw", 0, effort)
        self._check(self._lib.sfh_compress_bgzf(self._h, _ptr(src), src.size, dst.ctypes.data, cap, C.byref(out_n), C.byref(opt)))
        return dst[: out_n.value].tobytes()

    def compress_bgzf_tensor(self, src, out=None, strategy="auto", lazy=True, stream=None, stored_fast_path=True, effort="default",
                             **options):
        """src: 1-D uint8 tensor on this device.  Returns (out tensor, file byte count).  options: sfh_options fields the
        call refuses when set otherwise (container, final_stream, block_bytes), passed through for its refusals to be seen."""
        self._check_tensor(src)
        if out is None:
            out = self._new(self.bgzf_bound(src.numel()))
        self._check_tensor(out)
        out_n = C.c_size_t(0)
        opt = _capi.make_options(strategy, options.get("final_stream", True), lazy, stored_fast_path, options.get("container", "raw"),
                                 options.get("block_bytes", 0), effort)
        self._check(self._lib.sfh_compress_bgzf_device(self._h, src.data_ptr(), src.numel(), out.data_ptr(), out.numel(), C.byref(out_n),
                                                       C.byref(opt), self._stream(stream)))
        return out, out_n.value

    def compress_bgzf_tensor_async(self, src, out, size_out, strategy="auto", lazy=True, stream=None, effort="default"):
        """Enqueue only, no host synchronisation.  size_out: 1-element int64 CUDA tensor receiving the file's size."""
        self._compress_async(self._lib.sfh_compress_bgzf_device_async, src, out, size_out, stream, strategy=strategy,
                             final_stream=True, lazy=lazy, effort=effort)

    def bgzf_index(self, data):
        """The members of a BGZF file -> (member_off, out_off, info dict): bgzf_index() at module level, on the host."""
        return bgzf_index(data)

    def bgzf_index_tensor(self, src, stream=None):
        """src: 1-D uint8 tensor on this device holding a BGZF file -> (member_off, out_off: int64 tensors of members + 1
        entries on the device, info dict), found on the device by pointer jumping (sfh_bgzf_read_index_device).  A file that
        does not parse raises StarflateError with its DecompressStatus."""
        self._check_tensor(src)
        n = src.numel()
        info = _capi.BgzfInfo()
        cap = n // 26 + 2  # (a member is 26 bytes at least)
        moff, ooff = self._new(cap, "int64"), self._new(cap, "int64")
        self._check(self._lib.sfh_bgzf_read_index_device(self._h, src.data_ptr(), n, C.byref(info), moff.data_ptr(), ooff.data_ptr(), cap,
                                                         self._stream(stream)))
        if info.status:
            raise StarflateError(info.status, f"BGZF members: DecompressStatus {info.status}")
        m = info.members + 1
        return moff[:m].clone(), ooff[:m].clone(), _bgzf_info_dict(info)

    def decompress_bgzf(self, data):
        """Host buffers: a BGZF file -> (bytes, DecompressStatus int); every member's header, ISIZE and CRC-32 are verified.
        b"" when the status is not 0.  Every BGZF member is one segment of the indexed decoder: in its rows of 32 KiB when no
        member of the file holds more, else -- bgzip's and htslib's 65280 bytes, the format's 65536 -- in its wide rows of
        64 KiB (sfh_decompress_bgzf).  Only members claiming more than 65536 bytes, which is not BGZF, go through the stream
        decoder."""
        src = _as_bytes(data)
        try:
            _, out_off, _ = bgzf_index(src)
        except StarflateError as e:
            return b"", e.code
        cap = int(out_off[-1])
        dst = np.empty(max(cap, 1), dtype=np.uint8)
        got, st = C.c_uint64(0), C.c_uint32(0)
        self._check(self._lib.sfh_decompress_bgzf(self._h, _ptr(src), src.size, dst.ctypes.data, cap, C.byref(got), C.byref(st)))
        return (dst[: got.value].tobytes() if st.value == 0 else b""), int(st.value)

    def _decompress_bgzf_to(self, fn, src, total_n, out, stream):
        """decompress_bgzf_tensor and decompress_bgzf_wide_tensor: the two differ in the library entry"""
        self._check_tensor(src)
        out = self._out(out, total_n, 16)
        got, st = C.c_uint64(0), C.c_uint32(0)
        self._check(fn(self._h, src.data_ptr(), src.numel(), out.data_ptr(), int(total_n), C.byref(got), C.byref(st), self._stream(stream)))
        return out, int(got.value), int(st.value)

    def decompress_bgzf_tensor(self, src, total_n, out=None, stream=None):
        """src: 1-D uint8 tensor on this device holding a BGZF file of total_n output bytes (bgzf_index) -> (out tensor,
        bytes written, DecompressStatus int).  A member above 32 KiB raises StarflateError with code -8."""
        return self._decompress_bgzf_to(self._lib.sfh_decompress_bgzf_device, src, total_n, out, stream)

    def decompress_bgzf_wide_tensor(self, src, total_n, out=None, stream=None):
        """decompress_bgzf_tensor for every conforming BGZF file: members of up to 65536 bytes (bgzip and htslib write 65280)
        decode on the device, in the indexed decoder's wide rows (sfh_decompress_bgzf_wide_device); a file without a member
        above 32 KiB takes decompress_bgzf_tensor's path.  A member claiming more than 65536 bytes raises StarflateError with
        code -8."""
        return self._decompress_bgzf_to(self._lib.sfh_decompress_bgzf_wide_device, src, total_n, out, stream)

    # ---- BGZF random access: byte ranges of a BGZF file's output (sfh_decompress_bgzf_ranges*) ----
    def read_bgzf_ranges(self, bgzf, offsets, lengths, index=None):
        """Host buffers: byte ranges of what a BGZF file holds -> (list of bytes, None where a range's status is not 0; uint32
        status array).  index: bgzf_index()'s (member_off, out_off, info), reusable across calls; None: the members are walked on
        the host first (a file that does not parse gives every range the walk's status).  Of the file only the members that
        hold the ranges travel to the device; each is checked for its wrapper, its ISIZE and the size of its body.  No checksum
        is verified (a range cannot verify one).  Offsets from a tabix / BAI index: bgzf_voffsets_to_offsets."""
        src = _as_bytes(bgzf)
        offs, lens = [int(o) for o in offsets], [int(m) for m in lengths]
        if len(offs) != len(lens) or any(o < 0 or m < 0 for o, m in zip(offs, lens)):
            raise ValueError("offsets and lengths: one non-negative pair per range")
        if index is None:
            moff = ooff = info = None
        else:
            moff, ooff, info = _bgzf_index_args(index)
        return self._ranges_to_host(lens, lambda dp, st: self._lib.sfh_decompress_bgzf_ranges(
            self._h, _ptr(src), src.size, _addr(moff), _addr(ooff), C.byref(info) if info is not None else None, len(offs),
            _u64s(offs), _u64s(lens), dp, st))

    def _ranges_to_host(self, lens, call):
        """The host range readers' tail: a destination and a status per range, the library call -- call(the destinations'
        void*[k], the status array's address) -- and its results: (list of bytes, None where a range's status is not 0; uint32
        status array)."""
        k = len(lens)
        dsts = _host_dsts(lens)
        st = np.zeros(max(k, 1), dtype=np.uint32)
        self._check(call(_ptrs(dsts), st.ctypes.data))
        return [dsts[i][: lens[i]].tobytes() if st[i] == 0 else None for i in range(k)], st[:k]

    def read_bgzf_ranges_tensor(self, src, member_off, out_off, info, offsets, lengths, outs=None, stream=None):
        """Device buffers: src (1-D uint8 CUDA tensor holding a BGZF file) and bgzf_index_tensor()'s member_off, out_off (int64
        CUDA tensors of members + 1 entries) and info dict -> (outs, status).  outs: one uint8 tensor (or view, any alignment:
        slices of one packed buffer will do) of at least lengths[i] bytes per range, not overlapping (default: new ones);
        range i's bytes are outs[i][:lengths[i]]; status: an int32 tensor on the device, one DecompressStatus per range.  Two
        host synchronisations of `stream` (default: the current one): the planner's row total, then the end of the call."""
        self._check_tensor(src)
        if not (_device_array(member_off, "int64") and _device_array(out_off, "int64")):
            raise ValueError("member_off / out_off must be contiguous int64 CUDA tensors")
        binfo = _bgzf_info_struct(info)
        if member_off.numel() != binfo.members + 1 or out_off.numel() != binfo.members + 1:
            raise ValueError("member_off / out_off must hold members + 1 entries")
        offs, lens = [int(o) for o in offsets], [int(m) for m in lengths]
        if len(offs) != len(lens) or any(o < 0 or m < 0 for o, m in zip(offs, lens)):
            raise ValueError("offsets and lengths: one non-negative pair per range")
        k = len(offs)
        outs = self._outs(outs, lens, "range", "lengths")
        status = self._new(max(k, 1), "int32", zeros=True)
        self._check(self._lib.sfh_decompress_bgzf_ranges_device(
            self._h, src.data_ptr(), src.numel(), member_off.data_ptr(), out_off.data_ptr(), C.byref(binfo), k, _u64s(offs),
            _u64s(lens), _dptrs(outs), status.data_ptr(), self._stream(stream)))
        return outs, status[:k]

    # ---- many independent items, each its own stream, in one call (sfh_compress_batch*) ----
    def compress_batch(self, items, strategy="auto", final_stream=True, lazy=True, stored_fast_path=True, container="raw",
                       block_bytes=0, effort="default"):
        """Host buffers: a sequence of bytes-like items -> list of streams, item i's byte-identical to compress(items[i])
        with the same options (block_bytes=0 resolves per item)."""
        srcs = [_as_bytes(d) for d in items]
        k = len(srcs)
        caps = [self.compress_bound(a.size) for a in srcs]
        dsts = _host_dsts(caps)
        out_n = (C.c_uint64 * k)()
        opt = _capi.make_options(strategy, final_stream, lazy, stored_fast_path, container, block_bytes, effort)
        self._check(self._lib.sfh_compress_batch(self._h, k, _ptrs(srcs), _u64s(a.size for a in srcs), _ptrs(dsts), _u64s(caps), out_n,
                                                 C.byref(opt)))
        return [dsts[i][: out_n[i]].tobytes() for i in range(k)]

    def compress_batch_tensors(self, srcs, outs=None, stream=None, strategy="auto", final_stream=True, lazy=True,
                               stored_fast_path=True, container="raw", block_bytes=0, effort="default"):
        """Device buffers: 1-D uint8 tensors on this device -> (outs, sizes).  Enqueued on `stream` (default: the current
        one) without a host synchronisation; sizes is an int64 tensor on the device, valid once the stream gets there.
        outs default to new tensors of compress_bound(n) bytes."""
        srcs = list(srcs)
        self._check_tensors(srcs)
        if outs is None:
            outs = self._new_bytes(self.compress_bound(t.numel()) for t in srcs)
        outs = self._outs(outs, srcs, "item")
        sizes = self._new(len(srcs), "int64")  # (every entry is written by the call)
        opt = _capi.make_options(strategy, final_stream, lazy, stored_fast_path, container, block_bytes, effort)
        self._check(self._lib.sfh_compress_batch_device_async(
            self._h, len(srcs), _dptrs(srcs), _u64s(t.numel() for t in srcs), _dptrs(outs), _u64s(t.numel() for t in outs),
            sizes.data_ptr(), C.byref(opt), self._stream(stream)))
        return outs, sizes

    def last_batch_index(self):
        """Index of the last call when it was a compress batch: (index, subindex, block_bytes) -- the items' offsets
        flattened item after item (numpy uint64; item i of n_i bytes has max(1, ceil(n_i / 32768)) + 1 of them, relative to
        its own stream), their sub-index words (numpy uint32, 64 per segment) and every item's resolved block_bytes (numpy
        uint32): what decompress_batch takes."""
        items, entries = C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.sfh_batch_index_size(self._h, C.byref(items), C.byref(entries)))
        k, e = items.value, entries.value
        idx = np.empty(e, dtype=np.uint64)
        sub = np.empty(max((e - k) * _capi.SUBINDEX_WORDS, 1), dtype=np.uint32)
        bb = np.empty(max(k, 1), dtype=np.uint32)
        self._check(self._lib.sfh_copy_batch_index(self._h, idx.ctypes.data, sub.ctypes.data, bb.ctypes.data, 0, None))
        return idx, sub[: (e - k) * _capi.SUBINDEX_WORDS], bb[:k]

    # ---- ZIP archives ----
    @staticmethod
    def zip_bound(sizes, name_lens):
        return zip_bound(sizes, name_lens)

    def compress_zip(self, items, strategy="auto", lazy=True, stored_fast_path=True, block_bytes=0, effort="default"):
        """{name: bytes} or [(name, bytes)] -> one ZIP archive (bytes) of deflated entries, in that order; entry i's body is
        byte for byte compress_batch(...)[i] with container="raw" and the same options."""
        names, srcs = _zip_items(items)
        k = len(srcs)
        n = _u64s(a.size for a in srcs)
        ln = (C.c_uint32 * k)(*[len(b) for b in names])
        cap = self._lib.sfh_zip_bound(k, n, ln)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        np_ = (C.c_char_p * k)(*names)
        got = C.c_size_t()
        opt = _capi.make_options(strategy, True, lazy, stored_fast_path, "raw", block_bytes, effort)
        self._check(self._lib.sfh_compress_zip(self._h, k, _ptrs(srcs), n, np_, ln, out.ctypes.data, cap, C.byref(got), C.byref(opt)))
        return out[: got.value].tobytes()

    def compress_zip_tensors(self, names, srcs, out=None, stream=None, strategy="auto", lazy=True, stored_fast_path=True,
                             block_bytes=0, effort="default"):
        """Device buffers: names (str or bytes) and 1-D uint8 tensors on this device -> (out, size).  Enqueued on `stream`
        (default: the current one); size is an int64 tensor of one element on the device, valid once the stream gets there.
        out defaults to a new tensor of zip_bound bytes."""
        names = [b.encode("utf-8") if isinstance(b, str) else bytes(b) for b in names]
        srcs = list(srcs)
        if len(names) != len(srcs):
            raise ValueError("one name per item")
        self._check_tensors(srcs)
        k = len(srcs)
        n = _u64s(t.numel() for t in srcs)
        ln = (C.c_uint32 * k)(*[len(b) for b in names])
        if out is None:
            out = self._new(self._lib.sfh_zip_bound(k, n, ln))
        self._check_tensor(out)
        size = self._new(1, "int64")
        np_ = (C.c_char_p * k)(*names)
        opt = _capi.make_options(strategy, True, lazy, stored_fast_path, "raw", block_bytes, effort)
        self._check(self._lib.sfh_compress_zip_device_async(self._h, k, _dptrs(srcs), n, np_, ln, out.data_ptr(), out.numel(),
                                                            size.data_ptr(), C.byref(opt), self._stream(stream)))
        return out, size

    def zip_index_tensor(self, src, stream=None):
        """The entry table of a ZIP archive on this device -> (info dict, entries): entries is a numpy structured array
        (ZIP_ENTRY_DTYPE), on the host.  A file whose index fails: its status in info, no entries."""
        self._check_tensor(src)
        s = self._stream(stream)
        info = _capi.ZipInfo()
        rc = self._lib.sfh_zip_read_index_device(self._h, src.data_ptr(), src.numel(), C.byref(info), None, 0, s)
        ents = np.zeros(info.entries, ZIP_ENTRY_DTYPE)
        if rc == -2:
            rc = self._lib.sfh_zip_read_index_device(self._h, src.data_ptr(), src.numel(), C.byref(info), ents.ctypes.data, ents.size, s)
        self._check(rc)
        return _zip_info_dict(info), ents

    def decompress_zip_tensors(self, src, entries, outs=None, stream=None):
        """Entries (rows of a zip_index table, any subset in any order) of the archive `src` on this device -> (outs, statuses).
        outs default to views of one packed buffer in which every entry starts 16-byte aligned (the layout of out_off for the
        whole table); statuses: numpy uint32, 0 = decoded and its CRC-32 verified."""
        self._check_tensor(src)
        ents = np.ascontiguousarray(entries, dtype=ZIP_ENTRY_DTYPE).ravel()
        k = ents.size
        if outs is None:
            offs = np.concatenate([[0], np.cumsum((ents["usize"].astype(np.uint64) + np.uint64(15)) & ~np.uint64(15))]).astype(np.uint64)
            buf = self._new(max(int(offs[-1]), 16))
            outs = [buf[int(offs[i]): int(offs[i]) + int(ents["usize"][i])] for i in range(k)]
        outs = self._outs(outs, ents, "entry")
        st = np.zeros(k, np.uint32)
        self._check(self._lib.sfh_decompress_zip_device(self._h, src.data_ptr(), src.numel(), ents.ctypes.data, k, _dptrs(outs),
                                                        _u64s(t.numel() for t in outs), st.ctypes.data, self._stream(stream)))
        return outs, st

    def decompress_zip(self, data, names=None):
        """A ZIP archive (bytes-like) -> ({name: bytes}, statuses): every entry, or those called `names`; an entry whose
        status is not 0 maps to None.  Raises StarflateError when the archive's index does not parse."""
        src = _as_bytes(data)
        info, ents = zip_index(src)
        if info["status"]:
            raise StarflateError(info["status"], f"ZIP index: DecompressStatus {info['status']}")
        all_names = zip_names(src, ents)
        if names is not None:
            pick = [all_names.index(b if isinstance(b, str) else b.decode("utf-8")) for b in names]
            ents = ents[pick]
            all_names = [all_names[i] for i in pick]
        k = ents.size
        dsts = [np.empty(int(e["usize"]), dtype=np.uint8) for e in ents]
        st = np.zeros(k, np.uint32)
        self._check(self._lib.sfh_decompress_zip(self._h, src.ctypes.data, src.size, ents.ctypes.data, k, _ptrs(dsts),
                                                 _u64s(d.size for d in dsts), st.ctypes.data))
        return {nm: (d.tobytes() if not s else None) for nm, d, s in zip(all_names, dsts, st)}, st

    # ---- block index + GPU decompress (the reference's decompress(), /root/reference/src/decompress.hpp:63-71,
    #      for streams whose independently decodable 32 KiB segments are known) ----
    def last_block_bytes(self):
        """Strip size the last compress call used (block_bytes after defaulting)."""
        return int(self._lib.sfh_last_block_bytes(self._h))

    def last_error(self):
        """sfh_last_error: what the last failing call (or the last decode with a non-zero status) said."""
        e = self._lib.sfh_last_error(self._h)
        return e.decode() if e else ""

    def last_decode_scratch_bytes(self):
        """Bytes of token scratch the last decompress call used: one batch of whole strips (at most 4 GiB), whatever its size."""
        return int(self._lib.sfh_last_decode_scratch_bytes(self._h))

    def last_index(self, device=None):
        """Index of the last compress call: segments + 1 stream offsets.  numpy uint64 array, or (device given)
        an int64 tensor on that CUDA device."""
        n = self._lib.sfh_index_entries(self._h)
        if n == 0:
            raise StarflateError(-1, "no compress call on this context yet")
        if device is None:
            idx = np.empty(n, dtype=np.uint64)
            self._check(self._lib.sfh_copy_index(self._h, idx.ctypes.data, n, 0, None))
            return idx
        import torch

        idx = torch.empty(n, dtype=torch.int64, device=device)
        self._check(self._lib.sfh_copy_index(self._h, idx.data_ptr(), n, 1, self._stream(None, idx.device)))
        return idx

    def last_subindex(self, device=None):
        """Sub-index of the last compress call (32 x {bit offset, tokens before} per segment): numpy uint32
        array [segments, 32, 2], or (device given) an int32 tensor of that shape on the CUDA device."""
        nseg = self._lib.sfh_index_entries(self._h) - 1
        if nseg < 0:
            raise StarflateError(-1, "no compress call on this context yet")
        words = nseg * _capi.SUBINDEX_WORDS
        if device is None:
            sub = np.empty((nseg, 32, 2), dtype=np.uint32)
            self._check(self._lib.sfh_copy_subindex(self._h, sub.ctypes.data, words, 0, None))
            return sub
        import torch

        sub = torch.empty((nseg, 32, 2), dtype=torch.int32, device=device)
        self._check(self._lib.sfh_copy_subindex(self._h, sub.data_ptr(), words, 1, self._stream(None, sub.device)))
        return sub

    def decompress_tensor(self, stream, index, out_n, out=None, hip_stream=None, subindex=None, *, block_bytes):
        """stream: 1-D uint8 CUDA tensor (exactly the compressed bytes); index: int64 CUDA tensor of segments + 1
        offsets; subindex: optional int32 CUDA tensor [segments, 32, 2] (last_subindex); out_n: decompressed size;
        block_bytes (required): the strip size the stream was written with (last_block_bytes() of the compressing call --
        compress*() defaults to strips of up to 256 KiB, so there is no safe default here; 32768 = independent blocks).
        Returns (out tensor, DecompressStatus int, 0 = Success)."""
        import torch

        self._check_tensor(stream)
        if not _device_array(index, "int64"):
            raise ValueError("index must be a contiguous int64 CUDA tensor")
        nseg = index.numel() - 1
        out = self._out(out, out_n)
        if out.numel() < out_n:
            raise ValueError("out is smaller than out_n")
        st = C.c_uint32(0)
        if subindex is not None and not (subindex.is_cuda and subindex.dtype == torch.int32 and subindex.is_contiguous()
                                         and subindex.numel() == nseg * _capi.SUBINDEX_WORDS):
            raise ValueError("subindex must be a contiguous int32 CUDA tensor of segments * 64 words")
        self._check(self._lib.sfh_decompress_device(self._h, stream.data_ptr(), stream.numel(), index.data_ptr(), _addr(subindex), nseg,
                                                    out.data_ptr() if out_n else None, int(out_n), int(block_bytes),
                                                    C.byref(st), self._stream(hip_stream)))
        return out[:out_n], st.value

    def decompress(self, data, index, out_n, subindex=None, *, block_bytes):
        """Host buffers: bytes-like stream + numpy uint64 index [+ numpy uint32 sub-index] -> (bytes, DecompressStatus int)."""
        src = _as_bytes(data)
        idx = np.ascontiguousarray(index, dtype=np.uint64)
        dst = np.empty(max(int(out_n), 1), dtype=np.uint8)
        st = C.c_uint32(0)
        sub = None if subindex is None else np.ascontiguousarray(subindex, dtype=np.uint32)
        if sub is not None and sub.size != (idx.size - 1) * _capi.SUBINDEX_WORDS:
            raise ValueError("subindex must hold segments * 64 words")
        self._check(self._lib.sfh_decompress(self._h, src.ctypes.data, src.size, idx.ctypes.data, _addr(sub), idx.size - 1,
                                             dst.ctypes.data if out_n else None, int(out_n), int(block_bytes), C.byref(st)))
        return (dst[:out_n].tobytes() if st.value == 0 else b""), st.value

    # ---- one stream given alone: the segment index recovered on the GPU ----
    def recover_index(self, stream, out_n, container="raw", hip_stream=None):
        """stream: 1-D uint8 CUDA tensor (exactly the compressed bytes), out_n: its decoded size -> (index int64 CUDA tensor of
        segments + 1 offsets, depends uint8 CUDA tensor: 1 where a match of the segment reaches before its first byte).
        A stream that is not block-flushed every 32 KiB raises StarflateError with code -8 (SFH_E_NOT_INDEXABLE)."""
        self._check_tensor(stream)
        nseg = max(1, -(-int(out_n) // CHUNK_BYTES))
        index, depends = self._new(nseg + 1, "int64"), self._new(nseg)
        self._check(self._lib.sfh_recover_index_device(self._h, stream.data_ptr(), stream.numel(), _container(container),
                                                       int(out_n), index.data_ptr(), nseg, depends.data_ptr(), self._stream(hip_stream)))
        return index, depends

    def decompress_any_tensor(self, stream, out_n=None, container="raw", out=None, hip_stream=None):
        """stream: 1-D uint8 CUDA tensor; out_n: decoded size (None: gzip's ISIZE) -> (out tensor, DecompressStatus int).
        No index, no block_bytes: the stream's own flush markers give the segments.  Not block-flushed: StarflateError -8."""
        self._check_tensor(stream)
        kind = _container(container)
        if out_n is None:
            out_n = _isize(stream[-4:].cpu().numpy().tobytes() if stream.numel() >= 4 else b"", kind)
        out = self._out(out, out_n)
        if out.numel() < out_n:
            raise ValueError("out is smaller than out_n")
        st = C.c_uint32(0)
        self._check(self._lib.sfh_decompress_any_device(self._h, stream.data_ptr(), stream.numel(), kind,
                                                        out.data_ptr() if out_n else None, int(out_n), C.byref(st),
                                                        self._stream(hip_stream)))
        return out[:out_n], st.value

    def decompress_any(self, data, out_n=None, container="raw"):
        """Host buffers: a bytes-like raw / zlib / gzip stream -> (bytes, DecompressStatus int), on the GPU without an index;
        out_n None: gzip's ISIZE.  Not block-flushed every 32 KiB: StarflateError -8 (decompress() falls back instead)."""
        src = _as_bytes(data)
        kind = _container(container)
        n = _isize(src[-4:].tobytes(), kind) if out_n is None else int(out_n)
        dst = np.empty(max(n, 1), dtype=np.uint8)
        st = C.c_uint32(0)
        self._check(self._lib.sfh_decompress_any(self._h, _ptr(src), src.size, kind, dst.ctypes.data, n, n, None, C.byref(st)))
        return (dst[:n].tobytes() if st.value == 0 else b""), st.value

    def last_recover_stats(self):
        """The last recover / decompress_any call: {"scan_ms", "walk_ms"} (with profiling on), {"nodes", "rows"}."""
        ms = (C.c_float * 2)()
        cnt = (C.c_uint64 * 2)()
        self._check(self._lib.sfh_last_recover_stats(self._h, C.byref(ms), C.byref(cnt)))
        return {"scan_ms": ms[0], "walk_ms": ms[1], "nodes": cnt[0], "rows": cnt[1]}

    # ---- one stream without side information or flush points (sfh_inflate_stream*) ----
    def decompress_stream_tensor(self, stream, out_n=None, container="raw", out=None, hip_stream=None):
        """stream: 1-D uint8 CUDA tensor -> (out tensor of the decoded bytes, DecompressStatus int), decoded on the GPU from
        speculative block starts (no index, no flush points needed).  out_n: the output capacity (None: a size query first,
        then exactly the output size -- gzip: ISIZE where that is more, the room a gzip decode asks for whatever its body
        produces); out: a uint8 CUDA tensor of at least out_n bytes.  Synchronises the stream."""
        self._check_tensor(stream)
        kind = _stream_container(container)
        s = self._stream(hip_stream)
        st, n = C.c_uint32(0), C.c_uint64(0)
        src = stream.data_ptr()
        if out_n is None:
            self._check(self._lib.sfh_inflate_stream_device(self._h, src, stream.numel(), kind, None, 0, C.byref(n), C.byref(st), s))
            if st.value:
                return stream[:0], st.value
            out_n = max(n.value, _gzip_room(stream, kind))
        out_n = int(out_n)
        out = self._out(out, out_n)
        if out.numel() < out_n or out.numel() == 0:
            raise ValueError("out is smaller than out_n (or empty)")
        # (always a real pointer: a null dst with a capacity of 0 is the C interface's size query, which checks no trailer)
        self._check(self._lib.sfh_inflate_stream_device(self._h, src, stream.numel(), kind, out.data_ptr(), out_n, C.byref(n),
                                                        C.byref(st), s))
        return (out[: n.value] if st.value == 0 else out[:0]), st.value

    def decompress_stream(self, data, out_n=None, container="raw"):
        """Host buffers: a bytes-like raw / zlib / gzip stream (one member) -> (bytes, DecompressStatus int), on the GPU with no
        index and no flush points.  out_n: the output capacity (None: a size query first, then the queried size -- gzip: ISIZE
        where that is more, so that a trailer that claims more than the body gives is Error, as with any dst that holds
        ISIZE bytes).  b"" unless the status is 0."""
        src = _as_bytes(data)
        kind = _stream_container(container)
        st, n = C.c_uint32(0), C.c_uint64(0)
        sp = _ptr(src)
        if out_n is None:
            self._check(self._lib.sfh_inflate_stream(self._h, sp, src.size, kind, None, 0, C.byref(n), C.byref(st)))
            if st.value:
                return b"", st.value
            out_n = max(n.value, _gzip_room(src, kind))
        out_n = int(out_n)
        dst = np.empty(max(out_n, 1), dtype=np.uint8)
        self._check(self._lib.sfh_inflate_stream(self._h, sp, src.size, kind, dst.ctypes.data, out_n, C.byref(n), C.byref(st)))
        return (dst[: n.value].tobytes() if st.value == 0 else b""), st.value

    def last_stream_stats(self):
        """The last decompress_stream* call: per-stage ms (with profiling on, else zeros) and the chunk counts."""
        ms = (C.c_float * _capi.STREAM_NSTAGES)()
        cnt = (C.c_uint64 * _capi.STREAM_NCOUNTS)()
        self._check(self._lib.sfh_last_stream_stats(self._h, C.byref(ms), C.byref(cnt)))
        names = ("find_ms", "count_ms", "write_ms", "resolve_ms", "checksum_ms")
        keys = ("chunks", "candidates", "confirmed", "repair_rounds", "longest_chunk", "scratch_bytes")
        return {**{k: ms[i] for i, k in enumerate(names)}, **{k: cnt[i] for i, k in enumerate(keys)}}

    # ---- many streams without side information or flush points in one call (sfh_inflate_stream_batch*) ----
    def decompress_stream_batch(self, streams, sizes=None, container="raw"):
        """Host buffers: bytes-like raw / zlib / gzip streams (one member each) -> (list of bytes, list of DecompressStatus ints),
        every item exactly what decompress_stream gives for it alone.  sizes: the output capacities (None: a size-query call
        first, then the queried sizes -- gzip: ISIZE where that is more).  An item whose status is not 0 comes back as b""."""
        srcs, n, caps, kind = _stream_batch_args(streams, sizes, container)
        k = len(srcs)
        sp = _ptrs(srcs)
        out_n = (C.c_uint64 * k)()
        st = (C.c_uint32 * k)()
        if caps is None:
            self._check(self._lib.sfh_inflate_stream_batch(self._h, k, sp, n, kind, None, None, out_n, st))
            caps = [max(int(out_n[i]), _gzip_room(srcs[i], kind)) if st[i] == 0 else 0 for i in range(k)]
            live = [st[i] == 0 for i in range(k)]
            first = [int(st[i]) for i in range(k)]
        else:
            live, first = [True] * k, [0] * k
        dsts = _host_dsts(caps)
        # (an item that failed its size query is asked again as a query of its own: a null destination)
        dp = _ptrs(d if ok else None for d, ok in zip(dsts, live))
        if k:
            self._check(self._lib.sfh_inflate_stream_batch(self._h, k, sp, n, kind, dp, _u64s(caps), out_n, st))
        stats = [int(st[i]) if live[i] else first[i] for i in range(k)]
        return [dsts[i][: out_n[i]].tobytes() if stats[i] == 0 else b"" for i in range(k)], stats

    def decompress_stream_batch_tensors(self, streams, sizes=None, container="raw", outs=None, hip_stream=None):
        """Device buffers: 1-D uint8 CUDA tensors -> (list of output tensors, list of DecompressStatus ints); each output is
        exactly the item's decoded bytes (empty unless its status is 0).  sizes: the output capacities (None: a size-query
        call first, then the queried sizes -- gzip: ISIZE where that is more); outs: one uint8 CUDA tensor of at least sizes[i] bytes per item (default: new ones).  Synchronises the
        stream."""
        streams = list(streams)
        self._check_tensors(streams)
        kind = _stream_container(container)
        k = len(streams)
        s = self._stream(hip_stream)
        sp = _dptrs(streams)
        n = _u64s(t.numel() for t in streams)
        out_n = (C.c_uint64 * k)()
        st = (C.c_uint32 * k)()
        live, first = [True] * k, [0] * k
        if sizes is None:
            self._check(self._lib.sfh_inflate_stream_batch_device(self._h, k, sp, n, kind, None, None, out_n, st, s))
            sizes = [max(int(out_n[i]), _gzip_room(streams[i], kind)) if st[i] == 0 else 0 for i in range(k)]
            live = [st[i] == 0 for i in range(k)]
            first = [int(st[i]) for i in range(k)]
        caps = [int(m) for m in sizes]
        if len(caps) != k or any(m < 0 for m in caps):
            raise ValueError("sizes must hold one non-negative capacity per stream")
        outs = self._outs(outs, caps, "item", "sizes")
        dp = _dptrs(o if ok else None for o, ok in zip(outs, live))
        if k:
            self._check(self._lib.sfh_inflate_stream_batch_device(self._h, k, sp, n, kind, dp,
                                                                  _u64s(m if ok else 0 for m, ok in zip(caps, live)), out_n, st, s))
        stats = [int(st[i]) if live[i] else first[i] for i in range(k)]
        return [outs[i][: out_n[i]] if stats[i] == 0 else outs[i][:0] for i in range(k)], stats

    # ---- many block-flushed streams with no side information in one call (sfh_decompress_any_batch*) ----
    def decompress_any_batch(self, streams, sizes=None, container="raw"):
        """Host buffers: bytes-like raw / zlib / gzip streams, each block-flushed every 32 KiB (what compress_batch writes) ->
        (list of bytes, list of statuses), every item exactly what decompress_any gives for it alone.  sizes: the decoded
        sizes (None: gzip's ISIZE).  A status is a DecompressStatus, or ITEM_NOT_INDEXABLE for an item that is not
        block-flushed (decompress_stream_batch decodes those).  An item whose status is not 0 comes back as b""."""
        srcs, n, want, caps, kind = _any_batch_args(streams, sizes, container)
        k = len(srcs)
        if k == 0:
            return [], []
        dsts = _host_dsts(caps)
        out_n = (C.c_uint64 * k)()
        st = (C.c_uint32 * k)()
        self._check(self._lib.sfh_decompress_any_batch(self._h, k, _ptrs(srcs), n, kind, _ptrs(dsts), _u64s(caps), want, out_n, st))
        return [dsts[i][: out_n[i]].tobytes() if st[i] == 0 else b"" for i in range(k)], [int(v) for v in st]

    def decompress_any_batch_tensors(self, streams, sizes=None, container="raw", outs=None, hip_stream=None):
        """Device buffers: 1-D uint8 CUDA tensors -> (list of output tensors, list of statuses); each output is the item's
        decoded bytes (empty unless its status is 0).  sizes: the decoded sizes (None: gzip's ISIZE, read on the device; outs
        is then required and gives the capacities); outs: one uint8 CUDA tensor (16-byte aligned) of at least sizes[i] bytes
        per item (default: new ones).  Synchronises the stream."""
        streams = list(streams)
        kind = _container(container)
        k = len(streams)
        if sizes is None:
            if kind != 2:
                raise ValueError("sizes is required unless container='gzip' (whose trailer carries ISIZE)")
            if outs is None:
                raise ValueError("sizes=None on device tensors needs outs (the capacities)")
            want = [_capi.SIZE_FROM_TRAILER] * k
        else:
            want = [int(m) for m in sizes]
            if len(want) != k or any(m < 0 or m > (1 << 44) for m in want):
                raise ValueError("sizes must hold one size in [0, 2^44] per stream")
        self._check_tensors(streams)
        # (sizes=None: outs give the capacities, none of which is too small to ask the trailer)
        outs = self._outs(outs, want if sizes is not None else [0] * k, "item", "sizes")
        if k == 0:
            return [], []
        out_n = (C.c_uint64 * k)()
        st = (C.c_uint32 * k)()
        self._check(self._lib.sfh_decompress_any_batch_device(
            self._h, k, _dptrs(streams), _u64s(t.numel() for t in streams), kind, _dptrs(outs), _u64s(o.numel() for o in outs),
            _u64s(want), out_n, st, self._stream(hip_stream)))
        return [outs[i][: out_n[i]] if st[i] == 0 else outs[i][:0] for i in range(k)], [int(v) for v in st]

    def recover_index_batch(self, streams, sizes, container="raw", hip_stream=None):
        """streams: 1-D uint8 CUDA tensors, sizes: their decoded sizes -> (index: one int64 CUDA tensor, last_batch_index()'s
        flat layout -- item i's segments + 1 offsets behind those of the items before it -- and a list of statuses: 0, or
        ITEM_NOT_INDEXABLE for an item that is not block-flushed every 32 KiB, whose entries are 0)."""
        streams = list(streams)
        kind = _container(container)
        want = [int(m) for m in sizes]
        k = len(streams)
        if len(want) != k or any(m < 0 or m > (1 << 44) for m in want):
            raise ValueError("sizes must hold one size in [0, 2^44] per stream")
        self._check_tensors(streams)
        entries = sum(max(1, -(-m // CHUNK_BYTES)) + 1 for m in want)
        index = self._new(max(entries, 1), "int64", zeros=True)
        st = (C.c_uint32 * max(k, 1))()
        if k:
            self._check(self._lib.sfh_recover_index_batch_device(self._h, k, _dptrs(streams), _u64s(t.numel() for t in streams), kind,
                                                                 _u64s(want), index.data_ptr(), st, self._stream(hip_stream)))
        return index[:entries], [int(st[i]) for i in range(k)]

    # ---- many independent streams, each decoded into its own buffer, in one call (sfh_decompress_batch*) ----
    def decompress_batch(self, streams, sizes, index=None, subindex=None, block_bytes=None, container="raw"):
        """Host buffers: bytes-like streams and their decoded sizes -> (list of bytes, list of DecompressStatus ints).  index /
        subindex / block_bytes: last_batch_index()'s layout (flattened, item after item), or index=None when every size is at
        most 32768 (each stream one segment: pages from other tools).  An item whose status is not 0 comes back as b""."""
        srcs, n, dst_n, idx, sub, bb, kind = _batch_inflate_args(streams, sizes, index, subindex, block_bytes, container)
        k = len(srcs)
        dsts = _host_dsts(dst_n)
        st = np.zeros(max(k, 1), dtype=np.uint32)
        self._check(self._lib.sfh_decompress_batch(self._h, k, _ptrs(srcs), n, _addr(idx), _addr(sub), _ptrs(dsts), _u64s(dst_n),
                                                   _addr(bb), kind, st.ctypes.data))
        return [dsts[i][: dst_n[i]].tobytes() if st[i] == 0 else b"" for i in range(k)], [int(v) for v in st[:k]]

    def decompress_batch_tensors(self, streams, sizes, index=None, subindex=None, block_bytes=None, container="raw",
                                 outs=None, stream=None):
        """Device buffers: 1-D uint8 CUDA tensors -> (outs, status).  Enqueued on `stream` (default: the current one) without
        a host synchronisation.  index: int64 CUDA tensor, subindex: int32 CUDA tensor (last_batch_index()'s layout), or
        None; block_bytes: a host sequence.  outs: one uint8 tensor per item of at least sizes[i] bytes (default: new ones;
        each item's decoded bytes are outs[i][:sizes[i]]); status: an int32 tensor on the device, one DecompressStatus per item."""
        streams = list(streams)
        self._check_tensors(streams)
        dst_n, bb, kind = _batch_lengths(len(streams), sizes, None if index is None else index.numel(),
                                         None if subindex is None else subindex.numel(), block_bytes, container)
        k = len(streams)
        if not ((index is None or _device_array(index, "int64")) and (subindex is None or _device_array(subindex, "int32"))):
            raise ValueError("index / subindex must be contiguous int64 / int32 CUDA tensors")
        outs = self._outs(outs, dst_n, "item", "sizes")
        status = self._new(max(k, 1), "int32")
        self._check(self._lib.sfh_decompress_batch_device_async(
            self._h, k, _dptrs(streams), _u64s(t.numel() for t in streams), _addr(index), _addr(subindex), _dptrs(outs), _u64s(dst_n),
            _addr(bb), kind, status.data_ptr(), self._stream(stream)))
        return outs, status[:k]

    # ---- random access: byte ranges of one indexed stream's output (sfh_decompress_range*) ----
    def decompress_range(self, data, index, total_n, offset, length, subindex=None, *, block_bytes):
        """Host buffers: output bytes [offset, offset + length) of an indexed stream -> (bytes, DecompressStatus int); b"" when
        the status is not 0.  Only the range's decode span is uploaded and decoded (decompress_ranges)."""
        outs, st = self.decompress_ranges(data, index, total_n, [offset], [length], subindex, block_bytes=block_bytes)
        return (outs[0] if outs[0] is not None else b""), int(st[0])

    def decompress_ranges(self, data, index, total_n, offsets, lengths, subindex=None, *, block_bytes):
        """Host buffers: bytes-like stream, numpy uint64 index of segments + 1 entries [+ uint32 sub-index], the stream's whole
        output size and the ranges -> (list of bytes, None where a range's status is not 0; uint32 status array).  Of the
        stream only the ranges' decode spans travel to the device: from the start of the strip (block_bytes, required as in
        decompress) holding a range's first byte to the segment holding its last."""
        src = _as_bytes(data)
        idx = np.ascontiguousarray(index, dtype=np.uint64).ravel()
        sub = None if subindex is None else np.ascontiguousarray(subindex, dtype=np.uint32).ravel()
        total_n, offs, lens, nseg = _range_lengths(total_n, offsets, lengths, idx.size, None if sub is None else sub.size, block_bytes)
        return self._ranges_to_host(lens, lambda dp, st: self._lib.sfh_decompress_ranges(
            self._h, _ptr(src), src.size, idx.ctypes.data, _addr(sub), nseg, total_n, int(block_bytes), len(offs), _u64s(offs),
            _u64s(lens), dp, st))

    def decompress_ranges_tensors(self, stream, index, total_n, offsets, lengths, outs=None, subindex=None, hip_stream=None, *,
                                  block_bytes):
        """Device buffers: stream (1-D uint8 CUDA tensor), index (int64 CUDA tensor of segments + 1 offsets), optional
        subindex (int32 CUDA tensor of segments * 64 words) -> (outs, status).  Enqueued on hip_stream (default: the current
        one) without a host synchronisation.  outs: one uint8 tensor (or view, any alignment: slices of one packed buffer will
        do) of at least lengths[i] bytes per range, not overlapping (default: new ones); range i's bytes are
        outs[i][:lengths[i]]; status: an int32 tensor on the device, one DecompressStatus per range."""
        self._check_tensor(stream)
        if not ((index is None or _device_array(index, "int64")) and (subindex is None or _device_array(subindex, "int32"))):
            raise ValueError("index / subindex must be contiguous int64 / int32 CUDA tensors")
        if index is None:
            raise ValueError("an index is required")
        total_n, offs, lens, nseg = _range_lengths(total_n, offsets, lengths, index.numel(),
                                                   None if subindex is None else subindex.numel(), block_bytes)
        k = len(offs)
        outs = self._outs(outs, lens, "range", "lengths")
        status = self._new(max(k, 1), "int32")
        self._check(self._lib.sfh_decompress_ranges_device_async(
            self._h, stream.data_ptr(), stream.numel(), index.data_ptr(), _addr(subindex), nseg, total_n, int(block_bytes), k,
            _u64s(offs), _u64s(lens), _dptrs(outs), status.data_ptr(), self._stream(hip_stream)))
        return outs, status[:k]

    # ---- seekable gzip: files written with container="dictzip", read with nothing but their bytes (sfh_decompress_dz*) ----
    def decompress_dictzip(self, data):
        """Host buffers: a dictzip file of 32 KiB chunks -> (bytes, DecompressStatus int), decoded with the index its own header
        carries; header, ISIZE and CRC-32 are verified.  b"" when the status is not 0.  A gzip file without such a table raises
        StarflateError with code -8 (SFH_E_NOT_INDEXABLE)."""
        src = _as_bytes(data)
        try:
            _, cap = dictzip_index(src)  # the header first: the output is sized from an ISIZE that agrees with the table
        except StarflateError as e:
            if e.code < 0:
                raise
            return b"", e.code
        dst = np.empty(max(cap, 1), dtype=np.uint8)
        got, st = C.c_uint64(0), C.c_uint32(0)
        self._check(self._lib.sfh_decompress_dz(self._h, src.ctypes.data, src.size, dst.ctypes.data, cap, C.byref(got), C.byref(st)))
        return (dst[: got.value].tobytes() if st.value == 0 else b""), int(st.value)

    def read_ranges(self, data, offsets, lengths):
        """Host buffers: byte ranges of what a dictzip file of 32 KiB chunks holds, given nothing but the file -> (list of bytes,
        None where a range's status is not 0; uint32 status array).  The header is read on the host; of the file only the
        chunks that hold the ranges travel to the device (decompress_ranges).  No checksum is verified (a range cannot
        verify one)."""
        return self._read_ranges(*_dz_range_args(data, offsets, lengths))

    def _read_ranges(self, src, offs, lens):
        return self._ranges_to_host(lens, lambda dp, st: self._lib.sfh_decompress_dz_ranges(
            self._h, src.ctypes.data, src.size, len(offs), _u64s(offs), _u64s(lens), dp, st))

    def inflate_ms(self):
        ms = (C.c_float * _capi.INFLATE_NSTAGES)()
        self._check(self._lib.sfh_last_inflate_ms(self._h, C.byref(ms)))
        return {self._lib.sfh_inflate_stage_name(k).decode(): float(ms[k]) for k in range(_capi.INFLATE_NSTAGES)}

    def checksum_tensor(self, src, kind, stream=None):
        """kind "zlib" -> Adler-32, "gzip" -> CRC-32 of a 1-D uint8 tensor on this device (GPU kernels)."""
        self._check_tensor(src)
        out = C.c_uint32(0)
        self._check(self._lib.sfh_checksum_device(self._h, src.data_ptr(), src.numel(), _capi.CONTAINER[kind], C.byref(out),
                                                  self._stream(stream)))
        return out.value

    # ---- measurement / inspection ----
    def lds_order_check(self, op, blocks=256, iters=50):
        """sfh_lds_order_check: does the LDS execute a returning atomic's lanes in ascending order on this device (op 0:
        ds_wrxchg_rtn_b32, the chain efforts; op 1: ds_mskor_rtn_b32, effort "recent")? -> (mismatches, positions checked)"""
        bad, n = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.sfh_lds_order_check(self._h, int(op), int(blocks), int(iters), C.byref(bad), C.byref(n)))
        return bad.value, n.value

    def set_profiling(self, on=True):
        self._lib.sfh_set_profiling(self._h, int(bool(on)))

    def stage_ms(self):
        ms = (C.c_float * _capi.NSTAGES)()
        self._check(self._lib.sfh_last_stage_ms(self._h, C.byref(ms)))
        return {self._lib.sfh_stage_name(k).decode(): float(ms[k]) for k in range(_capi.NSTAGES)}

    def debug(self, what, nchunks):
        shapes = {
            _capi.DBG_NTOK: ((nchunks,), np.uint32),
            _capi.DBG_TOKENS: ((nchunks, CHUNK_BYTES), np.uint32),
            _capi.DBG_HIST: ((nchunks, 576), np.uint32),  # ll at 0, d at 288, raw len-3 counts at 320
            _capi.DBG_PLAN: ((nchunks, 4), np.uint32),
            _capi.DBG_LENS: ((nchunks, 320), np.uint8),
            _capi.DBG_OFFSETS: ((nchunks,), np.uint64),
            _capi.DBG_STAMPS: ((2, nchunks, 8), np.uint64),  # [0] k_lz77 phases, [1] k_plan phases
            _capi.DBG_SUBINDEX: ((nchunks, 32, 2), np.uint32),
            _capi.DBG_ITEMS: ((nchunks, CHUNK_BYTES), np.uint16),
            _capi.DBG_NITEMS: ((nchunks,), np.uint32),
            _capi.DBG_RITEM: ((nchunks, 32), np.uint32),  # the item index of each region's first token
            _capi.DBG_SEGINFO: ((nchunks, 6), np.uint32),  # decoder: status, tokens, raw | serial << 1, bytes, raw offset (u64)
        }
        shape, dt = shapes[what]
        a = np.empty(shape, dtype=dt)
        self._check(self._lib.sfh_debug_read(self._h, what, a.ctypes.data, a.nbytes))
        return a

    def debug_tokens(self, nchunks):
        """The compressor's 16-bit items of the last call as per-chunk uint32 token arrays in the oracle's format
        (bit 31 match, 16..23 len-3, 0..14 dist-1; literal = byte) -> (list of token arrays, list of (token
        index, region) pairs naming the flagged first tokens of parse regions)."""
        items = self.debug(_capi.DBG_ITEMS, nchunks)
        nit = self.debug(_capi.DBG_NITEMS, nchunks)
        toks, flags = [], []
        for c in range(nchunks):
            if nit[c] & 0x80000000:  # kItemsSkipped: stored fast path, the items behind the first 8 KiB were never written
                raise StarflateError(-1, f"chunk {c} took the stored fast path: its items are not materialised (stored_fast_path=False shows them)")
            it = items[c, : nit[c]].astype(np.uint32)
            start = (it & 0x8000) != 0  # kItemTok: a literal or a match head; clear: the distance behind a head
            head = start & ((it & 0x0100) != 0)  # kItemHead
            assert not np.any(head[:-1] & start[1:]) and (it.size == 0 or not head[-1]), "a head without its distance"
            nxt = np.zeros(it.size, dtype=np.uint32)
            nxt[:-1] = it[1:]
            tok = np.where(head, np.uint32(0x80000000) | ((it & 0xFF) << 16) | (nxt & 0x7FFF), it & 0xFF)[start]
            fl = ((it & 0x4000) != 0)[start]
            reg = ((it >> 9) & 31)[start]  # kItemRegionShift
            toks.append(tok.astype(np.uint32))
            flags.append([(int(k), int(reg[k])) for k in np.flatnonzero(fl)])
        return toks, flags


def compress_multi(compressors, data, strategy="auto", final_stream=True, lazy=True, stored_fast_path=True, container="raw",
                   block_bytes=0):
    """One process, several contexts (normally one per GPU): contiguous shards compressed concurrently, one stream
    out -- bit-identical to a single Compressor.compress call (sfh_compress_multi)."""
    L = _capi.lib()
    src = _as_bytes(data)
    cap = L.sfh_compress_bound(src.size, 0)
    dst = np.empty(cap, dtype=np.uint8)
    out_n = C.c_size_t(0)
    opt = _capi.make_options(strategy, final_stream, lazy, stored_fast_path, container, block_bytes)
    handles = (C.c_void_p * len(compressors))(*[c._h for c in compressors])
    rc = L.sfh_compress_multi(handles, len(compressors), _ptr(src), src.size, dst.ctypes.data, cap, C.byref(out_n), C.byref(opt))
    if rc:
        raise StarflateError(rc, "; ".join(L.sfh_last_error(c._h).decode() for c in compressors))
    return dst[: out_n.value].tobytes()


def checksum_combine(kind, a, b, len_b):
    """Checksum of A||B from checksum(A), checksum(B), len(B); kind "zlib" (Adler-32) or "gzip" (CRC-32)."""
    L = _capi.lib()
    return (L.sfh_adler32_combine if kind == "zlib" else L.sfh_crc32_combine)(a, b, int(len_b))


def wrapper_bytes(kind, checksum, n):
    """(header, trailer) of the zlib / gzip wrapper exactly as the kernels write them (for a multi-GPU job,
    whose rank 0 wraps the concatenated raw shard streams with the combined checksum)."""
    if kind == "zlib":
        return b"\x78\x9c", int(checksum).to_bytes(4, "big")
    if kind == "gzip":
        return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff", int(checksum).to_bytes(4, "little") + (n & 0xFFFFFFFF).to_bytes(4, "little")
    return b"", b""


def _batch_lengths(k, sizes, index_n, subindex_n, block_bytes, container):
    """decompress_batch's lengths, checked before anything reaches the device: k streams, their decoded sizes, the entries of
    the index and words of the sub-index (None: not given) -> (dst_n list, block_bytes array or None, container code)."""
    dst_n = [int(m) for m in sizes]
    if len(dst_n) != k:
        raise ValueError(f"{k} streams but {len(dst_n)} sizes")
    if any(m < 0 for m in dst_n):
        raise ValueError("sizes must not be negative")
    if container not in _capi.CONTAINER:
        raise ValueError(f"container must be one of {sorted(_capi.CONTAINER)}")
    nseg = sum(max(1, -(-m // CHUNK_BYTES)) for m in dst_n)
    if index_n is None:
        if subindex_n is not None:
            raise ValueError("a subindex needs an index")
        if any(m > CHUNK_BYTES for m in dst_n):
            raise ValueError("without an index every size must be at most 32768")
    else:
        if index_n != nseg + k:
            raise ValueError(f"index must hold sum(segments + 1) = {nseg + k} entries, not {index_n}")
        if subindex_n is not None and subindex_n != nseg * _capi.SUBINDEX_WORDS:
            raise ValueError(f"subindex must hold {nseg * _capi.SUBINDEX_WORDS} words, not {subindex_n}")
    bb = None
    if block_bytes is not None:
        bb = np.ascontiguousarray(block_bytes, dtype=np.uint32).ravel()
        if bb.size != k:
            raise ValueError("block_bytes must hold one value per item")
    return dst_n, bb, _capi.CONTAINER[container]


def _range_lengths(total_n, offsets, lengths, index_n, subindex_n, block_bytes):
    """decompress_ranges' lengths, checked before anything reaches the device: the stream's output size, the ranges, the
    entries of the index and the words of the sub-index (None: not given) -> (total_n, offsets list, lengths list, segments)."""
    total_n = int(total_n)
    if total_n < 0 or total_n > (1 << 44):
        raise ValueError("total_n must lie in [0, 2^44]")
    offs, lens = [int(v) for v in offsets], [int(v) for v in lengths]
    if len(offs) != len(lens):
        raise ValueError(f"{len(offs)} offsets but {len(lens)} lengths")
    for o, m in zip(offs, lens):
        if o < 0 or m < 0 or o + m > total_n:
            raise ValueError(f"range [{o}, {o} + {m}) does not lie inside the stream's {total_n} bytes of output")
    nseg = max(1, -(-total_n // CHUNK_BYTES))
    if index_n != nseg + 1:
        raise ValueError(f"index must hold segments + 1 = {nseg + 1} entries, not {index_n}")
    if subindex_n is not None and subindex_n != nseg * _capi.SUBINDEX_WORDS:
        raise ValueError(f"subindex must hold {nseg * _capi.SUBINDEX_WORDS} words, not {subindex_n}")
    bb = int(block_bytes)
    if bb < 0 or bb % CHUNK_BYTES or bb > (1 << 24):
        raise ValueError("block_bytes: a multiple of 32768 up to 16 MiB (0 = 32768)")
    return total_n, offs, lens, nseg


def _range_args(index, total_n, offsets, lengths, subindex, block_bytes):
    idx = np.ascontiguousarray(index, dtype=np.uint64).ravel()
    sub = None if subindex is None else np.ascontiguousarray(subindex, dtype=np.uint32).ravel()
    return _range_lengths(total_n, offsets, lengths, idx.size, None if sub is None else sub.size, block_bytes)


def _batch_inflate_args(streams, sizes, index, subindex, block_bytes, container):
    """decompress_batch's host arguments, checked (_batch_lengths): (sources, src_n, dst_n, index, subindex, block_bytes,
    container) as the C-ABI takes them."""
    srcs = [_as_bytes(d) for d in streams]
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.uint64).ravel()
    sub = None if subindex is None else np.ascontiguousarray(subindex, dtype=np.uint32).ravel()
    dst_n, bb, kind = _batch_lengths(len(srcs), sizes, None if idx is None else idx.size, None if sub is None else sub.size,
                                     block_bytes, container)
    return srcs, _u64s(a.size for a in srcs), dst_n, idx, sub, bb, kind


def _stream_batch_args(streams, sizes, container):
    """decompress_stream_batch's host arguments, checked before anything reaches the device: (sources, src_n, capacities or
    None, container code)."""
    if isinstance(streams, (bytes, bytearray, memoryview, np.ndarray)):
        raise ValueError("streams: a sequence of bytes-like streams")
    srcs = [_as_bytes(d) for d in streams]
    if not isinstance(container, str) or container not in _capi.STREAM_CONTAINER:
        raise ValueError(f"container must be one of {sorted(_capi.STREAM_CONTAINER)}")
    caps = None
    if sizes is not None:
        caps = [int(m) for m in sizes]
        if len(caps) != len(srcs):
            raise ValueError(f"{len(srcs)} streams but {len(caps)} sizes")
        if any(m < 0 or m > (1 << 44) for m in caps):
            raise ValueError("sizes must lie in [0, 2^44]")
    return srcs, _u64s(a.size for a in srcs), caps, _capi.STREAM_CONTAINER[container]


def _any_batch_args(streams, sizes, container):
    """decompress_any_batch's host arguments, checked before anything reaches the device: (sources, src_n, dst_n as the C-ABI
    takes it, capacities, container code).  sizes=None: gzip's ISIZE, which also gives the capacities here."""
    if isinstance(streams, (bytes, bytearray, memoryview, np.ndarray)):
        raise ValueError("streams: a sequence of bytes-like streams")
    srcs = [_as_bytes(d) for d in streams]
    if not isinstance(container, str) or container not in _capi.CONTAINER:
        raise ValueError(f"container must be one of {sorted(_capi.CONTAINER)}")
    kind = _capi.CONTAINER[container]
    k = len(srcs)
    if sizes is None:
        if kind != 2:
            raise ValueError("sizes is required unless container='gzip' (whose trailer carries ISIZE)")
        caps = [int.from_bytes(a[-4:].tobytes(), "little") if a.size >= 18 else 0 for a in srcs]
        want = [_capi.SIZE_FROM_TRAILER] * k
    else:
        caps = [int(m) for m in sizes]
        if len(caps) != k:
            raise ValueError(f"{k} streams but {len(caps)} sizes")
        if any(m < 0 or m > (1 << 44) for m in caps):
            raise ValueError("sizes must lie in [0, 2^44]")
        want = caps
    return srcs, _u64s(a.size for a in srcs), _u64s(want), caps, kind


_DEFAULT = {}


def _default(device):
    """the module-level functions' context of that device, created at its first use"""
    c = _DEFAULT.get(device)
    if c is None:
        c = _DEFAULT[device] = Compressor(device)
    return c


def _raise_on_status(st):
    if st:
        raise StarflateError(st, f"DecompressStatus {st}")


def compress(data, device=0, **kw):
    """bytes-like -> raw DEFLATE bytes, through the GPU (host buffers, PCIe inclusive)."""
    c = _default(device)
    return c.compress(data, **kw)


def compress_batch(items, device=0, **kw):
    """A sequence of bytes-like items -> one stream per item, all in one call (Compressor.compress_batch)."""
    c = _default(device)
    return c.compress_batch(items, **kw)


def _container(container):
    if isinstance(container, str) and container not in _capi.CONTAINER:
        raise ValueError(f"container must be one of {sorted(_capi.CONTAINER)}")
    kind = _capi.CONTAINER[container] if isinstance(container, str) else int(container)
    if kind not in (0, 1, 2):
        raise ValueError("container: raw, zlib or gzip")
    return kind


def _stream_container(container):
    """the decompress_stream* family's: _container's, and gzip_members (SFH_GZIP_MEMBERS)"""
    if isinstance(container, str) and container not in _capi.STREAM_CONTAINER:
        raise ValueError(f"container must be one of {sorted(_capi.STREAM_CONTAINER)}")
    kind = _capi.STREAM_CONTAINER[container] if isinstance(container, str) else int(container)
    if kind not in (0, 1, 2, 4):
        raise ValueError("container: raw, zlib, gzip or gzip_members")
    return kind


def _gzip_room(stream, kind):
    """the capacity a decode behind a size query needs beyond the queried size: container.hpp decodes a gzip body into the
    first ISIZE bytes of a dst that holds at least ISIZE, so a trailer that claims more than the body produces is that
    decode's Error, not a DstTooSmall of the caller's making.  stream: a numpy array or a CUDA tensor that passed its query."""
    if kind != 2:
        return 0
    tail = stream[-4:]
    return int.from_bytes((tail if isinstance(tail, np.ndarray) else tail.cpu().numpy()).tobytes(), "little")


def _isize(tail, kind):
    """out_n=None: gzip's ISIZE (little-endian, the last 4 bytes); other containers carry no size"""
    if kind != 2:
        raise ValueError("out_n is required unless container='gzip' (whose trailer carries ISIZE)")
    return int.from_bytes(tail, "little") if len(tail) == 4 else 0


def decompress(data, out_n=None, container="raw", device=0):
    """One stream given alone -> bytes, on the GPU (Compressor.decompress_any): the segment index is recovered from the
    stream's flush markers.  A status other than Success raises StarflateError; so does a stream that is not block-flushed
    every 32 KiB (code -8): such a stream is the serial decoder's."""
    _container(container)
    c = _default(device)
    out, st = c.decompress_any(data, out_n, container)
    _raise_on_status(st)
    return out


def decompress_stream(data, container="raw", out_n=None, device=0):
    """One raw / zlib / gzip stream with no index and no flush points -> bytes, on the GPU (Compressor.decompress_stream).
    A status other than Success raises StarflateError."""
    c = _default(device)
    out, st = c.decompress_stream(data, out_n, container)
    _raise_on_status(st)
    return out


def decompress_batch(streams, sizes, device=0, **kw):
    """Streams and their decoded sizes -> (list of bytes, list of statuses), all in one call (Compressor.decompress_batch).
    The arguments are checked before a device is touched."""
    _batch_inflate_args(streams, sizes, kw.get("index"), kw.get("subindex"), kw.get("block_bytes"), kw.get("container", "raw"))
    c = _default(device)
    return c.decompress_batch(streams, sizes, **kw)


def decompress_stream_batch(streams, sizes=None, container="raw", device=0):
    """Raw / zlib / gzip streams with no index and no flush points -> (list of bytes, list of statuses), all in one call
    (Compressor.decompress_stream_batch).  The arguments are checked before a device is touched."""
    _stream_batch_args(streams, sizes, container)
    c = _default(device)
    return c.decompress_stream_batch(streams, sizes, container)


def decompress_any_batch(streams, sizes=None, container="raw", device=0, fallback=True):
    """Raw / zlib / gzip streams given alone -> (list of bytes, list of statuses), all in one call on the GPU
    (Compressor.decompress_any_batch): what compress_batch wrote, read back with nothing but the streams.  sizes=None: gzip's
    ISIZE.  fallback=True: the items that are not block-flushed every 32 KiB (status ITEM_NOT_INDEXABLE) are decoded by one
    decompress_stream_batch call, on the GPU as well; fallback=False reports that status.  The arguments are checked before a
    device is touched."""
    _, _, _, caps, _ = _any_batch_args(streams, sizes, container)
    streams = list(streams)
    c = _default(device)
    outs, sts = c.decompress_any_batch(streams, sizes, container)
    rest = [i for i, st in enumerate(sts) if st == ITEM_NOT_INDEXABLE] if fallback else []
    if rest:
        o2, s2 = c.decompress_stream_batch([streams[i] for i in rest], [caps[i] for i in rest], container)
        for i, o, st in zip(rest, o2, s2):
            outs[i], sts[i] = o, st
    return outs, sts


def decompress_range(data, index, total_n, offset, length, subindex=None, *, block_bytes, device=0):
    """Output bytes [offset, offset + length) of an indexed stream -> bytes (Compressor.decompress_range).  The arguments are
    checked before a device is touched; a status other than Success raises StarflateError."""
    _range_args(index, total_n, [offset], [length], subindex, block_bytes)
    c = _default(device)
    out, st = c.decompress_range(data, index, total_n, offset, length, subindex, block_bytes=block_bytes)
    _raise_on_status(st)
    return out


def decompress_ranges(data, index, total_n, offsets, lengths, subindex=None, *, block_bytes, device=0):
    """Many ranges of one indexed stream -> (list of bytes or None, status array), all in one call
    (Compressor.decompress_ranges).  The arguments are checked before a device is touched."""
    _range_args(index, total_n, offsets, lengths, subindex, block_bytes)
    c = _default(device)
    return c.decompress_ranges(data, index, total_n, offsets, lengths, subindex, block_bytes=block_bytes)


def dictzip_index(data):
    """The segment index a dictzip file of 32 KiB chunks carries in its own gzip header -> (uint64 array of segments + 1
    offsets into the file, total_n): what decompress_ranges takes, with block_bytes=32768.  Host arithmetic on the header, no
    device.  A gzip file without such a table raises StarflateError with code -8 (SFH_E_NOT_INDEXABLE), a header that does not
    parse with its DecompressStatus (1 Error, 5 SrcTooSmall)."""
    src = _as_bytes(data)
    index = np.zeros(_capi.DZ_MAX_CHUNKS + 1, dtype=np.uint64)
    info = _capi.DzInfo()
    rc = _capi.lib().sfh_dz_read_index(_ptr(src), src.size, C.byref(info), index.ctypes.data, index.size)
    if rc:
        raise StarflateError(rc, "no dictzip table of 32 KiB chunks in the gzip header")
    if info.status:
        raise StarflateError(info.status, f"dictzip header: DecompressStatus {info.status}")
    return index[: info.nseg + 1].copy(), int(info.total_n)


def decompress_dictzip(data, device=0):
    """A dictzip file -> bytes, on the GPU, decoded with the index its header carries (Compressor.decompress_dictzip).  A file
    whose table the indexed decoder cannot use (dictzip's own default chunk length, or no table at all) is decoded by
    decompress_stream(data, container="gzip") instead, as decompress_any_batch(fallback=True) does for its items.  A status
    other than Success raises StarflateError."""
    c = _default(device)
    try:
        out, st = c.decompress_dictzip(data)
    except StarflateError as e:
        if e.code != _capi.E_NOT_INDEXABLE:
            raise
        return decompress_stream(data, container="gzip", device=device)
    _raise_on_status(st)
    return out


def _bgzf_info_dict(info):
    return {"total_n": int(info.total_n), "members": int(info.members), "max_isize": int(info.max_isize), "has_eof": bool(info.has_eof)}


def bgzf_index(data):
    """The members of a BGZF file (bgzip, BAM, BCF) -> (member_off, out_off, info): uint64 arrays of members + 1 entries --
    every member's first byte and the file's size; the prefix sums of the members' ISIZE -- and a dict with total_n, members,
    max_isize and has_eof.  Host arithmetic, no device.  A file that does not parse raises StarflateError with its
    DecompressStatus (1 Error, 5 SrcTooSmall)."""
    src = _as_bytes(data)
    info = _capi.BgzfInfo()
    L = _capi.lib()
    rc = L.sfh_bgzf_read_index(_ptr(src), src.size, C.byref(info), None, None, 0)  # the count
    if info.status:
        raise StarflateError(info.status, f"BGZF members: DecompressStatus {info.status}")
    moff = np.zeros(info.members + 1, dtype=np.uint64)
    ooff = np.zeros(info.members + 1, dtype=np.uint64)
    rc = L.sfh_bgzf_read_index(_ptr(src), src.size, C.byref(info), moff.ctypes.data, ooff.ctypes.data, moff.size)
    if rc:
        raise StarflateError(rc, "sfh_bgzf_read_index")
    return moff, ooff, _bgzf_info_dict(info)


def _bgzf_info_struct(info):
    """bgzf_index()'s info dict (or a BgzfInfo) -> sfh_bgzf_info; `status` (absent from the dict: 0) passes through"""
    if isinstance(info, _capi.BgzfInfo):
        return info
    return _capi.BgzfInfo(int(info["total_n"]), int(info["members"]), int(info["max_isize"]), int(bool(info["has_eof"])),
                          int(info.get("status", 0)))


def _bgzf_index_args(index):
    member_off, out_off, info = index
    moff = np.ascontiguousarray(member_off, dtype=np.uint64).ravel()
    ooff = np.ascontiguousarray(out_off, dtype=np.uint64).ravel()
    binfo = _bgzf_info_struct(info)
    if moff.size != binfo.members + 1 or ooff.size != binfo.members + 1:
        raise ValueError("member_off / out_off must hold members + 1 entries")
    return moff, ooff, binfo


def _voffset_call(fn, member_off, out_off, values):
    moff = np.ascontiguousarray(member_off, dtype=np.uint64).ravel()
    ooff = np.ascontiguousarray(out_off, dtype=np.uint64).ravel()
    if moff.size == 0 or moff.size != ooff.size:
        raise ValueError("member_off / out_off must hold members + 1 entries")
    src = np.ascontiguousarray(values, dtype=np.uint64).ravel()
    out = np.zeros(src.size, dtype=np.uint64)
    rc = fn(moff.ctypes.data, ooff.ctypes.data, moff.size - 1, src.size, _ptr(src), _ptr(out))
    if rc:
        raise StarflateError(rc, fn.__name__)
    return out


def bgzf_voffsets_to_offsets(member_off, out_off, voffsets):
    """The virtual offsets of a tabix / BAI index (coffset << 16 | uoffset) -> uint64 offsets into the file's output, by
    bgzf_index()'s arrays; 2^64 - 1 where a virtual offset names no member's first byte or a byte behind its output.  Host
    arithmetic, no device."""
    return _voffset_call(_capi.lib().sfh_bgzf_voffsets_to_offsets, member_off, out_off, voffsets)


def bgzf_offsets_to_voffsets(member_off, out_off, offsets):
    """Offsets into a BGZF file's output -> virtual offsets: the member that holds the byte (never an empty one) and the
    byte's place in it; total_n -> the file's end << 16; 2^64 - 1 above total_n.  Host arithmetic, no device."""
    return _voffset_call(_capi.lib().sfh_bgzf_offsets_to_voffsets, member_off, out_off, offsets)


def read_bgzf_ranges(bgzf, offsets, lengths, index=None, device=0):
    """Byte ranges of what a BGZF file holds -> (list of bytes or None, status array) (Compressor.read_bgzf_ranges)."""
    c = _default(device)
    return c.read_bgzf_ranges(bgzf, offsets, lengths, index=index)


def compress_bgzf(data, device=0, **options):
    """bytes-like -> a BGZF file on the GPU (Compressor.compress_bgzf)."""
    c = _default(device)
    return c.compress_bgzf(data, **options)


def decompress_bgzf(data, device=0):
    """A BGZF file -> bytes, on the GPU (Compressor.decompress_bgzf).  A status other than Success raises StarflateError."""
    c = _default(device)
    out, st = c.decompress_bgzf(data)
    _raise_on_status(st)
    return out


# ---- ZIP archives ----
ZIP_ENTRY_UNSUPPORTED = _capi.ZIP_ENTRY_UNSUPPORTED  # a per-entry status: a method other than 0 and 8, or an encrypted entry
ZIP_ENTRY_DTYPE = np.dtype([("local_off", "<u8"), ("data_off", "<u8"), ("csize", "<u8"), ("usize", "<u8"), ("out_off", "<u8"),
                            ("name_off", "<u8"), ("crc32", "<u4"), ("status", "<u4"), ("method", "<u2"), ("flags", "<u2"),
                            ("name_len", "<u2"), ("pad", "<u2")])  # sfh_zip_entry


def _zip_items(items):
    pairs = list(items.items()) if isinstance(items, dict) else list(items)
    names = [b.encode("utf-8") if isinstance(b, str) else bytes(b) for b, _ in pairs]
    return names, [_as_bytes(d) for _, d in pairs]


def _zip_info_dict(info):
    return {k: int(getattr(info, k)) for k, _ in info._fields_}


def zip_bound(sizes, name_lens):
    """sfh_zip_bound: the capacity compress_zip needs for items of these sizes and name lengths (bytes)"""
    k = len(sizes)
    return _capi.lib().sfh_zip_bound(k, _u64s(int(v) for v in sizes), (C.c_uint32 * k)(*[int(v) for v in name_lens]))


def zip_index(data):
    """The entry table of a ZIP archive in host memory, no device: (info dict, entries as a ZIP_ENTRY_DTYPE array)."""
    src = _as_bytes(data)
    L = _capi.lib()
    info = _capi.ZipInfo()
    rc = L.sfh_zip_read_index(_ptr(src), src.size, C.byref(info), None, 0)
    ents = np.zeros(info.entries, ZIP_ENTRY_DTYPE)
    if rc == -2:
        rc = L.sfh_zip_read_index(src.ctypes.data, src.size, C.byref(info), C.c_void_p(ents.ctypes.data), ents.size)
    if rc:
        raise StarflateError(rc, "sfh_zip_read_index")
    return _zip_info_dict(info), ents


def zip_names(data, entries):
    """the entries' names (str: UTF-8 with flag bit 11, else CP437), read where the table says they stand in the file"""
    src = _as_bytes(data)
    return [src[int(e["name_off"]): int(e["name_off"]) + int(e["name_len"])].tobytes().decode("utf-8" if int(e["flags"]) & 0x800 else "cp437")
            for e in entries]


def compress_zip(items, device=0, **options):
    """{name: bytes} or [(name, bytes)] -> a ZIP archive on the GPU (Compressor.compress_zip)."""
    c = _default(device)
    return c.compress_zip(items, **options)


def decompress_zip(data, names=None, device=0):
    """A ZIP archive -> ({name: bytes}, statuses) on the GPU (Compressor.decompress_zip)."""
    c = _default(device)
    return c.decompress_zip(data, names=names)


def _dz_range_args(data, offsets, lengths):
    """read_ranges' arguments, checked on the host: the file's header (dictzip_index) and the ranges against its ISIZE"""
    src = _as_bytes(data)
    _, total_n = dictzip_index(src)
    _, offs, lens, _ = _range_lengths(total_n, offsets, lengths, max(1, -(-total_n // CHUNK_BYTES)) + 1, None, CHUNK_BYTES)
    return src, offs, lens


def read_ranges(data, offsets, lengths, device=0):
    """Byte ranges of what a dictzip file holds, given nothing but its bytes -> (list of bytes or None, status array)
    (Compressor.read_ranges).  The header and the ranges are checked before a device is touched."""
    args = _dz_range_args(data, offsets, lengths)
    c = _default(device)
    return c._read_ranges(*args)
