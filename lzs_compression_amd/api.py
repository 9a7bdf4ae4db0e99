"""Python front-end of liblzs (MI355X build): a ctypes binding of the C-ABI declared in
include/lzs/lzs.h and include/lzs/lzs_batch.h.

The reference is a C library with no Python binding for its C path; this module mirrors
its one-shot interface (c/src/liblzs/lzs.h:218,229: ``lzs_compress`` / ``lzs_decompress``
with (out, out_capacity, in, in_len) -> bytes written) and adds the batch forms.  PyTorch
appears only as plumbing: device buffers and the current HIP stream.

There is no CPU fallback: if liblzs.so is missing, or there is no HIP device, calls raise.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "liblzs.so")

LZS_OK, LZS_E_NO_DEVICE, LZS_E_HIP, LZS_E_ARG, LZS_E_NOMEM = 0, -1, -2, -3, -4
LZS_MAX_HISTORY_SIZE = 2047


class LzsError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"liblzs error {code}: {message}")
        self.code = code


def compressed_max(n: int) -> int:
    """LZS_COMPRESSED_MAX (reference c/src/liblzs/lzs.h:77)."""
    return n + (n + 7) // 8 + 3


def decompressed_max(n: int) -> int:
    """LZS_DECOMPRESSED_MAX (reference c/src/liblzs/lzs.h:81)."""
    return n * 16


_lib = None
_vp, _sz, _u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
_BATCH_DEV = [_vp, _sz, _sz, _vp, _vp, _sz, _vp, _sz, _sz, _vp]
_BATCH_HOST = [_vp, _sz, _sz, _vp, _vp, _sz, _vp, _sz, _sz]
_CHANNELS_DEV = [_vp, _sz, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp]
_BURST_DEV = [_vp, _sz, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _vp]


def lib() -> ctypes.CDLL:
    """The loaded liblzs.so.  Raises ImportError (loudly) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise ImportError(
                f"{_SO} is missing: the HIP library has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C lzs_compression_amd/csrc`).  There is no CPU fallback.")
        # If PyTorch is installed, let it load ITS HIP runtime first: liblzs.so and torch must share
        # one libamdhip64 in the process, and torch only finds its GPUs through the copy it ships
        # (liblzs.so works with either).  Loaded the other way round, torch.cuda reports no devices.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(os.environ.get("LZS_LIBRARY", _SO))     # (LZS_LIBRARY: A/B builds during development)
        for name in ("lzs_compress", "lzs_decompress", "lzs_decompress_concat"):
            f = getattr(L, name)
            f.restype, f.argtypes = _sz, [_vp, _sz, _vp, _sz]
        L.lzs_last_error.restype, L.lzs_last_error.argtypes = ctypes.c_char_p, []
        if hasattr(L, "lzs_release_thread_cache"):      # (an older build named by LZS_LIBRARY, for A/B runs, has none)
            L.lzs_release_thread_cache.restype, L.lzs_release_thread_cache.argtypes = None, []
        L.lzs_backend_info.restype, L.lzs_backend_info.argtypes = ctypes.c_int, [ctypes.c_char_p, _sz]
        for name in ("lzs_compress_batch_device", "lzs_decompress_batch_device"):
            f = getattr(L, name)
            f.restype, f.argtypes = ctypes.c_int, _BATCH_DEV
        for name in ("lzs_compress_batch", "lzs_decompress_batch", "lzs_decompress_batch_device_sync"):
            f = getattr(L, name)
            f.restype, f.argtypes = ctypes.c_int, _BATCH_HOST
        if hasattr(L, "lzs_compress_batch_device_sync"):          # (an older build named by LZS_LIBRARY, for A/B runs, has none)
            L.lzs_compress_batch_device_sync.restype, L.lzs_compress_batch_device_sync.argtypes = ctypes.c_int, _BATCH_HOST
        L.lzs_compress_stream_device.restype = ctypes.c_int
        L.lzs_compress_stream_device.argtypes = [_vp, _sz, ctypes.POINTER(_sz), _vp, _sz]
        L.lzs_decompress_stream_device.restype = ctypes.c_int
        L.lzs_decompress_stream_device.argtypes = [_vp, _sz, ctypes.POINTER(_sz), _vp, _sz]
        L.lzs_compact_device.restype = ctypes.c_int
        L.lzs_compact_device.argtypes = [_vp, _vp, _vp, _sz, _vp, _sz, _vp]
        for name in ("lzs_compress_init_quick", "lzs_compress_init_full", "lzs_decompress_init"):
            f = getattr(L, name)
            f.restype, f.argtypes = None, [_vp]
        L.lzs_compress_incremental.restype, L.lzs_compress_incremental.argtypes = _sz, [_vp, ctypes.c_bool]
        L.lzs_simple_compress.restype, L.lzs_simple_compress.argtypes = _sz, [_vp, _sz, _vp, _sz]
        L.lzs_simple_compress_init.restype, L.lzs_simple_compress_init.argtypes = None, [_vp]
        L.lzs_simple_compress_incremental.restype, L.lzs_simple_compress_incremental.argtypes = _sz, [_vp, ctypes.c_bool]
        L.lzs_decompress_incremental.restype, L.lzs_decompress_incremental.argtypes = _sz, [_vp]
        for name in ("lzs_compress_channels_device", "lzs_decompress_channels_device"):
            if hasattr(L, name):        # (an older build named by LZS_LIBRARY, for A/B runs, has none)
                f = getattr(L, name)
                f.restype, f.argtypes = ctypes.c_int, _CHANNELS_DEV
        for name in ("lzs_compress_channels_burst_device", "lzs_decompress_channels_burst_device"):
            if hasattr(L, name):
                f = getattr(L, name)
                f.restype, f.argtypes = ctypes.c_int, _BURST_DEV
        if hasattr(L, "lzs_channels_burst_work_bytes"):
            L.lzs_channels_burst_work_bytes.restype, L.lzs_channels_burst_work_bytes.argtypes = _sz, [_sz, _sz]
        if hasattr(L, "lzs_channels_burst_split_work_bytes"):
            L.lzs_channels_burst_split_work_bytes.restype = _sz
            L.lzs_channels_burst_split_work_bytes.argtypes = [_sz, _sz, _sz]
        if hasattr(L, "lzs_decompressed_size_batch_device"):      # (an older build named by LZS_LIBRARY, for A/B runs, has none)
            L.lzs_decompressed_size_batch_device.restype = ctypes.c_int
            L.lzs_decompressed_size_batch_device.argtypes = [_vp, _vp, _vp, _sz, _vp, _sz, _sz, _sz, _vp]
        if hasattr(L, "lzs_decompressed_size_stream_device"):     # (the same: the size query for long streams)
            _u64p, _u64 = ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64
            for name in ("lzs_decompressed_size_stream_device", "lzs_decompressed_size_stream"):
                f = getattr(L, name)
                f.restype, f.argtypes = ctypes.c_int, [_u64p, _vp, _vp, _sz, _u64, ctypes.c_uint]
            L.lzs_decompressed_size_batch_device_sync.restype = ctypes.c_int
            L.lzs_decompressed_size_batch_device_sync.argtypes = [_vp, _vp, _vp, _sz, _vp, _sz, _sz, _sz]
        if hasattr(L, "lzs_decompress_batch_packed_device"):      # (the same: the packed calls)
            L.lzs_offsets_from_sizes_device.restype = ctypes.c_int
            L.lzs_offsets_from_sizes_device.argtypes = [_vp, _vp, _sz, _sz, _vp]
            L.lzs_decompressed_size_packed_device.restype = ctypes.c_int
            L.lzs_decompressed_size_packed_device.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _sz, _vp]
            L.lzs_decompress_batch_packed_device.restype = ctypes.c_int
            L.lzs_decompress_batch_packed_device.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
            L.lzs_decompress_channels_packed_device.restype = ctypes.c_int
            L.lzs_decompress_channels_packed_device.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
        if hasattr(L, "lzs_compress_batch_packed_device"):        # (the same: packed compression)
            L.lzs_compressed_bound_packed_device.restype = ctypes.c_int
            L.lzs_compressed_bound_packed_device.argtypes = [_vp, _vp, _vp, _sz, _vp]
            L.lzs_compress_batch_packed_device.restype = ctypes.c_int
            L.lzs_compress_batch_packed_device.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
            L.lzs_compress_channels_packed_device.restype = ctypes.c_int
            L.lzs_compress_channels_packed_device.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
            L.lzs_compact_packed_device.restype = ctypes.c_int
            L.lzs_compact_packed_device.argtypes = [_vp, _vp, _vp, _vp, _vp, _sz, _vp]
        if hasattr(L, "lzs_compress_channels_burst_packed_device"):      # (the same: packed bursts)
            L.lzs_channels_burst_packed_split_work_bytes.restype = _sz
            L.lzs_channels_burst_packed_split_work_bytes.argtypes = [_sz, _sz, ctypes.c_uint64]
            for name in ("lzs_compress_channels_burst_packed_device", "lzs_decompress_channels_burst_packed_device"):
                f = getattr(L, name)
                f.restype, f.argtypes = ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _vp]
        if hasattr(L, "lzs_compress_channels_burst_flags_device"):       # (the same: history resets inside a burst)
            for name in ("lzs_compress_channels_burst_flags_device", "lzs_decompress_channels_burst_flags_device"):
                f = getattr(L, name)
                f.restype, f.argtypes = ctypes.c_int, _BURST_DEV[:9] + [_vp] + _BURST_DEV[9:]
            for name in ("lzs_compress_channels_burst_packed_flags_device", "lzs_decompress_channels_burst_packed_flags_device"):
                f = getattr(L, name)
                f.restype, f.argtypes = ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _vp]
        _lib = L
    return _lib


def last_error() -> str:
    return lib().lzs_last_error().decode("utf-8", "replace")


def _check(rc: int) -> None:
    if rc != LZS_OK:
        raise LzsError(rc, last_error())


def release_thread_cache() -> None:
    """lzs_release_thread_cache(): what the CALLING THREAD's earlier host-buffer and one-shot calls left behind (device
    staging, streams, pinned pieces) is given back now instead of when the thread exits (include/lzs/lzs_batch.h)."""
    lib().lzs_release_thread_cache()


def backend_info() -> str:
    buf = ctypes.create_string_buffer(512)
    rc = lib().lzs_backend_info(buf, len(buf))
    if rc != LZS_OK:
        raise LzsError(rc, buf.value.decode("utf-8", "replace"))
    return buf.value.decode()


# ------------------------------------------------------------------ one-shot (host bytes)
def _one_shot(fn, data: bytes, cap: int) -> bytes:
    data = bytes(data)
    src = ctypes.create_string_buffer(data, max(len(data), 1))      # exactly len bytes: no spare byte
    dst = ctypes.create_string_buffer(max(cap, 1))
    n = fn(ctypes.addressof(dst), cap, ctypes.addressof(src), len(data))
    if n == 0:
        # the one-shot calls clear the thread's error text on entry, so a message here
        # means THIS call failed (no device, HIP error) rather than "0 bytes produced"
        msg = last_error()
        if msg:
            raise LzsError(LZS_E_HIP, msg)
    if n > cap:
        raise LzsError(LZS_E_ARG, f"library reported {n} bytes for a {cap}-byte buffer")
    return dst.raw[:n]


def compress(data: bytes, out_capacity: Optional[int] = None) -> bytes:
    """lzs_compress(): ``data`` as ONE LZS stream (reference lzs-compression.c:249-467).
    ``out_capacity`` plays a_outBufferSize: a smaller value cuts the stream there."""
    cap = compressed_max(len(data)) if out_capacity is None else out_capacity
    return _one_shot(lib().lzs_compress, data, cap)


def decompress(data: bytes, out_capacity: Optional[int] = None) -> bytes:
    """lzs_decompress() (reference lzs-decompression.c:156-412).  ``out_capacity`` None: the size is asked first
    (decompressed_size) and the output allocated exactly."""
    if out_capacity is None:
        out_capacity = decompressed_size(data)[0]
    return _one_shot(lib().lzs_decompress, data, out_capacity)


def decompress_concat(data: bytes, out_capacity: Optional[int] = None) -> bytes:
    """A file of streams back to back, decoded as the reference's file tool does
    (decoder carries on after each end marker: reference lzs-decompression.c:564-576).  ``out_capacity`` None: the size is
    asked first (decompressed_size with concat=True) and the output allocated exactly."""
    if out_capacity is None:
        out_capacity = decompressed_size(data, concat=True)[0]
    return _one_shot(lib().lzs_decompress_concat, data, out_capacity)


# --------------------------------------------------------------- host batches (numpy)
def _host_batch(fn, blocks: np.ndarray, in_len: Optional[np.ndarray], out_cap: int):
    assert blocks.dtype == np.uint8 and blocks.ndim == 2 and blocks.flags.c_contiguous
    nb, stride = blocks.shape
    out = np.zeros((nb, max(out_cap, 1)), dtype=np.uint8)
    out_len = np.zeros(nb, dtype=np.uint32)
    if in_len is not None:
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
        assert in_len.shape == (nb,) and (in_len <= stride).all()
    _check(fn(out.ctypes.data, out.shape[1], out_cap, out_len.ctypes.data, blocks.ctypes.data,
              stride, None if in_len is None else in_len.ctypes.data, stride, nb))
    return out, out_len


def compress_batch(blocks: np.ndarray, in_len: Optional[np.ndarray] = None,
                   out_capacity: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Rows of ``blocks`` (host uint8 [nblocks, stride]) as independent streams."""
    cap = compressed_max(blocks.shape[1]) if out_capacity is None else out_capacity
    return _host_batch(lib().lzs_compress_batch, blocks, in_len, cap)


def decompress_batch(blocks: np.ndarray, in_len: Optional[np.ndarray], out_capacity: int):
    return _host_batch(lib().lzs_decompress_batch, blocks, in_len, out_capacity)


# -------------------------------------------------------- device batches (torch tensors)
def _stream_handle(stream) -> Optional[int]:
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    return ctypes.c_void_p(s.cuda_stream)


def _device_batch(fn, x, in_len, out_cap, out, out_len, stream):
    import torch
    assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.stride(1) == 1, \
        "blocks must be a CUDA uint8 tensor [nblocks, stride] with contiguous rows"
    nb = x.shape[0]
    if out is None:
        # 16-byte-aligned slot stride so every slot takes the aligned store path
        stride = (max(out_cap, 1) + 15) // 16 * 16
        out = torch.empty((nb, stride), dtype=torch.uint8, device=x.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape[0] == nb and out.stride(1) == 1
    assert out.shape[1] >= out_cap
    if out_len is None:
        out_len = torch.empty(nb, dtype=torch.int32, device=x.device)
    assert out_len.is_cuda and out_len.dtype == torch.int32 and out_len.numel() == nb
    if in_len is not None:
        assert in_len.is_cuda and in_len.dtype == torch.int32 and in_len.numel() == nb
    _check(fn(out.data_ptr(), out.stride(0) if nb > 1 else out.shape[1], out_cap, out_len.data_ptr(),
              x.data_ptr(), x.stride(0) if nb > 1 else x.shape[1],
              None if in_len is None else in_len.data_ptr(), x.shape[1], nb,
              _stream_handle(stream)))
    return out, out_len


def compress_blocks(x, in_len=None, out_capacity: Optional[int] = None, out=None, out_len=None,
                    stream=None):
    """Device batch: each row of ``x`` (CUDA uint8 [nblocks, stride]) is one independent
    lzs_compress() call; asynchronous on ``stream`` (default: torch's current stream).
    Returns (slots [nblocks, slot_stride] uint8, lengths [nblocks] int32)."""
    cap = compressed_max(x.shape[1]) if out_capacity is None else out_capacity
    return _device_batch(lib().lzs_compress_batch_device, x, in_len, cap, out, out_len, stream)


def decompress_blocks(x, in_len, out_capacity: int, out=None, out_len=None, stream=None):
    """Device batch of independent lzs_decompress() calls; arguments as compress_blocks."""
    return _device_batch(lib().lzs_decompress_batch_device, x, in_len, out_capacity, out, out_len, stream)


def decompress_blocks_sync(x, in_len, out_capacity: int, out=None):
    """lzs_decompress_batch_device_sync(): a SMALL batch of streams in device memory (``x``: uint8
    [nblocks, stride]) with their lengths on the host (``in_len``: sequence / numpy array, or None
    for full rows), every block cut into segments for many wavefronts.  Synchronous.  Returns
    (out [nblocks, out_capacity] on the device, lengths as a numpy array)."""
    import torch
    assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.stride(1) == 1
    nblocks = x.shape[0]
    if out is None:
        out = torch.empty((nblocks, out_capacity), dtype=torch.uint8, device=x.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape[0] == nblocks and out.stride(1) == 1
    lens = None if in_len is None else np.ascontiguousarray(in_len, dtype=np.uint32)
    out_len = np.zeros(nblocks, dtype=np.uint32)
    torch.cuda.current_stream().synchronize()             # the call runs on the library's own stream
    _check(lib().lzs_decompress_batch_device_sync(
        out.data_ptr(), out.stride(0), out_capacity, out_len.ctypes.data,
        x.data_ptr(), x.stride(0), None if lens is None else lens.ctypes.data, x.shape[1], nblocks))
    return out, out_len


def compress_blocks_sync(x, in_len=None, out_capacity: Optional[int] = None, out=None):
    """lzs_compress_batch_device_sync(): a batch of FEW LONG blocks in device memory (``x``: uint8 [nblocks, stride]) with their
    lengths on the host (``in_len``: sequence / numpy array, or None for full rows), every block cut into segments for the whole
    device where that is faster.  Same streams as compress_blocks().  Synchronous.  Returns
    (out [nblocks, slot_stride] on the device -- the capacity rounded up to 4 --, lengths as a numpy array)."""
    import torch
    assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.stride(1) == 1
    nblocks = x.shape[0]
    cap = compressed_max(x.shape[1]) if out_capacity is None else out_capacity
    if out is None:
        out = torch.empty((nblocks, (max(cap, 1) + 3) // 4 * 4), dtype=torch.uint8, device=x.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape[0] == nblocks and out.stride(1) == 1
    lens = None if in_len is None else np.ascontiguousarray(in_len, dtype=np.uint32)
    assert lens is None or (lens.shape == (nblocks,) and (lens <= x.shape[1]).all())
    out_len = np.zeros(nblocks, dtype=np.uint32)
    torch.cuda.current_stream().synchronize()             # the call runs on the library's own stream
    _check(lib().lzs_compress_batch_device_sync(
        out.data_ptr(), out.stride(0) if nblocks > 1 else out.shape[1], cap, out_len.ctypes.data,
        x.data_ptr(), x.stride(0) if nblocks > 1 else x.shape[1], None if lens is None else lens.ctypes.data, x.shape[1], nblocks))
    return out, out_len


def compress_stream(x, out=None):
    """lzs_compress_stream_device(): the device tensor ``x`` (uint8, contiguous) as ONE LZS stream,
    compressed by the whole device (segments of 4-64 KiB).  Returns
    (buffer uint8 [compressed_max(n) + 1024], nbytes); the stream is buffer[:nbytes].  Synchronous."""
    import torch
    n = x.numel()
    need = compressed_max(n) + 1024
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=x.device)
    got = _sz(0)
    torch.cuda.current_stream().synchronize()             # the call runs on the library's own stream
    _check(lib().lzs_compress_stream_device(out.data_ptr(), out.numel(), ctypes.byref(got), x.data_ptr(), n))
    return out, int(got.value)


def decompress_stream(x, out_capacity=None, out=None):
    """lzs_decompress_stream_device(): the device tensor ``x`` (one LZS stream, uint8) decompressed
    by many wavefronts.  Returns (buffer uint8 [out_capacity], nbytes).  Synchronous.  ``out_capacity`` None:
    the size is asked first (decompressed_size_stream) and the buffer is exactly that long -- or ``out``, if given, is its room."""
    import torch
    if out_capacity is None:
        out_capacity = out.numel() if out is not None else decompressed_size_stream(x)[0]
    if out is None:
        out = torch.empty(out_capacity, dtype=torch.uint8, device=x.device)
    got = _sz(0)
    torch.cuda.current_stream().synchronize()             # the call runs on the library's own stream
    _check(lib().lzs_decompress_stream_device(out.data_ptr(), out_capacity, ctypes.byref(got), x.data_ptr(), x.numel()))
    return out, int(got.value)


def compact(slots, lengths, stream=None, dense=None, offsets=None):
    """Dense concatenation of the first lengths[b] bytes of every slot.
    Returns (dense uint8 [>= sum], offsets int64 [nblocks+1]); asynchronous.  ``dense`` /
    ``offsets`` may be passed in for reuse (dense: at least nblocks * slot bytes)."""
    import torch
    nb = slots.shape[0]
    if offsets is None:
        offsets = torch.empty(nb + 1, dtype=torch.int64, device=slots.device)
    if dense is None:
        dense = torch.empty(nb * slots.shape[1], dtype=torch.uint8, device=slots.device)
    assert offsets.dtype == torch.int64 and offsets.numel() == nb + 1 and offsets.is_cuda
    assert dense.dtype == torch.uint8 and dense.numel() >= nb * slots.shape[1] and dense.is_contiguous()
    _check(lib().lzs_compact_device(dense.data_ptr(), offsets.data_ptr(), slots.data_ptr(),
                                    slots.stride(0) if nb > 1 else slots.shape[1],
                                    lengths.data_ptr(), nb, _stream_handle(stream)))
    return dense, offsets


# -------------------------------------------------- sizes before decoding (lzs_batch.h)
SIZE_LIMIT_NONE = 0xFFFFFFFF        # limit of the size query that asks for the true size


def decompressed_sizes(x, in_len=None, limit: Optional[int] = None, size=None, status=None, stream=None):
    """lzs_decompressed_size_batch_device(): what decoding each row of ``x`` (CUDA uint8 [nblocks, stride], ``in_len[b]`` bytes or
    whole rows) at an output capacity of ``limit`` would give, without decoding -- a token walk, no output traffic.  ``limit``
    None: 0xFFFFFFFF, the true size.  Returns (size int32 [nblocks] -- the bits of a uint32: a size of 2 GiB and more reads
    negative --, status uint8 [nblocks]: the STATUS_* bits decompress_channels gives at ``out_capacity=limit``, STATUS_END_MARKER
    for a whole stream); both may be passed in for reuse.  The same for channel and burst packets, whatever their channel's
    history.  Asynchronous on ``stream``."""
    import torch
    assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.stride(1) == 1, \
        "blocks must be a CUDA uint8 tensor [nblocks, stride] with contiguous rows"
    nb = x.shape[0]
    limit = SIZE_LIMIT_NONE if limit is None else int(limit)
    if size is None:
        size = torch.empty(nb, dtype=torch.int32, device=x.device)
    assert size.is_cuda and size.dtype == torch.int32 and size.numel() == nb and size.is_contiguous()
    if status is None:
        status = torch.empty(nb, dtype=torch.uint8, device=x.device)
    assert status.is_cuda and status.dtype == torch.uint8 and status.numel() == nb and status.is_contiguous()
    if in_len is not None:
        assert in_len.is_cuda and in_len.dtype == torch.int32 and in_len.numel() == nb
    _check(lib().lzs_decompressed_size_batch_device(
        size.data_ptr(), status.data_ptr(), x.data_ptr(), x.stride(0) if nb > 1 else x.shape[1],
        None if in_len is None else in_len.data_ptr(), x.shape[1], limit, nb, _stream_handle(stream)))
    return size, status


SIZE_CONCAT = 1                     # LZS_SIZE_CONCAT: the file rule of decompress_concat
_SIZE_MAX64 = (1 << 64) - 1


def _size_stream(fn, ptr, n: int, limit: Optional[int], concat: bool) -> Tuple[int, int]:
    size, status = ctypes.c_uint64(0), ctypes.c_uint8(0)
    _check(fn(ctypes.byref(size), ctypes.addressof(status), ptr, n, _SIZE_MAX64 if limit is None else int(limit),
              SIZE_CONCAT if concat else 0))
    return int(size.value), int(status.value)


def decompressed_size(data: bytes, limit: Optional[int] = None, concat: bool = False) -> Tuple[int, int]:
    """lzs_decompressed_size_stream(): (size, status) of ONE stream in host memory at an output capacity of ``limit`` (None: no
    limit, the true size), without decoding it: len(decompress(data, limit)) and the STATUS_* bits the size query of a batch
    gives -- with ``concat`` len(decompress_concat(data, limit)), and STATUS_NO_OUTPUT_BUFFER_SPACE if that is the limit,
    otherwise STATUS_INPUT_STARVED | STATUS_INPUT_FINISHED.  A segmented walk over the whole device."""
    data = bytes(data)
    src = ctypes.create_string_buffer(data, max(len(data), 1))      # exactly len bytes: no spare byte
    return _size_stream(lib().lzs_decompressed_size_stream, ctypes.addressof(src), len(data), limit, concat)


def decompressed_size_stream(x, limit: Optional[int] = None, concat: bool = False) -> Tuple[int, int]:
    """lzs_decompressed_size_stream_device(): the same for the device tensor ``x`` (one LZS stream, uint8, contiguous; any
    alignment).  Synchronous."""
    import torch
    assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous()
    torch.cuda.current_stream().synchronize()             # the call runs on the library's own stream
    return _size_stream(lib().lzs_decompressed_size_stream_device, x.data_ptr(), x.numel(), limit, concat)


def decompressed_sizes_sync(x, in_len=None, limit: Optional[int] = None):
    """lzs_decompressed_size_batch_device_sync(): decompressed_sizes() for a batch of LONG blocks in device memory (``x``: uint8
    [nblocks, stride]) with their lengths on the host (``in_len``: sequence / numpy array, or None for full rows) -- cut into
    segments for the whole device where the blocks are long enough, one lane a block otherwise.  Synchronous.  Returns
    (size uint32 [nblocks], status uint8 [nblocks]) as numpy arrays."""
    import torch
    assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.stride(1) == 1
    nblocks = x.shape[0]
    lens = None if in_len is None else np.ascontiguousarray(in_len, dtype=np.uint32)
    assert lens is None or (lens.shape == (nblocks,) and (lens <= x.shape[1]).all())
    size = np.zeros(nblocks, dtype=np.uint32)
    status = np.zeros(nblocks, dtype=np.uint8)
    torch.cuda.current_stream().synchronize()             # the call runs on the library's own stream
    _check(lib().lzs_decompressed_size_batch_device_sync(
        size.ctypes.data, status.ctypes.data, x.data_ptr(), x.stride(0) if nblocks > 1 else x.shape[1],
        None if lens is None else lens.ctypes.data, x.shape[1], SIZE_LIMIT_NONE if limit is None else int(limit), nblocks))
    return size, status


def decompress_blocks_dense(x, in_len=None, stream=None):
    """The rows of ``x`` (whole LZS streams, as for decompress_blocks) decoded into ONE dense byte string by a caller who does
    not know their sizes: decompressed_sizes(), one host read of the largest size, decompress_blocks() at that capacity, then
    compact().  Returns (dense uint8, offsets int64 [nblocks + 1]): block b is dense[offsets[b]:offsets[b + 1]].  Raises
    ValueError naming the first block that does not end in an end marker (a truncated stream).  Peak device memory is
    nblocks * max(size) bytes of slots beside the dense result of the same capacity; one host read, which waits for the
    sizes.  decompress_dense() does the same from packed streams without the slots."""
    import torch
    nb = x.shape[0]
    size, status = decompressed_sizes(x, in_len, None, stream=stream)
    if nb == 0:
        return torch.empty(0, dtype=torch.uint8, device=x.device), torch.zeros(1, dtype=torch.int64, device=x.device)
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        bad = status != STATUS_END_MARKER
        first = bad.to(torch.uint8).argmax()
        top = torch.stack([(size.to(torch.int64) & 0xFFFFFFFF).max(), bad.any().to(torch.int64), first.to(torch.int64),
                           status[first].to(torch.int64)]).cpu()                         # the one host read
    cap, any_bad, first_bad, its_status = (int(v) for v in top)
    if any_bad:
        raise ValueError(f"decompress_blocks_dense: block {first_bad} does not end in an end marker (status 0x{its_status:02x})")
    slots, lens = decompress_blocks(x, in_len, cap, stream=stream)
    return compact(slots, lens, stream=stream)


# ------------------------------- packed streams, packed outputs (lzs_batch.h, lzs_channels.h)
def _packed_input(data, in_off, in_len, nb=None):
    """The checks of a packed input; returns the number of blocks (``nb`` if given)."""
    import torch
    assert data.is_cuda and data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous(), \
        "packed streams are one contiguous CUDA uint8 tensor"
    assert in_off.is_cuda and in_off.dtype == torch.int64 and in_off.dim() == 1 and in_off.is_contiguous(), \
        "offsets are a contiguous CUDA int64 tensor"
    if in_len is not None:
        assert in_len.is_cuda and in_len.dtype == torch.int32 and in_len.dim() == 1 and in_len.is_contiguous()
        n = in_len.numel() if nb is None else nb
        assert in_len.numel() == n and in_off.numel() >= n
    else:
        n = max(in_off.numel() - 1, 0) if nb is None else nb
        assert in_off.numel() >= n + 1, "without in_len the offsets have nblocks + 1 entries"
    return n


def offsets_from_sizes(size, align: int = 1, offsets=None, stream=None):
    """lzs_offsets_from_sizes_device(): offsets[0] = 0, offsets[b + 1] = offsets[b] + size[b] rounded up to ``align`` (a power of
    two from 1 to 256) -- int64 [nblocks + 1], the total in offsets[-1].  ``size``: CUDA int32 [nblocks], read as uint32 (what
    decompressed_sizes_packed returns).  Asynchronous on ``stream``."""
    import torch
    assert size.is_cuda and size.dtype == torch.int32 and size.dim() == 1 and size.is_contiguous()
    nb = size.numel()
    if offsets is None:
        offsets = torch.empty(nb + 1, dtype=torch.int64, device=size.device)
    assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.numel() == nb + 1 and offsets.is_contiguous()
    _check(lib().lzs_offsets_from_sizes_device(offsets.data_ptr(), size.data_ptr(), int(align), nb, _stream_handle(stream)))
    return offsets


def decompressed_sizes_packed(data, in_off, in_len=None, limit: Optional[int] = None, size=None, status=None, stream=None):
    """lzs_decompressed_size_packed_device(): decompressed_sizes() for packed streams -- block b is the ``in_len[b]`` bytes of
    ``data`` (CUDA uint8, one dimension) at ``in_off[b]`` (int64), or data[in_off[b]:in_off[b + 1]] without ``in_len``.  Returns
    (size int32 [nblocks], status uint8 [nblocks]); an entry that is not a block (decreasing offsets, a length above 3 GiB) has
    size 0 and STATUS_ERROR.  Asynchronous on ``stream``."""
    import torch
    nb = _packed_input(data, in_off, in_len)
    limit = SIZE_LIMIT_NONE if limit is None else int(limit)
    if size is None:
        size = torch.empty(nb, dtype=torch.int32, device=data.device)
    assert size.is_cuda and size.dtype == torch.int32 and size.numel() == nb and size.is_contiguous()
    if status is None:
        status = torch.empty(nb, dtype=torch.uint8, device=data.device)
    assert status.is_cuda and status.dtype == torch.uint8 and status.numel() == nb and status.is_contiguous()
    _check(lib().lzs_decompressed_size_packed_device(
        size.data_ptr(), status.data_ptr(), _ptr(data, in_off), in_off.data_ptr(), None if in_len is None else in_len.data_ptr(),
        limit, nb, _stream_handle(stream)))
    return size, status


def _ptr(t, other):
    """An empty tensor has no address, and the C calls want one: every block in it is empty and every room in it 0, so nothing is
    read or written through the stand-in."""
    return t.data_ptr() or other.data_ptr()


def _packed_output(out, out_off):
    import torch
    assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous()
    assert out_off.is_cuda and out_off.dtype == torch.int64 and out_off.dim() == 1 and out_off.is_contiguous() and out_off.numel() >= 1
    return out_off.numel() - 1


def decompress_packed(data, in_off, out, out_off, in_len=None, out_len=None, stream=None):
    """lzs_decompress_batch_packed_device(): block b (as for decompressed_sizes_packed) decoded to out[out_off[b]:out_off[b + 1]]
    -- that slice is its room, its out_capacity.  ``out``: CUDA uint8, one dimension; ``out_off``: int64 [nblocks + 1].  Nothing of
    ``out`` outside out[out_off[b] : out_off[b] + out_len[b]] is written.  Returns (out, out_len int32 [nblocks]).  Asynchronous."""
    import torch
    nb = _packed_output(out, out_off)
    _packed_input(data, in_off, in_len, nb)
    if out_len is None:
        out_len = torch.empty(nb, dtype=torch.int32, device=data.device)
    assert out_len.is_cuda and out_len.dtype == torch.int32 and out_len.numel() == nb and out_len.is_contiguous()
    _check(lib().lzs_decompress_batch_packed_device(
        _ptr(out, out_off), out_off.data_ptr(), out_len.data_ptr(), _ptr(data, in_off), in_off.data_ptr(),
        None if in_len is None else in_len.data_ptr(), nb, _stream_handle(stream)))
    return out, out_len


def decompress_channels_packed(data, in_off, channels, states, out, out_off, in_len=None, out_len=None, status=None, stream=None):
    """lzs_decompress_channels_packed_device(): decompress_channels() from packed packets to packed outputs, one packet per
    channel per call (``channels``: int32 [npackets] or None for packet b on channel b; ``states`` from new_channel_states).
    Returns (out, out_len int32, status uint8).  Asynchronous."""
    import torch
    nb = _packed_output(out, out_off)
    _packed_input(data, in_off, in_len, nb)
    if out_len is None:
        out_len = torch.empty(nb, dtype=torch.int32, device=data.device)
    assert out_len.is_cuda and out_len.dtype == torch.int32 and out_len.numel() == nb and out_len.is_contiguous()
    if status is None:
        status = torch.empty(nb, dtype=torch.uint8, device=data.device)
    assert status.is_cuda and status.dtype == torch.uint8 and status.numel() == nb and status.is_contiguous()
    if channels is not None:
        assert channels.is_cuda and channels.dtype == torch.int32 and channels.numel() == nb and channels.is_contiguous()
    assert states.is_cuda and states.dtype == torch.uint8 and states.is_contiguous()
    _check(lib().lzs_decompress_channels_packed_device(
        _ptr(out, out_off), out_off.data_ptr(), out_len.data_ptr(), _ptr(data, in_off), in_off.data_ptr(),
        None if in_len is None else in_len.data_ptr(), None if channels is None else channels.data_ptr(), states.data_ptr(),
        status.data_ptr(), nb, _stream_handle(stream)))
    return out, out_len, status


def decompress_dense(data, in_off, in_len=None, align: int = 1, stream=None):
    """Packed streams (whole LZS streams, as for decompressed_sizes_packed) decoded into ONE dense byte string by a caller who
    does not know their sizes: decompressed_sizes_packed(), offsets_from_sizes(), one host read -- the total, and the first
    block that does not end in its end marker --, one allocation of exactly the total, decompress_packed().  Returns (dense
    uint8 [total], offsets int64 [nblocks + 1]); block b is dense[offsets[b] : offsets[b] + size[b]], and with ``align`` 1 that is
    dense[offsets[b]:offsets[b + 1]].  Raises ValueError naming the first block that does not end in an end marker.

    Peak device memory: the result (offsets[-1] bytes) and two small arrays, the sizes (int32 [nblocks], also the decoder's
    lengths) and the offsets (int64 [nblocks + 1]); what the check of the statuses needs is smaller than those two and is
    released before the result is allocated.  No slots: decompress_blocks_dense() needs nblocks * max(size) bytes of them
    beside its result.  One host read, which waits for the sizes."""
    import torch
    nb = _packed_input(data, in_off, in_len)
    if nb == 0:
        return torch.empty(0, dtype=torch.uint8, device=data.device), torch.zeros(1, dtype=torch.int64, device=data.device)
    size, status = decompressed_sizes_packed(data, in_off, in_len, None, stream=stream)
    offsets = offsets_from_sizes(size, align, stream=stream)
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        bad = status != STATUS_END_MARKER
        first = bad.to(torch.uint8).argmax()
        top = torch.stack([offsets[nb], bad.any().to(torch.int64), first.to(torch.int64), status[first].to(torch.int64)]).cpu()   # the one host read
        del bad, first
    total, any_bad, first_bad, its_status = (int(v) for v in top)
    del status, top
    if any_bad:
        raise ValueError(f"decompress_dense: block {first_bad} does not end in an end marker (status 0x{its_status:02x})")
    dense = torch.empty(total, dtype=torch.uint8, device=data.device)
    decompress_packed(data, in_off, dense, offsets, in_len=in_len, out_len=size, stream=stream)
    return dense, offsets


# ------------------------------- packed compression (lzs_batch.h "PACKED COMPRESSION", lzs_channels.h)
def compressed_bounds_packed(in_off, in_len=None, bound=None, stream=None):
    """lzs_compressed_bound_packed_device(): bound[b] = LZS_COMPRESSED_MAX(length of packed block b) -- int32 [nblocks], the bits of
    a uint32 --, 0 for an entry that is not a block.  ``in_off``: int64 [nblocks + 1], or [nblocks] with ``in_len`` (int32), which
    then says the lengths.  offsets_from_sizes(bound, align) makes the rooms of it.  Asynchronous on ``stream``."""
    import torch
    assert in_off.is_cuda and in_off.dtype == torch.int64 and in_off.dim() == 1 and in_off.is_contiguous(), \
        "offsets are a contiguous CUDA int64 tensor"
    if in_len is not None:
        assert in_len.is_cuda and in_len.dtype == torch.int32 and in_len.dim() == 1 and in_len.is_contiguous()
        nb = in_len.numel()
        assert in_off.numel() >= nb
    else:
        assert in_off.numel() >= 1, "without in_len the offsets have nblocks + 1 entries"
        nb = in_off.numel() - 1
    if bound is None:
        bound = torch.empty(nb, dtype=torch.int32, device=in_off.device)
    assert bound.is_cuda and bound.dtype == torch.int32 and bound.numel() == nb and bound.is_contiguous()
    _check(lib().lzs_compressed_bound_packed_device(bound.data_ptr(), in_off.data_ptr(), None if in_len is None else in_len.data_ptr(),
                                                    nb, _stream_handle(stream)))
    return bound


def compress_packed(data, in_off, out, out_off, in_len=None, out_len=None, stream=None):
    """lzs_compress_batch_packed_device(): block b (data[in_off[b]:in_off[b + 1]], or ``in_len[b]`` bytes at in_off[b]) compressed
    to out[out_off[b]:out_off[b + 1]] -- that slice is its room, its out_capacity, and nothing outside it is written for the block.
    ``data``, ``out``: CUDA uint8, one dimension, not overlapping; ``out_off``: int64 [nblocks + 1].  Returns (out, out_len int32
    [nblocks]); an entry that is not a block has length 0.  Asynchronous."""
    import torch
    nb = _packed_output(out, out_off)
    _packed_input(data, in_off, in_len, nb)
    if out_len is None:
        out_len = torch.empty(nb, dtype=torch.int32, device=data.device)
    assert out_len.is_cuda and out_len.dtype == torch.int32 and out_len.numel() == nb and out_len.is_contiguous()
    _check(lib().lzs_compress_batch_packed_device(
        _ptr(out, out_off), out_off.data_ptr(), out_len.data_ptr(), _ptr(data, in_off), in_off.data_ptr(),
        None if in_len is None else in_len.data_ptr(), nb, _stream_handle(stream)))
    return out, out_len


def compress_channels_packed(data, in_off, channels, states, out, out_off, in_len=None, out_len=None, status=None, stream=None):
    """lzs_compress_channels_packed_device(): compress_channels() from packed packets to packed rooms, one packet per channel per
    call (``channels``: int32 [npackets] or None for packet b on channel b; ``states`` from new_channel_states).  Returns (out,
    out_len int32, status uint8: 0x07, or 0x0B where the room cut the packet, STATUS_ERROR for an entry that is not a block or a
    slot that is no state).  Asynchronous."""
    import torch
    nb = _packed_output(out, out_off)
    _packed_input(data, in_off, in_len, nb)
    if out_len is None:
        out_len = torch.empty(nb, dtype=torch.int32, device=data.device)
    assert out_len.is_cuda and out_len.dtype == torch.int32 and out_len.numel() == nb and out_len.is_contiguous()
    if status is None:
        status = torch.empty(nb, dtype=torch.uint8, device=data.device)
    assert status.is_cuda and status.dtype == torch.uint8 and status.numel() == nb and status.is_contiguous()
    if channels is not None:
        assert channels.is_cuda and channels.dtype == torch.int32 and channels.numel() == nb and channels.is_contiguous()
    assert states.is_cuda and states.dtype == torch.uint8 and states.is_contiguous()
    _check(lib().lzs_compress_channels_packed_device(
        _ptr(out, out_off), out_off.data_ptr(), out_len.data_ptr(), _ptr(data, in_off), in_off.data_ptr(),
        None if in_len is None else in_len.data_ptr(), None if channels is None else channels.data_ptr(), states.data_ptr(),
        status.data_ptr(), nb, _stream_handle(stream)))
    return out, out_len, status


def compact_packed(src, src_off, lengths, stream=None, dense=None, offsets=None):
    """lzs_compact_packed_device(): compact() with slot b at src[src_off[b]:] -- the rooms of compress_packed.  Returns (dense
    uint8, offsets int64 [nblocks + 1]): offsets is the scan of ``lengths`` (int32 [nblocks]), dense[offsets[b]:offsets[b + 1]] the
    first lengths[b] bytes of slot b.  ``dense`` (at least sum(lengths) bytes, not overlapping ``src``; by default as large as
    ``src``) and ``offsets`` may be passed in.  Asynchronous."""
    import torch
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 1 and src.is_contiguous()
    assert lengths.is_cuda and lengths.dtype == torch.int32 and lengths.dim() == 1 and lengths.is_contiguous()
    nb = lengths.numel()
    assert src_off.is_cuda and src_off.dtype == torch.int64 and src_off.is_contiguous() and src_off.numel() >= nb
    if offsets is None:
        offsets = torch.empty(nb + 1, dtype=torch.int64, device=src.device)
    if dense is None:
        dense = torch.empty(src.numel(), dtype=torch.uint8, device=src.device)
    assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.numel() == nb + 1 and offsets.is_contiguous()
    assert dense.is_cuda and dense.dtype == torch.uint8 and dense.is_contiguous()
    if nb == 0:
        offsets.zero_()                                            # (the C call touches nothing for an empty batch)
        return dense, offsets
    _check(lib().lzs_compact_packed_device(_ptr(dense, offsets), offsets.data_ptr(), _ptr(src, offsets), src_off.data_ptr(),
                                           lengths.data_ptr(), nb, _stream_handle(stream)))
    return dense, offsets


def compress_dense(data, in_off, in_len=None, align: int = 16, stream=None):
    """Packed blocks compressed into ONE dense byte string of independent LZS streams: compressed_bounds_packed(),
    offsets_from_sizes() at ``align`` for the rooms, one host read of their total, one allocation of the rooms, compress_packed(),
    the scan of the lengths, one host read of the dense total, one allocation of exactly that, compact_packed().  Returns (dense
    uint8 [total], offsets int64 [nblocks + 1]); stream b is dense[offsets[b]:offsets[b + 1]], and decompress_dense(dense, offsets)
    gives the blocks back.  An entry that is not a block becomes an empty stream.

    Peak device memory: the rooms (the sum of LZS_COMPRESSED_MAX(len[b]) rounded up to ``align``: 9/8 of the data and 3 to
    3 + ``align`` bytes a block) plus the result plus three small arrays -- the bounds, which become the lengths (int32 [nblocks]),
    the rooms' offsets and the result's offsets (int64 [nblocks + 1] each).  No input slots and no nblocks x max anything: the
    strided route needs nblocks * max(len) bytes of input slots and nblocks * LZS_COMPRESSED_MAX(max(len)) of output slots
    beside the same result.  Two host reads, which wait for the work before them."""
    import torch
    nb = _packed_input(data, in_off, in_len)
    if nb == 0:
        return torch.empty(0, dtype=torch.uint8, device=data.device), torch.zeros(1, dtype=torch.int64, device=data.device)
    size = compressed_bounds_packed(in_off, in_len, stream=stream)
    room_off = offsets_from_sizes(size, align, stream=stream)
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        rooms = torch.empty(int(room_off[nb].cpu()), dtype=torch.uint8, device=data.device)          # the first host read
        compress_packed(data, in_off, rooms, room_off, in_len=in_len, out_len=size, stream=stream)   # (the bounds are spent: the lengths take their place)
        offsets = offsets_from_sizes(size, 1, stream=stream)
        dense = torch.empty(int(offsets[nb].cpu()), dtype=torch.uint8, device=data.device)           # the second host read
    compact_packed(rooms, room_off, size, stream=stream, dense=dense, offsets=offsets)
    return dense, offsets


# ------------------------------------------------------ incremental interface (lzs.h)
STATUS_INPUT_STARVED, STATUS_INPUT_FINISHED, STATUS_END_MARKER = 0x01, 0x02, 0x04
STATUS_NO_OUTPUT_BUFFER_SPACE, STATUS_ERROR = 0x08, 0x10


class CompressParameters(ctypes.Structure):
    """LzsCompressParameters_t (reference c/src/liblzs/lzs.h:101-134): same public members,
    same size."""
    _fields_ = [("inPtr", _vp), ("outPtr", _vp), ("inLength", _sz), ("outLength", _sz),
                ("status", ctypes.c_uint8), ("reserved_", ctypes.c_uint8 * 14399)]


class SimpleCompressParameters(ctypes.Structure):
    """LzsSimpleCompressParameters_t (reference c/src/liblzs/lzs.h:136-166): 2112 bytes."""
    _fields_ = [("inPtr", _vp), ("outPtr", _vp), ("inLength", _sz), ("outLength", _sz),
                ("status", ctypes.c_uint8), ("reserved_", ctypes.c_uint8 * 2079)]


class DecompressParameters(ctypes.Structure):
    """LzsDecompressParameters_t (reference c/src/liblzs/lzs.h:180-211)."""
    _fields_ = [("inPtr", _vp), ("outPtr", _vp), ("inLength", _sz), ("outLength", _sz),
                ("status", ctypes.c_uint8), ("reserved_", ctypes.c_uint8 * 2063)]


class _Incremental:
    """One parameter block driven the way the reference's tools and tests drive it: set
    inPtr/inLength/outPtr/outLength, call, read back what moved."""

    def _call(self, fn, data: bytes, out_space: int, *extra):
        src = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
        dst = ctypes.create_string_buffer(max(out_space, 1))
        p = self.params
        p.inPtr, p.inLength = ctypes.addressof(src), len(data)
        p.outPtr, p.outLength = ctypes.addressof(dst), out_space
        n = fn(ctypes.addressof(p), *extra)
        if p.status & STATUS_ERROR:
            raise LzsError(LZS_E_HIP, last_error())
        assert n == out_space - p.outLength and p.outPtr == ctypes.addressof(dst) + n
        assert p.inPtr == ctypes.addressof(src) + len(data) - p.inLength
        return dst.raw[:n], len(data) - p.inLength, int(p.status)


class IncrementalCompressor(_Incremental):
    """lzs_compress_init() + lzs_compress_incremental() (reference lzs-compression.c:479-823)."""

    def __init__(self, simple: bool = False):
        """``simple``: the reference's low-memory block and lzs_simple_compress_incremental()
        (lzs-compression-simple.c: same stream, 2112-byte block)."""
        self.simple = simple
        if simple:
            self.params = SimpleCompressParameters()
            lib().lzs_simple_compress_init(ctypes.addressof(self.params))
        else:
            self.params = CompressParameters()
            lib().lzs_compress_init_full(ctypes.addressof(self.params))

    def step(self, data: bytes, out_space: int, add_end_marker: bool = False):
        """One call: returns (output bytes, input bytes consumed, status flags)."""
        fn = lib().lzs_simple_compress_incremental if self.simple else lib().lzs_compress_incremental
        return self._call(fn, data, out_space, add_end_marker)


class IncrementalDecompressor(_Incremental):
    """lzs_decompress_init() + lzs_decompress_incremental() (reference lzs-decompression.c:420-743)."""

    def __init__(self):
        self.params = DecompressParameters()
        lib().lzs_decompress_init(ctypes.addressof(self.params))

    def step(self, data: bytes, out_space: int):
        return self._call(lib().lzs_decompress_incremental, data, out_space)


def incremental_compress(data: bytes, in_chunk: int, out_chunk: int, simple: bool = False) -> bytes:
    """``data`` through lzs_compress_incremental() the way the reference's file tool drives it
    (c/src/utils/lzs-compress.c:91-134): ``in_chunk`` bytes offered and ``out_chunk`` bytes of room
    per call, unread input offered again, add_end_marker once the input is used up, until the
    call reports END_MARKER.  Returns the whole stream."""
    c, out, pos, piece, finish = IncrementalCompressor(simple), bytearray(), 0, b"", False
    status, calls = 0, 0
    while not (status & STATUS_END_MARKER):
        if not piece and not finish:
            piece = bytes(data[pos:pos + in_chunk])
            pos += len(piece)
        if not piece and (status & STATUS_INPUT_STARVED or pos >= len(data)):
            finish = True
        got, used, status = c.step(piece, out_chunk, finish)
        out += got
        piece = piece[used:]
        calls += 1
        if calls > 32 * (len(data) // max(1, min(in_chunk, out_chunk)) + 64):
            raise LzsError(LZS_E_HIP, "lzs_compress_incremental makes no progress")
    return bytes(out)


# ------------------------------------------- many channels, one packet each (lzs_channels.h)
CHANNEL_STATE_BYTES = 2112          # LZS_CHANNEL_STATE_BYTES: uint32 hist_len, reserved to 64, hist[2048]


def new_channel_states(n: int, device=None):
    """``n`` new channels: a zeroed CUDA uint8 tensor [n, CHANNEL_STATE_BYTES] (an all-zero slot is a fresh
    lzs_compress_init_full() / lzs_decompress_init(); compressor and decompressor each need their own array)."""
    import torch
    return torch.zeros((n, CHANNEL_STATE_BYTES), dtype=torch.uint8, device="cuda" if device is None else device)


def _device_channels(fn, x, in_len, channels, states, out_cap, out, out_len, status, stream):
    import torch
    assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.stride(1) == 1, \
        "packets must be a CUDA uint8 tensor [npackets, stride] with contiguous rows"
    nb = x.shape[0]
    assert states.is_cuda and states.dtype == torch.uint8 and states.dim() == 2 and states.is_contiguous() \
        and states.shape[1] == CHANNEL_STATE_BYTES, "states must be a contiguous CUDA uint8 tensor [nchannels, CHANNEL_STATE_BYTES]"
    if channels is None:
        assert states.shape[0] >= nb, "without channel ids packet b uses channel b"
    else:
        assert channels.is_cuda and channels.dtype == torch.int32 and channels.numel() == nb and channels.is_contiguous()
    if out is None:
        out = torch.empty((nb, (max(out_cap, 1) + 15) // 16 * 16), dtype=torch.uint8, device=x.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape[0] == nb and out.stride(1) == 1 and out.shape[1] >= out_cap
    if out_len is None:
        out_len = torch.empty(nb, dtype=torch.int32, device=x.device)
    assert out_len.is_cuda and out_len.dtype == torch.int32 and out_len.numel() == nb
    if status is None:
        status = torch.empty(nb, dtype=torch.uint8, device=x.device)
    assert status.is_cuda and status.dtype == torch.uint8 and status.numel() == nb
    if in_len is not None:
        assert in_len.is_cuda and in_len.dtype == torch.int32 and in_len.numel() == nb
    _check(fn(out.data_ptr(), out.stride(0) if nb > 1 else out.shape[1], out_cap, out_len.data_ptr(),
              x.data_ptr(), x.stride(0) if nb > 1 else x.shape[1],
              None if in_len is None else in_len.data_ptr(), x.shape[1],
              None if channels is None else channels.data_ptr(), states.data_ptr(), status.data_ptr(), nb,
              _stream_handle(stream)))
    return out, out_len, status


def compress_channels(x, in_len, channels, states, out_capacity: Optional[int] = None, out=None, out_len=None, status=None,
                      stream=None):
    """lzs_compress_channels_device(): row b of ``x`` (CUDA uint8 [npackets, stride], ``in_len[b]`` bytes or whole rows) is
    one packet on channel ``channels[b]`` (CUDA int32, or None: channel b), compressed with that channel's history in
    ``states`` (new_channel_states) as lzs_compress_incremental(add_end_marker) would, and the history advanced.  A channel
    may appear at most once per call (ChannelCodec splits repeated ids).  Asynchronous on ``stream``.
    Returns (slots [npackets, slot_stride] uint8, lengths int32, status uint8: LZS_C_STATUS_* bits)."""
    cap = compressed_max(x.shape[1]) if out_capacity is None else out_capacity
    return _device_channels(lib().lzs_compress_channels_device, x, in_len, channels, states, cap, out, out_len, status, stream)


def decompress_channels(x, in_len, channels, states, out_capacity: int, out=None, out_len=None, status=None, stream=None):
    """lzs_decompress_channels_device(): the reverse, with the decompressor's own ``states``; arguments as
    compress_channels, status LZS_D_STATUS_* bits (END_MARKER for a whole packet)."""
    return _device_channels(lib().lzs_decompress_channels_device, x, in_len, channels, states, out_capacity, out, out_len,
                            status, stream)


# ------------------------------------------- many packets per channel in one call (lzs_channels.h, bursts)
_BURST_WORK = {}                    # device -> the work area the burst calls reuse (grown on demand)


def channels_burst_work_bytes(npackets: int, nchannels: int) -> int:
    """lzs_channels_burst_work_bytes(): the device work area both burst calls need."""
    return int(lib().lzs_channels_burst_work_bytes(npackets, nchannels))


def channels_burst_split_work_bytes(npackets: int, nchannels: int, out_capacity: int) -> int:
    """lzs_channels_burst_split_work_bytes(): the work area with which decompress_channels_burst may split long runs over the
    device -- channels_burst_work_bytes() plus about two bytes per packet and byte of ``out_capacity``."""
    if not hasattr(lib(), "lzs_channels_burst_split_work_bytes"):      # (an older build named by LZS_LIBRARY, for A/B runs: no split)
        return channels_burst_work_bytes(npackets, nchannels)
    return int(lib().lzs_channels_burst_split_work_bytes(npackets, nchannels, out_capacity))


PACKET_RESET = 1                    # LZS_PACKET_RESET: flags[b] & 1 resets the channel's history in front of packet b


def _burst_flags(flags, nb, device):
    """``flags`` of a burst call, checked: a contiguous CUDA uint8 tensor [npackets], or None."""
    import torch
    if flags is not None:
        assert flags.is_cuda and flags.dtype == torch.uint8 and flags.is_contiguous() and flags.numel() == nb \
            and flags.device == device, "flags must be a contiguous CUDA uint8 tensor [npackets]"
    return flags


def _device_burst(fn, x, in_len, channels, states, out_cap, out, out_len, status, work, stream, split=False, flags=None):
    import torch
    assert channels is not None and channels.is_cuda and channels.dtype == torch.int32 and channels.is_contiguous() \
        and channels.numel() == x.shape[0], "channels must be a contiguous CUDA int32 tensor [npackets]"
    nb, nch = x.shape[0], states.shape[0]
    need = channels_burst_split_work_bytes(nb, nch, out_cap) if split else channels_burst_work_bytes(nb, nch)
    if work is None:
        work = _BURST_WORK.get(str(x.device))
        if work is None or work.numel() < need:
            work = torch.empty(max(need, 256), dtype=torch.uint8, device=x.device)
            _BURST_WORK[str(x.device)] = work
    assert work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous(), "work must be a contiguous CUDA uint8 tensor"
    if _burst_flags(flags, nb, x.device) is None:
        return _device_channels(lambda *a: fn(*a[:10], nch, a[10], work.data_ptr(), work.numel(), *a[11:]), x, in_len, channels,
                                states, out_cap, out, out_len, status, stream)
    fn = getattr(lib(), fn.__name__.replace("_burst_device", "_burst_flags_device"))
    return _device_channels(lambda *a: fn(*a[:9], flags.data_ptr(), a[9], nch, a[10], work.data_ptr(), work.numel(), *a[11:]), x, in_len,
                            channels, states, out_cap, out, out_len, status, stream)


def compress_channels_burst(x, in_len, channels, states, out_capacity: Optional[int] = None, out=None, out_len=None, status=None,
                            work=None, stream=None, flags=None):
    """lzs_compress_channels_burst_device(): as compress_channels, but ``channels`` (CUDA int32, required) may repeat: the packets
    of a channel are taken in row order, each with the history of the ones before it -- what ChannelCodec.compress gives, in one
    call, with no host synchronisation.  An id >= len(states) gives that packet STATUS_ERROR and length 0.  ``work``: a CUDA
    uint8 tensor of channels_burst_work_bytes() bytes or more (default: one per device, kept and reused -- give each stream
    that runs burst calls at the same time its own).  ``flags`` (CUDA uint8 [npackets], or None): a packet with PACKET_RESET set is
    compressed from an empty history, as if its channel's hist_len had been zeroed in front of it -- a reset inside the queue
    (lzs_compress_channels_burst_flags_device).  Returns (slots, lengths int32, status uint8)."""
    cap = compressed_max(x.shape[1]) if out_capacity is None else out_capacity
    return _device_burst(lib().lzs_compress_channels_burst_device, x, in_len, channels, states, cap, out, out_len, status, work,
                         stream, flags=flags)


def decompress_channels_burst(x, in_len, channels, states, out_capacity: int, out=None, out_len=None, status=None, work=None,
                              stream=None, flags=None):
    """lzs_decompress_channels_burst_device(): the reverse, on the decompressor's states -- what ChannelCodec.decompress gives,
    in one call.  Arguments as compress_channels_burst.  The default work area has channels_burst_split_work_bytes() bytes, with
    which long runs are split over the device; a caller's ``work`` decides by its size (the results are the same).
    ``flags``: as for compress_channels_burst -- a flagged packet is decoded from an empty history and starts a run of its own.
    Returns (out, lengths int32, status uint8: LZS_D_STATUS_* bits)."""
    return _device_burst(lib().lzs_decompress_channels_burst_device, x, in_len, channels, states, out_capacity, out, out_len,
                         status, work, stream, split=True, flags=flags)


# ------------------------------- packed bursts: many packets per channel, addressed by offsets (lzs_channels.h)
def channels_burst_packed_split_work_bytes(npackets: int, nchannels: int, out_bytes: int) -> int:
    """lzs_channels_burst_packed_split_work_bytes(): the work area with which decompress_channels_burst_packed may split long runs
    -- channels_burst_work_bytes() plus two bytes per byte of room, ``out_bytes`` being the sum of the rooms."""
    return int(lib().lzs_channels_burst_packed_split_work_bytes(npackets, nchannels, out_bytes))


def _device_burst_packed(fn, data, in_off, channels, states, out, out_off, in_len, out_len, status, work, stream, split, flags=None):
    import torch
    nb = _packed_output(out, out_off)
    _packed_input(data, in_off, in_len, nb)
    assert channels is not None and channels.is_cuda and channels.dtype == torch.int32 and channels.is_contiguous() \
        and channels.numel() == nb, "channels must be a contiguous CUDA int32 tensor [npackets]"
    assert states.is_cuda and states.dtype == torch.uint8 and states.dim() == 2 and states.is_contiguous() \
        and states.shape[1] == CHANNEL_STATE_BYTES, "states must be a contiguous CUDA uint8 tensor [nchannels, CHANNEL_STATE_BYTES]"
    nch = states.shape[0]
    if out_len is None:
        out_len = torch.empty(nb, dtype=torch.int32, device=data.device)
    assert out_len.is_cuda and out_len.dtype == torch.int32 and out_len.numel() == nb and out_len.is_contiguous()
    if status is None:
        status = torch.empty(nb, dtype=torch.uint8, device=data.device)
    assert status.is_cuda and status.dtype == torch.uint8 and status.numel() == nb and status.is_contiguous()
    if work is None:
        # (the rooms lie in ``out``: its size stands for their sum, which only the device knows -- and it checks)
        need = channels_burst_packed_split_work_bytes(nb, nch, out.numel()) if split else channels_burst_work_bytes(nb, nch)
        work = _BURST_WORK.get(str(data.device))
        if work is None or work.numel() < need:
            work = torch.empty(max(need, 256), dtype=torch.uint8, device=data.device)
            _BURST_WORK[str(data.device)] = work
    assert work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous(), "work must be a contiguous CUDA uint8 tensor"
    extra = ()
    if _burst_flags(flags, nb, data.device) is not None:
        fn = getattr(lib(), fn.__name__.replace("_packed_device", "_packed_flags_device"))
        extra = (flags.data_ptr(),)
    _check(fn(_ptr(out, out_off), out_off.data_ptr(), out_len.data_ptr(), _ptr(data, in_off), in_off.data_ptr(),
              None if in_len is None else in_len.data_ptr(), channels.data_ptr(), *extra, states.data_ptr(), nch, status.data_ptr(),
              work.data_ptr(), work.numel(), nb, _stream_handle(stream)))
    return out, out_len, status


def compress_channels_burst_packed(data, in_off, channels, states, out, out_off, in_len=None, out_len=None, status=None, work=None,
                                   stream=None, flags=None):
    """lzs_compress_channels_burst_packed_device(): compress_channels_burst() from packed packets to packed rooms -- a drained
    queue compressed where it lies.  Packet b is data[in_off[b]:in_off[b + 1]] (or ``in_len[b]`` bytes at in_off[b]) on channel
    ``channels[b]`` (CUDA int32, required; ids may repeat, the packets of a channel are taken in order of b) and goes to
    out[out_off[b]:out_off[b + 1]], its room.  ``work``: as for compress_channels_burst.  Returns (out, out_len int32, status uint8:
    0x07, 0x0B where the room cut the packet, STATUS_ERROR for an entry that is not a block, an id >= len(states) or a slot that is
    no state).  ``flags``: as for compress_channels_burst; a flag on an entry that is not a block is ignored.  Asynchronous."""
    return _device_burst_packed(lib().lzs_compress_channels_burst_packed_device, data, in_off, channels, states, out, out_off, in_len,
                                out_len, status, work, stream, False, flags)


def decompress_channels_burst_packed(data, in_off, channels, states, out, out_off, in_len=None, out_len=None, status=None, work=None,
                                     stream=None, flags=None):
    """lzs_decompress_channels_burst_packed_device(): the reverse, on the decompressor's states.  Arguments as
    compress_channels_burst_packed.  The default work area has channels_burst_packed_split_work_bytes() bytes for rooms of
    len(out) bytes, with which long runs are split over the device; a caller's ``work`` decides by its size (the results are the
    same).  ``flags``: as for compress_channels_burst_packed.  Returns (out, out_len int32, status uint8: LZS_D_STATUS_* bits)."""
    return _device_burst_packed(lib().lzs_decompress_channels_burst_packed_device, data, in_off, channels, states, out, out_off, in_len,
                                out_len, status, work, stream, True, flags)


def compress_channels_dense(data, in_off, channels, states, in_len=None, align: int = 16, stream=None, flags=None):
    """A drained packet queue compressed into ONE dense byte string of channel packets: compressed_bounds_packed(),
    offsets_from_sizes() at ``align`` for the rooms, one host read of their total, one allocation of the rooms,
    compress_channels_burst_packed() on ``states``, the scan of the lengths, one host read of the dense total, one allocation of
    exactly that, compact_packed().  Returns (dense uint8 [total], offsets int64 [npackets + 1], status uint8 [npackets]); packet b's
    stream is dense[offsets[b]:offsets[b + 1]] -- empty for a packet that got STATUS_ERROR --, and decompress_channels_dense(dense,
    offsets, channels, peer_states) gives the packets back -- with the same ``flags`` (as for compress_channels_burst_packed), if any
    were given.  Peak device memory: as compress_dense(), and the burst work area."""
    import torch
    nb = _packed_input(data, in_off, in_len)
    if nb == 0:
        return (torch.empty(0, dtype=torch.uint8, device=data.device), torch.zeros(1, dtype=torch.int64, device=data.device),
                torch.empty(0, dtype=torch.uint8, device=data.device))
    size = compressed_bounds_packed(in_off, in_len, stream=stream)
    room_off = offsets_from_sizes(size, align, stream=stream)
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        rooms = torch.empty(int(room_off[nb].cpu()), dtype=torch.uint8, device=data.device)          # the first host read
        _, _, status = compress_channels_burst_packed(data, in_off, channels, states, rooms, room_off, in_len=in_len, out_len=size,
                                                      stream=stream, flags=flags)                              # (the lengths take the bounds' place)
        offsets = offsets_from_sizes(size, 1, stream=stream)
        dense = torch.empty(int(offsets[nb].cpu()), dtype=torch.uint8, device=data.device)           # the second host read
    compact_packed(rooms, room_off, size, stream=stream, dense=dense, offsets=offsets)
    return dense, offsets, status


def decompress_channels_dense(data, in_off, channels, states, in_len=None, align: int = 1, stream=None, flags=None):
    """Packed channel packets decoded into ONE dense byte string by a caller who does not know their sizes:
    decompressed_sizes_packed() -- a packet's size does not depend on its channel's history --, offsets_from_sizes(), one host read
    -- the total, and the first packet that does not end in its end marker --, one allocation of exactly the total,
    decompress_channels_burst_packed() on ``states``.  Returns (dense uint8 [total], offsets int64 [npackets + 1], status uint8
    [npackets]); packet b is dense[offsets[b] : offsets[b] + size[b]].  Raises ValueError naming the first packet that does not end
    in an end marker, before any state is touched.  ``flags``: as for decompress_channels_burst_packed."""
    import torch
    nb = _packed_input(data, in_off, in_len)
    if nb == 0:
        return (torch.empty(0, dtype=torch.uint8, device=data.device), torch.zeros(1, dtype=torch.int64, device=data.device),
                torch.empty(0, dtype=torch.uint8, device=data.device))
    size, status = decompressed_sizes_packed(data, in_off, in_len, None, stream=stream)
    offsets = offsets_from_sizes(size, align, stream=stream)
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        bad = status != STATUS_END_MARKER
        first = bad.to(torch.uint8).argmax()
        top = torch.stack([offsets[nb], bad.any().to(torch.int64), first.to(torch.int64), status[first].to(torch.int64)]).cpu()   # the one host read
        del bad, first
    total, any_bad, first_bad, its_status = (int(v) for v in top)
    del top
    if any_bad:
        raise ValueError(f"decompress_channels_dense: packet {first_bad} does not end in an end marker (status 0x{its_status:02x})")
    dense = torch.empty(total, dtype=torch.uint8, device=data.device)
    decompress_channels_burst_packed(data, in_off, channels, states, dense, offsets, in_len=in_len, out_len=size, status=status,
                                     stream=stream, flags=flags)
    return dense, offsets, status


def _occurrence_rank(channels) -> np.ndarray:
    """rank[b] = how many packets before b have the same channel id."""
    ch = np.asarray(channels, dtype=np.int64).reshape(-1)
    n = ch.size
    order = np.argsort(ch, kind="stable")
    srt = ch[order]
    first = np.ones(n, dtype=bool)
    first[1:] = srt[1:] != srt[:-1]
    start = np.maximum.accumulate(np.where(first, np.arange(n), 0)) if n else np.zeros(0, dtype=np.int64)
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n) - start
    return rank


class ChannelCodec:
    """``nchannels`` channels with a compressor and a decompressor state array each (``enc_states``, ``dec_states``).
    Unlike the raw calls, a batch may name a channel more than once: it is split into launches of distinct ids, in order
    (launch k takes every channel's k-th packet), so that packet k of a channel always sees its packets before k."""

    def __init__(self, nchannels: int, device=None):
        self.enc_states = new_channel_states(nchannels, device)
        self.dec_states = new_channel_states(nchannels, device)

    def _run(self, call, states, x, in_len, channels, out_cap, stream, resets=None):
        import torch
        ids = np.asarray(channels, dtype=np.int64).reshape(-1)
        nb = x.shape[0]
        rs = np.zeros(nb, dtype=bool) if resets is None else (np.asarray(resets, dtype=np.int64).reshape(-1) & PACKET_RESET) != 0
        assert rs.size == nb, "resets: one entry a packet"

        assert ids.size == nb and (nb == 0 or (ids.min() >= 0 and ids.max() < states.shape[0])), "channel ids out of range"
        out = torch.empty((nb, (max(out_cap, 1) + 15) // 16 * 16), dtype=torch.uint8, device=x.device)
        out_len = torch.empty(nb, dtype=torch.int32, device=x.device)
        status = torch.empty(nb, dtype=torch.uint8, device=x.device)
        rank = _occurrence_rank(ids)
        for r in range(int(rank.max()) + 1 if nb else 0):
            sel = np.nonzero(rank == r)[0]
            hit = ids[sel][rs[sel]]
            if hit.size:             # the reset: hist_len = 0 in front of this launch, in stream order
                with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
                    states[:, :4].index_fill_(0, torch.from_numpy(hit).to(x.device), 0)
            if sel.size == nb:       # every id once: one launch over the caller's own tensors
                call(x, in_len, torch.from_numpy(ids.astype(np.int32)).to(x.device), states, out_cap, out, out_len, status, stream)
                break
            idx = torch.from_numpy(sel).to(x.device)
            o, ol, st = call(x.index_select(0, idx).contiguous(), None if in_len is None else in_len.index_select(0, idx).contiguous(),
                             torch.from_numpy(ids[sel].astype(np.int32)).to(x.device), states, out_cap, None, None, None, stream)
            out[idx, :o.shape[1]] = o
            out_len[idx] = ol
            status[idx] = st
        return out, out_len, status

    def compress(self, x, in_len, channels, out_capacity: Optional[int] = None, stream=None, resets=None):
        """Row b of ``x`` on channel ``channels[b]`` (a host sequence; ids may repeat).  ``resets`` (a host sequence, one entry a
        packet, or None): where PACKET_RESET is set the channel's hist_len is zeroed in front of the launch that takes the packet --
        the rule of the burst calls' ``flags``, written out.  Returns (slots, lengths, status)."""
        cap = compressed_max(x.shape[1]) if out_capacity is None else out_capacity
        return self._run(lambda *a: compress_channels(*a[:4], out_capacity=a[4], out=a[5], out_len=a[6], status=a[7], stream=a[8]),
                         self.enc_states, x, in_len, channels, cap, stream, resets)

    def decompress(self, x, in_len, channels, out_capacity: int, stream=None, resets=None):
        """The reverse on the decompressor states; ``resets`` as for compress.  Returns (out, lengths, status)."""
        return self._run(lambda *a: decompress_channels(*a[:4], out_capacity=a[4], out=a[5], out_len=a[6], status=a[7], stream=a[8]),
                         self.dec_states, x, in_len, channels, out_capacity, stream, resets)

