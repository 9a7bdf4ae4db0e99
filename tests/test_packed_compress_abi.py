"""CPU-side checks of the packed compress calls (include/lzs/lzs_batch.h "PACKED COMPRESSION", lzs_channels.h):
both headers compile from C99 and C++17 with the five prototypes taken through function pointers, the symbols are exported from
both libraries, the package has the five front-ends, every bad argument is refused with the call's name and a message before
the device is asked, empty batches need nothing, and a valid call without a device says so."""
import ctypes
import os
import subprocess

import pytest

import lzs_compression_amd as lzs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INC = os.path.join(ROOT, "include")
BOUND, BLOCKS, CHANNELS = "lzs_compressed_bound_packed_device", "lzs_compress_batch_packed_device", "lzs_compress_channels_packed_device"
COMPACT = "lzs_compact_packed_device"
CALLS = (BOUND, BLOCKS, CHANNELS, COMPACT)
PYTHON = ("compressed_bounds_packed", "compress_packed", "compress_channels_packed", "compact_packed", "compress_dense")

PROGRAM = r'''
#include "lzs.h"
#include "lzs_batch.h"
#include "lzs_channels.h"
#include <stdio.h>
int main(void) {
    int (*bound)(uint32_t *, const uint64_t *, const uint32_t *, size_t, void *) = lzs_compressed_bound_packed_device;
    int (*blocks)(void *, const uint64_t *, uint32_t *, const void *, const uint64_t *, const uint32_t *, size_t, void *) =
        lzs_compress_batch_packed_device;
    int (*channels)(void *, const uint64_t *, uint32_t *, const void *, const uint64_t *, const uint32_t *, const uint32_t *, void *,
                    uint8_t *, size_t, void *) = lzs_compress_channels_packed_device;
    int (*compact)(void *, uint64_t *, const void *, const uint64_t *, const uint32_t *, size_t, void *) = lzs_compact_packed_device;
    int (*scan)(uint64_t *, const uint32_t *, size_t, size_t, void *) = lzs_offsets_from_sizes_device;
    /* (empty batches: LZS_OK without a device; the scan without its output, the bounds without theirs: LZS_E_ARG) */
    printf("%d %d %d %d %d %d\n", bound(0, 0, 0, 0, 0), blocks(0, 0, 0, 0, 0, 0, 0, 0), channels(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
           compact(0, 0, 0, 0, 0, 0, 0), scan(0, 0, 1, 0, 0), bound(0, 0, 0, 1, 0));
    return 0;
}
'''


def _build_and_run(tmp_path, compiler, std, suffix):
    src = tmp_path / f"t{suffix}"
    src.write_text(PROGRAM)
    exe = tmp_path / f"t_{compiler}"
    subprocess.run([compiler, f"-std={std}", "-Wall", "-Werror", f"-I{INC}/lzs", str(src),
                    f"-L{ROOT}/lzs_compression_amd", "-llzs", f"-Wl,-rpath,{ROOT}/lzs_compression_amd", "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()


def test_headers_compile_as_c99_and_cxx17_with_the_five_prototypes(tmp_path):
    assert _build_and_run(tmp_path, "gcc", "c99", ".c") == ["0", "0", "0", "0", "-3", "-3"]
    assert _build_and_run(tmp_path, "g++", "c++17", ".cc") == ["0", "0", "0", "0", "-3", "-3"]


def test_the_calls_are_exported_and_in_the_package():
    variants = ctypes.CDLL(os.path.join(ROOT, "lzs_compression_amd", "liblzs_variants.so"))
    batch, channels = (open(os.path.join(INC, "lzs", h)).read() for h in ("lzs_batch.h", "lzs_channels.h"))
    for call in CALLS:
        assert hasattr(lzs.lib(), call) and hasattr(variants, call), call
        assert call in (channels if call == CHANNELS else batch), call
    for name in PYTHON:
        assert name in lzs.__all__ and getattr(lzs, name) is getattr(lzs.api, name), name


# ---- the arguments: made-up addresses, nothing is dereferenced before the device is asked
def _p(v):
    return ctypes.c_void_p(v) if v else None


def _bound(bound=0x2000, in_off=0x5000, in_len=0x4000, nblocks=4):
    return getattr(lzs.lib(), BOUND)(_p(bound), _p(in_off), _p(in_len), nblocks, None)


def _blocks(out=0x9003, out_off=0x6000, out_len=0x2000, d_in=0x1001, in_off=0x5000, in_len=0x4000, nblocks=4):
    return getattr(lzs.lib(), BLOCKS)(_p(out), _p(out_off), _p(out_len), _p(d_in), _p(in_off), _p(in_len), nblocks, None)


def _channels(out=0x9003, out_off=0x6000, out_len=0x2000, d_in=0x1001, in_off=0x5000, in_len=0x4000, channel=0x7000, states=0x8000,
              status=0x3000, nblocks=4):
    return getattr(lzs.lib(), CHANNELS)(_p(out), _p(out_off), _p(out_len), _p(d_in), _p(in_off), _p(in_len), _p(channel), _p(states),
                                        _p(status), nblocks, None)


def _compact(dense=0xA001, offsets=0xB000, src=0x9003, src_off=0x6000, length=0x2000, nblocks=4):
    return getattr(lzs.lib(), COMPACT)(_p(dense), _p(offsets), _p(src), _p(src_off), _p(length), nblocks, None)


BAD = [
    (_bound, BOUND, dict(bound=0), "bound is NULL"), (_bound, BOUND, dict(in_off=0), "in_off is NULL"),
    (_bound, BOUND, dict(in_off=0x5004), "d_in_off is not 8-byte aligned"), (_bound, BOUND, dict(bound=0x4000), "same array"),
    (_bound, BOUND, dict(nblocks=0x80000000), "too many blocks"),
    (_compact, COMPACT, dict(dense=0), "dense is NULL"), (_compact, COMPACT, dict(offsets=0), "offsets is NULL"),
    (_compact, COMPACT, dict(src=0), "src is NULL"), (_compact, COMPACT, dict(src_off=0), "src_off is NULL"),
    (_compact, COMPACT, dict(length=0), "len is NULL"), (_compact, COMPACT, dict(offsets=0xB004), "d_offsets is not 8-byte aligned"),
    (_compact, COMPACT, dict(src_off=0x6001), "d_src_off is not 8-byte aligned"), (_compact, COMPACT, dict(nblocks=0x80000000), "too many blocks"),
]
for _fn, _name in ((_blocks, BLOCKS), (_channels, CHANNELS)):
    BAD += [(_fn, _name, dict(out=0), "output is NULL"), (_fn, _name, dict(out_off=0), "out_off is NULL"), (_fn, _name, dict(out_len=0), "out_len is NULL"),
            (_fn, _name, dict(d_in=0), "input is NULL"), (_fn, _name, dict(in_off=0), "in_off is NULL"),
            (_fn, _name, dict(out_off=0x6002), "d_out_off is not 8-byte aligned"), (_fn, _name, dict(in_off=0x5001), "d_in_off is not 8-byte aligned"),
            (_fn, _name, dict(out_len=0x4000), "same array"), (_fn, _name, dict(nblocks=0x80000000), "too many blocks")]
BAD += [(_channels, CHANNELS, dict(states=0), "states is NULL"), (_channels, CHANNELS, dict(states=0x8002), "states is not 4-byte aligned")]


@pytest.mark.parametrize("fn,name,kw,words", BAD, ids=[f"{n}-{'-'.join(f'{k}={v:#x}' for k, v in kw.items())}" for _, n, kw, _ in BAD])
def test_argument_errors_are_refused_before_the_device(fn, name, kw, words):
    A = lzs.api
    rc = fn(**kw)
    assert rc == A.LZS_E_ARG and words in A.last_error() and name in A.last_error(), (kw, rc, A.last_error())


def test_empty_batches_are_ok_and_need_nothing():
    assert _bound(nblocks=0, bound=0, in_off=0, in_len=0) == lzs.api.LZS_OK
    assert _blocks(nblocks=0, out=0, out_off=0, out_len=0, d_in=0, in_off=0) == lzs.api.LZS_OK
    assert _channels(nblocks=0, out=0, out_off=0, out_len=0, d_in=0, in_off=0, states=0) == lzs.api.LZS_OK
    assert _compact(nblocks=0, dense=0, offsets=0, src=0, src_off=0, length=0) == lzs.api.LZS_OK


@pytest.mark.parametrize("fn,kw", [(_bound, dict()), (_bound, dict(in_len=0)), (_blocks, dict()), (_blocks, dict(in_len=0)),
                                   (_channels, dict()), (_channels, dict(channel=0, status=0, in_len=0)), (_compact, dict())])
def test_a_valid_call_without_a_device_says_so(fn, kw):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    A = lzs.api
    rc = fn(**kw)
    assert rc == A.LZS_E_NO_DEVICE and "no HIP device" in A.last_error(), (fn.__name__, kw, rc, A.last_error())
