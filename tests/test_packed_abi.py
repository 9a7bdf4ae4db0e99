"""CPU-side checks of the packed calls (include/lzs/lzs_batch.h "PACKED streams", lzs_channels.h): both headers compile from
C99 and C++17 with the four prototypes taken through function pointers, the symbols are exported from both libraries, the
package has the five front-ends, every bad argument is refused with the call's name and a message before the device is asked,
and a valid call without a device says so."""
import ctypes
import os
import subprocess

import pytest

import lzs_compression_amd as lzs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INC = os.path.join(ROOT, "include")
OFFSETS, SIZES = "lzs_offsets_from_sizes_device", "lzs_decompressed_size_packed_device"
BLOCKS, CHANNELS = "lzs_decompress_batch_packed_device", "lzs_decompress_channels_packed_device"
CALLS = (OFFSETS, SIZES, BLOCKS, CHANNELS)
PYTHON = ("offsets_from_sizes", "decompressed_sizes_packed", "decompress_packed", "decompress_channels_packed", "decompress_dense")

PROGRAM = r'''
#include "lzs.h"
#include "lzs_batch.h"
#include "lzs_channels.h"
#include <stdio.h>
int main(void) {
    int (*scan)(uint64_t *, const uint32_t *, size_t, size_t, void *) = lzs_offsets_from_sizes_device;
    int (*size)(uint32_t *, uint8_t *, const void *, const uint64_t *, const uint32_t *, size_t, size_t, void *) =
        lzs_decompressed_size_packed_device;
    int (*blocks)(void *, const uint64_t *, uint32_t *, const void *, const uint64_t *, const uint32_t *, size_t, void *) =
        lzs_decompress_batch_packed_device;
    int (*channels)(void *, const uint64_t *, uint32_t *, const void *, const uint64_t *, const uint32_t *, const uint32_t *, void *,
                    uint8_t *, size_t, void *) = lzs_decompress_channels_packed_device;
    /* (empty batches: LZS_OK without a device; the scan without its output: LZS_E_ARG) */
    printf("%d %d %d %d\n", scan(0, 0, 1, 0, 0), size(0, 0, 0, 0, 0, 0, 0, 0), blocks(0, 0, 0, 0, 0, 0, 0, 0),
           channels(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0));
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


def test_headers_compile_as_c99_and_cxx17_with_the_four_prototypes(tmp_path):
    assert _build_and_run(tmp_path, "gcc", "c99", ".c") == ["-3", "0", "0", "0"]
    assert _build_and_run(tmp_path, "g++", "c++17", ".cc") == ["-3", "0", "0", "0"]


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


def _scan(offsets=0x1000, size=0x2000, align=16, nblocks=4):
    return getattr(lzs.lib(), OFFSETS)(_p(offsets), _p(size), align, nblocks, None)


def _sizes(size=0x2000, status=0x3000, d_in=0x1001, in_off=0x5000, in_len=0x4000, limit=0xFFFFFFFF, nblocks=4):
    return getattr(lzs.lib(), SIZES)(_p(size), _p(status), _p(d_in), _p(in_off), _p(in_len), limit, nblocks, None)


def _blocks(out=0x9003, out_off=0x6000, out_len=0x2000, d_in=0x1001, in_off=0x5000, in_len=0x4000, nblocks=4):
    return getattr(lzs.lib(), BLOCKS)(_p(out), _p(out_off), _p(out_len), _p(d_in), _p(in_off), _p(in_len), nblocks, None)


def _channels(out=0x9003, out_off=0x6000, out_len=0x2000, d_in=0x1001, in_off=0x5000, in_len=0x4000, channel=0x7000, states=0x8000,
              status=0x3000, nblocks=4):
    return getattr(lzs.lib(), CHANNELS)(_p(out), _p(out_off), _p(out_len), _p(d_in), _p(in_off), _p(in_len), _p(channel), _p(states),
                                        _p(status), nblocks, None)


BAD = [
    (_scan, OFFSETS, dict(offsets=0), "offsets is NULL"), (_scan, OFFSETS, dict(size=0), "size is NULL"),
    (_scan, OFFSETS, dict(offsets=0x1004), "not 8-byte aligned"), (_scan, OFFSETS, dict(nblocks=0x80000000), "too many blocks"),
    (_scan, OFFSETS, dict(align=0), "align"), (_scan, OFFSETS, dict(align=3), "align"), (_scan, OFFSETS, dict(align=512), "align"),
    (_scan, OFFSETS, dict(align=24), "align"),
    (_sizes, SIZES, dict(size=0), "size is NULL"), (_sizes, SIZES, dict(d_in=0), "input is NULL"), (_sizes, SIZES, dict(in_off=0), "in_off is NULL"),
    (_sizes, SIZES, dict(in_off=0x5004), "d_in_off is not 8-byte aligned"), (_sizes, SIZES, dict(size=0x4000), "same array"),
    (_sizes, SIZES, dict(nblocks=0x80000000), "too many blocks"), (_sizes, SIZES, dict(limit=1 << 32), "limit"),
    (_sizes, SIZES, dict(limit=(1 << 64) - 1), "limit"),
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
    assert _sizes(nblocks=0, size=0, d_in=0, in_off=0, limit=1 << 40) == lzs.api.LZS_OK
    assert _blocks(nblocks=0, out=0, out_off=0, out_len=0, d_in=0, in_off=0) == lzs.api.LZS_OK
    assert _channels(nblocks=0, out=0, out_off=0, out_len=0, d_in=0, in_off=0, states=0) == lzs.api.LZS_OK


@pytest.mark.parametrize("fn,kw", [(_scan, dict()), (_scan, dict(align=1)), (_scan, dict(align=256, nblocks=0, size=0)), (_sizes, dict()),
                                   (_sizes, dict(status=0, in_len=0, limit=0)), (_blocks, dict()), (_blocks, dict(in_len=0)),
                                   (_channels, dict()), (_channels, dict(channel=0, status=0, in_len=0))])
def test_a_valid_call_without_a_device_says_so(fn, kw):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    A = lzs.api
    rc = fn(**kw)
    assert rc == A.LZS_E_NO_DEVICE and "no HIP device" in A.last_error(), (fn.__name__, kw, rc, A.last_error())
