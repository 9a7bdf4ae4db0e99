"""CPU-side checks of the four flags entries of include/lzs/lzs_channels.h (history resets inside a burst, LZS_PACKET_RESET;
DESIGN.md 3.18): the header compiles from C99 and C++17 with the prototypes taken through function pointers and the constant 1, the
symbols are exported from both libraries, the package has PACKET_RESET and the ``flags`` / ``resets`` keywords, every bad argument of
the burst entries is refused with the flags entry's own name before the device is asked -- with flags given and with NULL --, an empty
call touches nothing, and a valid call without a device says so."""
import ctypes
import inspect
import os
import subprocess

import pytest

import lzs_compression_amd as lzs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INC = os.path.join(ROOT, "include")
STRIDED = ("lzs_compress_channels_burst_flags_device", "lzs_decompress_channels_burst_flags_device")
PACKED = ("lzs_compress_channels_burst_packed_flags_device", "lzs_decompress_channels_burst_packed_flags_device")
CHANNELS_MAX = 0x7FFFFFFF

PROGRAM = r'''
#include "lzs.h"
#include "lzs_batch.h"
#include "lzs_channels.h"
#include <stdio.h>
typedef int (*strided_fn)(void *, size_t, size_t, uint32_t *, const void *, size_t, const uint32_t *, size_t, const uint32_t *,
                          const uint8_t *, void *, size_t, uint8_t *, void *, size_t, size_t, void *);
typedef int (*packed_fn)(void *, const uint64_t *, uint32_t *, const void *, const uint64_t *, const uint32_t *, const uint32_t *,
                         const uint8_t *, void *, size_t, uint8_t *, void *, size_t, size_t, void *);
int main(void) {
    strided_fn c = lzs_compress_channels_burst_flags_device, d = lzs_decompress_channels_burst_flags_device;
    packed_fn pc = lzs_compress_channels_burst_packed_flags_device, pd = lzs_decompress_channels_burst_packed_flags_device;
    /* (empty calls: LZS_OK without a device; one packet and nothing else: LZS_E_ARG) */
    printf("%d %d %d %d %d %d %d %d %u\n", c(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), d(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
           pc(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), pd(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
           c(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0), d(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
           pc(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0), pd(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0), LZS_PACKET_RESET);
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


def test_the_header_compiles_as_c99_and_cxx17_with_the_four_prototypes(tmp_path):
    want = ["0", "0", "0", "0", "-3", "-3", "-3", "-3", "1"]
    assert _build_and_run(tmp_path, "gcc", "c99", ".c") == want
    assert _build_and_run(tmp_path, "g++", "c++17", ".cc") == want


def test_the_calls_are_exported_and_in_the_package():
    variants = ctypes.CDLL(os.path.join(ROOT, "lzs_compression_amd", "liblzs_variants.so"))
    header = open(os.path.join(INC, "lzs", "lzs_channels.h")).read()
    for call in STRIDED + PACKED:
        assert hasattr(lzs.lib(), call) and hasattr(variants, call), call
        assert call + "(" in header, call
    assert "#define LZS_PACKET_RESET 0x01u" in header
    assert lzs.PACKET_RESET == 1 and "PACKET_RESET" in lzs.__all__
    for name in ("compress_channels_burst", "decompress_channels_burst", "compress_channels_burst_packed", "decompress_channels_burst_packed",
                 "compress_channels_dense", "decompress_channels_dense"):
        assert inspect.signature(getattr(lzs, name)).parameters["flags"].default is None, name
    for name in ("compress", "decompress"):
        assert inspect.signature(getattr(lzs.ChannelCodec, name)).parameters["resets"].default is None, name


# ---- the arguments: made-up addresses, nothing is dereferenced before the device is asked
def _p(v):
    return ctypes.c_void_p(v) if v else None


def _strided(name, out=0x1000, out_len=0x3000, d_in=0x1000, in_len=0x4000, channel=0x5000, flags=0x6001, states=0x2000, nchannels=8,
             work=0x100000, work_bytes=None, npackets=4):
    if work_bytes is None:
        work_bytes = lzs.channels_burst_work_bytes(min(npackets, CHANNELS_MAX), nchannels)
    return getattr(lzs.lib(), name)(_p(out), 128, 100, _p(out_len), _p(d_in), 128, _p(in_len), 64, _p(channel), _p(flags), _p(states), nchannels,
                                    None, _p(work), work_bytes, npackets, None)


def _packed(name, out=0x9003, out_off=0x6000, out_len=0x2000, d_in=0x1001, in_off=0x5000, in_len=0x4000, channel=0x7000, flags=0x7801,
            states=0x8000, nchannels=3, status=0x3000, work=0x10000, work_bytes=None, npackets=4):
    if work_bytes is None:
        work_bytes = lzs.channels_burst_work_bytes(min(npackets, CHANNELS_MAX), nchannels)
    return getattr(lzs.lib(), name)(_p(out), _p(out_off), _p(out_len), _p(d_in), _p(in_off), _p(in_len), _p(channel), _p(flags), _p(states),
                                    nchannels, _p(status), _p(work), work_bytes, npackets, None)


BAD_STRIDED = ((dict(channel=0), "channel is NULL"), (dict(states=0), "states is NULL"), (dict(out_len=0), "out_len is NULL"),
               (dict(work=0), "work is NULL"), (dict(work_bytes=lzs.channels_burst_work_bytes(4, 8) - 1), "smaller than"),
               (dict(states=0x2002), "aligned"), (dict(work=0x100010), "aligned"), (dict(out_len=0x3000, in_len=0x3000), "same array"),
               (dict(nchannels=0), "no channels"), (dict(nchannels=CHANNELS_MAX + 1), "too many channels"),
               (dict(npackets=0x80000000, work_bytes=1 << 62), "too many packets"), (dict(d_in=0), "input is NULL"), (dict(out=0), "output is NULL"))
BAD_PACKED = ((dict(out_len=0), "out_len is NULL"), (dict(states=0), "states is NULL"), (dict(channel=0), "channel is NULL"),
              (dict(work=0), "work is NULL"), (dict(in_off=0), "in_off is NULL"), (dict(out_off=0), "out_off is NULL"),
              (dict(out=0), "output is NULL"), (dict(d_in=0), "input is NULL"),
              (dict(in_off=0x5004), "d_in_off is not 8-byte aligned"), (dict(out_off=0x6001), "d_out_off is not 8-byte aligned"),
              (dict(states=0x8002), "states is not 4-byte aligned"), (dict(work=0x10080), "work is not 256-byte aligned"),
              (dict(work_bytes=0), "work_bytes 0 is smaller than lzs_channels_burst_work_bytes()"),
              (dict(nchannels=0), "no channels for 4 packets"), (dict(nchannels=CHANNELS_MAX + 1), "too many channels"),
              (dict(npackets=CHANNELS_MAX + 1), "too many"), (dict(out_len=0x4000), "same array"))
BAD = [(_strided, name, kw, words) for name in STRIDED for kw, words in BAD_STRIDED] + \
      [(_packed, name, kw, words) for name in PACKED for kw, words in BAD_PACKED]


@pytest.mark.parametrize("flags", (0, 0x6001), ids=("null-flags", "flags"))
@pytest.mark.parametrize("call,name,kw,words", BAD, ids=[f"{n}-{'-'.join(f'{k}={v:#x}' for k, v in kw.items())}" for _, n, kw, _ in BAD])
def test_argument_errors_are_refused_before_the_device(call, name, kw, words, flags):
    A = lzs.api
    rc = call(name, flags=flags, **kw)
    assert rc == A.LZS_E_ARG and words in A.last_error() and name + ":" in A.last_error(), (kw, rc, A.last_error())


@pytest.mark.parametrize("name", STRIDED + PACKED)
def test_an_empty_call_is_ok_and_needs_nothing(name):
    if name in STRIDED:
        rc = _strided(name, npackets=0, out=0, out_len=0, d_in=0, in_len=0, channel=0, flags=0, states=0, nchannels=0, work=0, work_bytes=0)
    else:
        rc = _packed(name, npackets=0, out=0, out_off=0, out_len=0, d_in=0, in_off=0, in_len=0, channel=0, flags=0, states=0, nchannels=0,
                     status=0, work=0, work_bytes=0)
    assert rc == lzs.api.LZS_OK


@pytest.mark.parametrize("flags", (0, 0x6001), ids=("null-flags", "unaligned-flags"))
@pytest.mark.parametrize("name", STRIDED + PACKED)
def test_a_valid_call_without_a_device_says_so(name, flags):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    A = lzs.api
    rc = (_strided if name in STRIDED else _packed)(name, flags=flags)
    assert rc == A.LZS_E_NO_DEVICE and "no HIP device" in A.last_error(), (name, rc, A.last_error())
