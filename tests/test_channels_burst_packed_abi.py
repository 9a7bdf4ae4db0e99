"""CPU-side checks of the packed burst calls (include/lzs/lzs_channels.h "PACKED BURSTS"): the header compiles from
C99 and C++17 with the three prototypes taken through function pointers, the symbols are exported from both libraries and installed
by `make install`, the package has the five front-ends, the split work-area size has its properties, every bad argument is refused
with the call's name and a message before the device is asked, an empty call needs nothing, and a valid call without a device says
so."""
import ctypes
import os
import subprocess

import pytest

import lzs_compression_amd as lzs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INC = os.path.join(ROOT, "include")
SIZE, COMPRESS, DECOMPRESS = ("lzs_channels_burst_packed_split_work_bytes", "lzs_compress_channels_burst_packed_device",
                              "lzs_decompress_channels_burst_packed_device")
CALLS = (SIZE, COMPRESS, DECOMPRESS)
PYTHON = ("channels_burst_packed_split_work_bytes", "compress_channels_burst_packed", "decompress_channels_burst_packed",
          "compress_channels_dense", "decompress_channels_dense")
SIZE_MAX = ctypes.c_size_t(-1).value
CHANNELS_MAX = 0x7FFFFFFF

PROGRAM = r'''
#include "lzs.h"
#include "lzs_batch.h"
#include "lzs_channels.h"
#include <stdio.h>
typedef int (*burst_fn)(void *, const uint64_t *, uint32_t *, const void *, const uint64_t *, const uint32_t *, const uint32_t *, void *,
                        size_t, uint8_t *, void *, size_t, size_t, void *);
int main(void) {
    size_t (*size)(size_t, size_t, uint64_t) = lzs_channels_burst_packed_split_work_bytes;
    burst_fn compress = lzs_compress_channels_burst_packed_device, decompress = lzs_decompress_channels_burst_packed_device;
    /* (empty calls: LZS_OK without a device; one packet and nothing else: LZS_E_ARG) */
    printf("%d %d %d %d %d\n", compress(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), decompress(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
           compress(0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0), decompress(0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0),
           size(3, 2, 1000) == lzs_channels_burst_work_bytes(3, 2) + 2000);
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


def test_the_header_compiles_as_c99_and_cxx17_with_the_three_prototypes(tmp_path):
    assert _build_and_run(tmp_path, "gcc", "c99", ".c") == ["0", "0", "-3", "-3", "1"]
    assert _build_and_run(tmp_path, "g++", "c++17", ".cc") == ["0", "0", "-3", "-3", "1"]


def test_the_calls_are_exported_and_in_the_package():
    variants = ctypes.CDLL(os.path.join(ROOT, "lzs_compression_amd", "liblzs_variants.so"))
    header = open(os.path.join(INC, "lzs", "lzs_channels.h")).read()
    for call in CALLS:
        assert hasattr(lzs.lib(), call) and hasattr(variants, call), call
        assert call + "(" in header, call
    for name in PYTHON:
        assert name in lzs.__all__ and getattr(lzs, name) is getattr(lzs.api, name), name


def test_make_install_installs_the_header_and_the_symbols(tmp_path):
    prefix = tmp_path / "prefix"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lzs_compression_amd", "csrc"), "install", f"PREFIX={prefix}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    header = (prefix / "include" / "lzs" / "lzs_channels.h").read_text()
    installed = ctypes.CDLL(str(prefix / "lib" / "liblzs.so.4"))
    for call in CALLS:
        assert call + "(" in header and hasattr(installed, call), call


# ---- the size of the larger work area
def _size(npackets, nchannels, out_bytes):
    return lzs.channels_burst_packed_split_work_bytes(npackets, nchannels, out_bytes)


def test_the_split_size_is_the_burst_size_and_two_bytes_per_byte_of_room():
    for n, nch in ((0, 0), (1, 1), (7, 3), (65536, 16384), (CHANNELS_MAX, CHANNELS_MAX)):
        base = lzs.channels_burst_work_bytes(n, nch)
        assert _size(n, nch, 0) == base
        for out_bytes in (1, 1500, 51 << 20, 1 << 40):
            got = _size(n, nch, out_bytes)
            assert got >= base and got >= base + 2 * out_bytes and got == base + 2 * out_bytes, (n, nch, out_bytes)


def test_the_split_size_is_monotone_in_each_argument():
    grid_n, grid_ch, grid_out = (0, 1, 2, 255, 256, 70000), (1, 2, 1000, 1 << 20), (0, 1, 2, 4095, 4096, 1 << 33)
    for nch in grid_ch:
        for out_bytes in grid_out:
            sizes = [_size(n, nch, out_bytes) for n in grid_n]
            assert sizes == sorted(sizes), (nch, out_bytes)
    for n in grid_n:
        for out_bytes in grid_out:
            sizes = [_size(n, nch, out_bytes) for nch in grid_ch]
            assert sizes == sorted(sizes), (n, out_bytes)
        for nch in grid_ch:
            sizes = [_size(n, nch, out_bytes) for out_bytes in grid_out]
            assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (n, nch)


def test_the_split_size_is_size_max_where_it_does_not_fit():
    base = lzs.channels_burst_work_bytes(10, 4)
    fits = (SIZE_MAX - base) // 2
    assert _size(10, 4, fits) == base + 2 * fits
    assert _size(10, 4, fits + 1) == SIZE_MAX
    assert _size(10, 4, (1 << 64) - 1) == SIZE_MAX and _size(10, 4, 1 << 63) == SIZE_MAX


# ---- the arguments: made-up addresses, nothing is dereferenced before the device is asked
def _p(v):
    return ctypes.c_void_p(v) if v else None


def _call(name, out=0x9003, out_off=0x6000, out_len=0x2000, d_in=0x1001, in_off=0x5000, in_len=0x4000, channel=0x7000, states=0x8000,
          nchannels=3, status=0x3000, work=0x10000, work_bytes=None, npackets=4):
    if work_bytes is None:
        work_bytes = lzs.channels_burst_work_bytes(min(npackets, CHANNELS_MAX), nchannels)
    return getattr(lzs.lib(), name)(_p(out), _p(out_off), _p(out_len), _p(d_in), _p(in_off), _p(in_len), _p(channel), _p(states),
                                    nchannels, _p(status), _p(work), work_bytes, npackets, None)


BAD = [(name, kw, words) for name in (COMPRESS, DECOMPRESS) for kw, words in (
    (dict(out_len=0), "out_len is NULL"), (dict(states=0), "states is NULL"), (dict(channel=0), "channel is NULL"),
    (dict(work=0), "work is NULL"), (dict(in_off=0), "in_off is NULL"), (dict(out_off=0), "out_off is NULL"),
    (dict(out=0), "output is NULL"), (dict(d_in=0), "input is NULL"),
    (dict(in_off=0x5004), "d_in_off is not 8-byte aligned"), (dict(out_off=0x6001), "d_out_off is not 8-byte aligned"),
    (dict(states=0x8002), "states is not 4-byte aligned"), (dict(work=0x10080), "work is not 256-byte aligned"),
    (dict(work_bytes=0), "work_bytes 0 is smaller than lzs_channels_burst_work_bytes()"),
    (dict(work_bytes=lzs.channels_burst_work_bytes(4, 3) - 1), "is smaller than lzs_channels_burst_work_bytes()"),
    (dict(nchannels=0), "no channels for 4 packets"), (dict(nchannels=CHANNELS_MAX + 1), "too many channels"),
    (dict(npackets=CHANNELS_MAX + 1), "too many"), (dict(out_len=0x4000), "same array"))]


@pytest.mark.parametrize("name,kw,words", BAD, ids=[f"{n}-{'-'.join(f'{k}={v:#x}' for k, v in kw.items())}" for n, kw, _ in BAD])
def test_argument_errors_are_refused_before_the_device(name, kw, words):
    A = lzs.api
    rc = _call(name, **kw)
    assert rc == A.LZS_E_ARG and words in A.last_error() and name in A.last_error(), (kw, rc, A.last_error())


@pytest.mark.parametrize("name", (COMPRESS, DECOMPRESS))
def test_an_empty_call_is_ok_and_needs_nothing(name):
    assert _call(name, npackets=0, out=0, out_off=0, out_len=0, d_in=0, in_off=0, in_len=0, channel=0, states=0, nchannels=0, status=0,
                 work=0, work_bytes=0) == lzs.api.LZS_OK


@pytest.mark.parametrize("kw", (dict(), dict(in_len=0, status=0), dict(work_bytes="split")), ids=("all", "optional-null", "split-size"))
@pytest.mark.parametrize("name", (COMPRESS, DECOMPRESS))
def test_a_valid_call_without_a_device_says_so(name, kw):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    A = lzs.api
    if kw.get("work_bytes") == "split":
        kw = dict(work_bytes=lzs.channels_burst_packed_split_work_bytes(4, 3, 6000))
    rc = _call(name, **kw)
    assert rc == A.LZS_E_NO_DEVICE and "no HIP device" in A.last_error(), (name, kw, rc, A.last_error())
