"""CPU-side checks of lzs_channels_burst_split_work_bytes (include/lzs/lzs_channels.h): the larger work area with which
lzs_decompress_channels_burst_device may split long runs over the device.  The header compiles from C99 and C++ beside lzs.h
with the new prototype, the symbol is exported and installed, the size is monotone in each argument, never below the burst
size and holds two bytes per packet and byte of out_cap, SIZE_MAX where that does not fit; and with a work area of that size
the decode entry refuses every bad argument as before and says so when there is no device."""
import ctypes
import os
import subprocess

import pytest

import lzs_compression_amd as lzs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "lzs", "lzs_channels.h")
DECODE = "lzs_decompress_channels_burst_device"
SIZE_MAX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1

PROGRAM = r'''
#include "lzs.h"
#include "lzs_channels.h"
#include <stdio.h>
int main(void) {
    size_t (*w)(size_t, size_t, size_t) = lzs_channels_burst_split_work_bytes;
    printf("%d %d\n", w != 0, w(100, 10, 1500) >= lzs_channels_burst_work_bytes(100, 10) + 2u * 100u * 1500u);
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


def test_header_compiles_as_c99_and_cxx_with_the_split_size(tmp_path):
    assert _build_and_run(tmp_path, "gcc", "c99", ".c") == ["1", "1"]
    assert _build_and_run(tmp_path, "g++", "c++17", ".cc") == ["1", "1"]


def test_the_split_size_is_exported_and_in_the_package():
    assert hasattr(lzs.lib(), "lzs_channels_burst_split_work_bytes")
    assert "channels_burst_split_work_bytes" in lzs.__all__
    assert lzs.channels_burst_split_work_bytes(100, 10, 1500) == lzs.api.channels_burst_split_work_bytes(100, 10, 1500)


SIZES = list(range(0, 300)) + [1000, 4096, 65536, 65537, 1 << 20, 0x7FFFFFFF]
CAPS = (0, 1, 1500, 65536)


def test_split_size_is_monotone_and_never_below_the_burst_size():
    for nch in (1, 16384):
        for cap in CAPS:
            prev = 0
            for n in SIZES:
                w = lzs.channels_burst_split_work_bytes(n, nch, cap)
                assert w >= lzs.channels_burst_work_bytes(n, nch) and w >= 2 * n * cap and w >= prev, (n, nch, cap, w, prev)
                prev = w
        for n in SIZES:
            prev = 0
            for cap in CAPS + (1 << 20, (1 << 32) - 1, 1 << 40):
                w = lzs.channels_burst_split_work_bytes(n, nch, cap)
                assert w >= prev, (n, nch, cap, w, prev)
                prev = w
    for n in SIZES:
        for cap in CAPS:
            assert lzs.channels_burst_split_work_bytes(n, 16384, cap) >= lzs.channels_burst_split_work_bytes(n, 1, cap)
    assert lzs.channels_burst_split_work_bytes((1 << 31) - 1, 1, (1 << 32) - 1) == SIZE_MAX
    assert lzs.channels_burst_split_work_bytes(1 << 40, 1, 1 << 40) == SIZE_MAX       # (both clipped to their limits first)


WORK = 0x100000


def _call(name, states=0x2000, out_len=0x3000, in_len=0x4000, channel=0x5000, nchannels=8, work=WORK, work_bytes=None,
          npackets=4):
    A = lzs.api
    fake = ctypes.c_void_p(0x1000)
    if work_bytes is None:
        work_bytes = lzs.channels_burst_split_work_bytes(npackets, nchannels, 100)
    return getattr(A.lib(), name)(fake, 128, 100, out_len and ctypes.c_void_p(out_len), fake, 128,
                                  in_len and ctypes.c_void_p(in_len), 64, channel and ctypes.c_void_p(channel),
                                  states and ctypes.c_void_p(states), nchannels, None, work and ctypes.c_void_p(work), work_bytes,
                                  npackets, None)


def test_argument_errors_are_refused_with_a_split_work_area():
    A = lzs.api
    assert lzs.channels_burst_split_work_bytes(4, 8, 100) > lzs.channels_burst_work_bytes(4, 8)
    for kw, words in ((dict(channel=0), "channel is NULL"), (dict(states=0), "states is NULL"),
                      (dict(out_len=0), "out_len is NULL"), (dict(work=0), "work is NULL"),
                      (dict(work_bytes=lzs.channels_burst_work_bytes(4, 8) - 1), "smaller than"),
                      (dict(states=0x2002), "aligned"), (dict(work=WORK + 16), "aligned"),
                      (dict(out_len=0x3000, in_len=0x3000), "same array"), (dict(nchannels=0), "no channels"),
                      (dict(npackets=0x80000000, work_bytes=1 << 62), "too many packets")):
        rc = _call(DECODE, **kw)
        assert rc == A.LZS_E_ARG and words in A.last_error(), (kw, rc, A.last_error())
    assert _call(DECODE, npackets=0, channel=0, work=0) == A.LZS_OK       # nothing to do: no device needed


@pytest.mark.parametrize("name", [DECODE, "lzs_compress_channels_burst_device"])
def test_a_valid_call_with_a_split_work_area_without_a_device_says_so(name):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    A = lzs.api
    for work_bytes in (None, lzs.channels_burst_split_work_bytes(4, 8, 100) - 1, SIZE_MAX):
        rc = _call(name, work_bytes=work_bytes)
        assert rc == A.LZS_E_NO_DEVICE and "no HIP device" in A.last_error(), (rc, A.last_error())


def test_make_install_ships_the_split_size(tmp_path):
    prefix = tmp_path / "prefix"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lzs_compression_amd", "csrc"), "install", f"PREFIX={prefix}"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    installed = prefix / "include" / "lzs" / "lzs_channels.h"
    assert installed.exists() and installed.read_bytes() == open(HEADER, "rb").read()
    assert b"lzs_channels_burst_split_work_bytes" in installed.read_bytes()
    lib = ctypes.CDLL(str(prefix / "lib" / "liblzs.so.4"))
    assert hasattr(lib, "lzs_channels_burst_split_work_bytes")
