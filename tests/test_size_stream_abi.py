"""The size query for long streams (include/lzs/lzs_batch.h) at the drop-in boundary, without a GPU: the three
prototypes compile from C99 and C++17, both libraries export them, the Python names are public, every argument error is refused
with the call's name before the device is asked, the calls that need no device return LZS_OK, and a valid call says
LZS_E_NO_DEVICE where there is none."""
import ctypes
import os
import subprocess

import pytest

import lzs_compression_amd as lzs
from lzs_compression_amd import api

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INC = os.path.join(ROOT, "include")
PKG = os.path.join(ROOT, "lzs_compression_amd")
NAMES = ("lzs_decompressed_size_stream_device", "lzs_decompressed_size_stream", "lzs_decompressed_size_batch_device_sync")
BLOCK_MAX = 3 << 30
MAX64 = (1 << 64) - 1

CALLER = r'''
#include "lzs.h"
#include "lzs_batch.h"
#include <stdio.h>
int main(void) {
    int (*a)(uint64_t *, uint8_t *, const void *, size_t, uint64_t, unsigned) = lzs_decompressed_size_stream_device;
    int (*b)(uint64_t *, uint8_t *, const uint8_t *, size_t, uint64_t, unsigned) = lzs_decompressed_size_stream;
    int (*c)(uint32_t *, uint8_t *, const void *, size_t, const uint32_t *, size_t, size_t, size_t) = lzs_decompressed_size_batch_device_sync;
    uint64_t size = 7; uint8_t status = 7;
    int rc = a(&size, &status, 0, 0, 5, 0) | b(&size, &status, 0, 0, 5, LZS_SIZE_CONCAT) | c(0, 0, 0, 0, 0, 0, 0, 0);
    printf("%d %u %u %u\n", rc, (unsigned)size, (unsigned)status, (unsigned)LZS_SIZE_CONCAT);
    return 0;
}
'''


@pytest.mark.parametrize("compiler, std, suffix", [("gcc", "-std=c99", ".c"), ("g++", "-std=c++17", ".cc")])
def test_the_prototypes_compile_and_link(tmp_path, compiler, std, suffix):
    src = tmp_path / ("t" + suffix)
    src.write_text(CALLER)
    exe = tmp_path / "t"
    subprocess.run([compiler, std, "-Wall", "-Werror", f"-I{INC}/lzs", str(src), f"-L{PKG}", "-llzs", f"-Wl,-rpath,{PKG}", "-o", str(exe)],
                   check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["0", "0", "3", "1"]


@pytest.mark.parametrize("so", ["liblzs.so", "liblzs_variants.so"])
def test_both_libraries_export_the_calls(so):
    dyn = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, so)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if " T " in line}
    assert set(NAMES) <= exported


def test_the_python_names_are_public():
    for name in ("decompressed_size", "decompressed_size_stream", "decompressed_sizes_sync", "SIZE_CONCAT"):
        assert name in lzs.__all__ and hasattr(lzs, name), name
    assert lzs.SIZE_CONCAT == 1


def _stream_calls():
    L = lzs.lib()
    return (("lzs_decompressed_size_stream_device", L.lzs_decompressed_size_stream_device),
            ("lzs_decompressed_size_stream", L.lzs_decompressed_size_stream))


def test_argument_errors_are_refused_before_the_device_is_asked():
    L = lzs.lib()
    size, status = ctypes.c_uint64(0), ctypes.c_uint8(0)
    buf = ctypes.create_string_buffer(b"\xC0\x00", 2)
    ps, pt, pb = ctypes.byref(size), ctypes.addressof(status), ctypes.addressof(buf)
    for name, fn in _stream_calls():
        for args, what in (((None, pt, pb, 2, MAX64, 0), "size is NULL"),
                           ((ps, pt, pb, 2, MAX64, 2), "unknown flags"),
                           ((ps, pt, pb, 2, MAX64, 0x80000001), "unknown flags"),
                           ((ps, pt, pb, BLOCK_MAX + 1, MAX64, 0), "exceeds LZS_BLOCK_MAX"),
                           ((ps, pt, None, 2, MAX64, 0), "input is NULL")):
            assert fn(*args) == api.LZS_E_ARG, (name, what)
            message = lzs.last_error()
            assert message.startswith(name + ":") and what in message, (name, what, message)
    name, fn = "lzs_decompressed_size_batch_device_sync", L.lzs_decompressed_size_batch_device_sync
    sizes, lens = (ctypes.c_uint32 * 2)(), (ctypes.c_uint32 * 2)(2, 2)
    for args, what in (((None, None, pb, 0, lens, 2, 100, 2), "size is NULL"),
                       ((sizes, None, pb, 0, None, BLOCK_MAX + 1, 100, 2), "exceeds LZS_BLOCK_MAX"),
                       ((sizes, None, pb, 0, lens, 2, 100, 0x80000000), "too many blocks"),
                       ((sizes, None, pb, 0, lens, 2, 1 << 32, 2), "exceeds 0xFFFFFFFF"),
                       ((sizes, None, None, 0, lens, 2, 100, 2), "input is NULL")):
        assert fn(*args) == api.LZS_E_ARG, what
        message = lzs.last_error()
        assert message.startswith(name + ":") and what in message, (what, message)


def test_calls_that_need_no_device():
    size, status = ctypes.c_uint64(9), ctypes.c_uint8(9)
    for name, fn in _stream_calls():
        for flags in (0, 1):
            size.value, status.value = 9, 9
            assert fn(ctypes.byref(size), ctypes.addressof(status), None, 0, 100, flags) == api.LZS_OK
            assert (size.value, status.value) == (0, 0x03), (name, flags)
            assert fn(ctypes.byref(size), None, None, 0, MAX64, flags) == api.LZS_OK and size.value == 0      # status may be NULL
            assert fn(ctypes.byref(size), ctypes.addressof(status), None, 0, 0, flags) == api.LZS_OK
            assert (size.value, status.value) == (0, 0x08), (name, flags)     # the lane query's answer for no bytes and no room
    assert lzs.lib().lzs_decompressed_size_batch_device_sync(None, None, None, 0, None, 0, 0, 0) == api.LZS_OK
    assert lzs.decompressed_size(b"") == (0, 3) and lzs.decompressed_size(b"", 0, concat=True) == (0, 8)


def test_a_valid_call_without_a_device_says_so():
    import torch
    size, status = ctypes.c_uint64(0), ctypes.c_uint8(0)
    buf = ctypes.create_string_buffer(b"\xC0\x00", 2)
    rc = lzs.lib().lzs_decompressed_size_stream(ctypes.byref(size), ctypes.addressof(status), ctypes.addressof(buf), 2, MAX64, 0)
    if torch.cuda.is_available():
        assert rc == api.LZS_OK and (size.value, status.value) == (0, 0x04)
        return
    assert rc == api.LZS_E_NO_DEVICE and "no HIP device" in lzs.last_error()
    sizes, lens = (ctypes.c_uint32 * 1)(), (ctypes.c_uint32 * 1)(2)
    assert lzs.lib().lzs_decompressed_size_batch_device_sync(sizes, None, ctypes.addressof(buf), 2, lens, 2, 100, 1) == api.LZS_E_NO_DEVICE
    with pytest.raises(lzs.LzsError) as e:
        lzs.decompress(b"\xC0\x00")
    assert e.value.code == api.LZS_E_NO_DEVICE
