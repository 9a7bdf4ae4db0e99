"""lzs_compress_batch_device_sync() (include/lzs/lzs_batch.h) at the drop-in boundary, without a GPU: the
prototype compiles from C99 and C++17, both libraries export it, the Python name is public, every argument error is refused with
the call's name before the device is asked, a batch of no blocks is LZS_OK and touches nothing, and a valid call says
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
NAME = "lzs_compress_batch_device_sync"
BLOCK_MAX = 3 << 30

CALLER = r'''
#include "lzs.h"
#include "lzs_batch.h"
#include <stdio.h>
int main(void) {
    int (*f)(void *, size_t, size_t, uint32_t *, const void *, size_t, const uint32_t *, size_t, size_t) = lzs_compress_batch_device_sync;
    uint32_t len = 7;
    int rc = f(0, 0, 0, &len, 0, 0, 0, 0, 0);
    int bad = f(0, 0, 0, 0, 0, 0, 0, 0, 1);
    printf("%d %u %d\n", rc, (unsigned)len, bad == LZS_E_ARG);
    return 0;
}
'''


@pytest.mark.parametrize("compiler, std, suffix", [("gcc", "-std=c99", ".c"), ("g++", "-std=c++17", ".cc")])
def test_the_prototype_compiles_and_links(tmp_path, compiler, std, suffix):
    src = tmp_path / ("t" + suffix)
    src.write_text(CALLER)
    exe = tmp_path / "t"
    subprocess.run([compiler, std, "-Wall", "-Werror", f"-I{INC}/lzs", str(src), f"-L{PKG}", "-llzs", f"-Wl,-rpath,{PKG}", "-o", str(exe)],
                   check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["0", "7", "1"]


@pytest.mark.parametrize("so", ["liblzs.so", "liblzs_variants.so"])
def test_both_libraries_export_the_call(so):
    dyn = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, so)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if " T " in line}
    assert NAME in exported


def test_the_python_name_is_public_and_bound():
    assert "compress_blocks_sync" in lzs.__all__ and hasattr(lzs, "compress_blocks_sync")
    fn = lzs.lib().lzs_compress_batch_device_sync
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(lzs.lib().lzs_decompress_batch_device_sync.argtypes)


def test_argument_errors_are_refused_before_the_device_is_asked():
    fn = lzs.lib().lzs_compress_batch_device_sync
    buf = ctypes.create_string_buffer(64)
    out = ctypes.create_string_buffer(64)
    pb, po = ctypes.addressof(buf), ctypes.addressof(out)
    lens, got = (ctypes.c_uint32 * 2)(2, 2), (ctypes.c_uint32 * 2)(9, 9)
    huge = (ctypes.c_uint32 * 2)(2, 0xC0000001)
    for args, what in (((po, 32, 32, None, pb, 32, lens, 2, 2), "out_len is NULL"),
                       ((po, 32, 32, got, None, 32, None, 2, 2), "input is NULL"),
                       ((po, 32, 32, got, None, 32, lens, 0, 2), "input is NULL"),
                       ((po, 32, 32, got, pb, 32, None, BLOCK_MAX + 1, 2), "exceeds LZS_BLOCK_MAX"),
                       ((po, 32, 32, got, pb, 32, huge, 2, 2), "exceeds LZS_BLOCK_MAX"),
                       ((po, 32, 32, got, pb, 32, lens, 2, 0x80000000), "too many blocks"),
                       ((None, 32, 32, got, pb, 32, lens, 2, 2), "output is NULL")):
        assert fn(*args) == api.LZS_E_ARG, what
        message = lzs.last_error()
        assert message.startswith(NAME + ":") and what in message, (what, message)
    assert list(got) == [9, 9] and out.raw == bytes(64)


def test_no_blocks_is_ok_and_touches_nothing():
    fn = lzs.lib().lzs_compress_batch_device_sync
    got = (ctypes.c_uint32 * 1)(9)
    assert fn(None, 0, 0, None, None, 0, None, 0, 0) == api.LZS_OK
    assert fn(None, 0, 100, got, None, 0, None, BLOCK_MAX + 1, 0) == api.LZS_OK and got[0] == 9


def test_a_valid_call_without_a_device_says_so():
    import torch
    if torch.cuda.is_available():
        return
    buf, out = ctypes.create_string_buffer(b"ab", 2), ctypes.create_string_buffer(16)
    lens, got = (ctypes.c_uint32 * 1)(2), (ctypes.c_uint32 * 1)(9)
    rc = lzs.lib().lzs_compress_batch_device_sync(ctypes.addressof(out), 16, 16, got, ctypes.addressof(buf), 2, lens, 2, 1)
    assert rc == api.LZS_E_NO_DEVICE and "no HIP device" in lzs.last_error()
