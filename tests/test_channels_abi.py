"""CPU-side checks of the channel calls (include/lzs/lzs_channels.h): the header compiles from C99 and C++ beside lzs.h,
every function it declares is exported, the slot size agrees with the Python package, arguments are refused before the
device is asked, a valid call without a device says so, and `make install` ships the header."""
import ctypes
import os
import re
import subprocess

import pytest

import lzs_compression_amd as lzs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "lzs", "lzs_channels.h")
CALLS = ("lzs_compress_channels_device", "lzs_decompress_channels_device")

PROGRAM = r'''
#include "lzs.h"
#include "lzs_channels.h"
#include <stdio.h>
int main(void) {
    int (*c)(void *, size_t, size_t, uint32_t *, const void *, size_t, const uint32_t *, size_t, const uint32_t *, void *,
             uint8_t *, size_t, void *) = lzs_compress_channels_device;
    int (*d)(void *, size_t, size_t, uint32_t *, const void *, size_t, const uint32_t *, size_t, const uint32_t *, void *,
             uint8_t *, size_t, void *) = lzs_decompress_channels_device;
    printf("%u %u %u %d\n", (unsigned)LZS_CHANNEL_STATE_BYTES, (unsigned)LZS_CHANNEL_HISTORY_AT,
           (unsigned)LZS_COMPRESSED_MAX(1500u), (c != 0) && (d != 0));
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


def test_channels_header_compiles_as_c99_and_cxx_beside_lzs_h(tmp_path):
    want = ["2112", "64", str(lzs.compressed_max(1500)), "1"]
    assert _build_and_run(tmp_path, "gcc", "c99", ".c") == want
    assert _build_and_run(tmp_path, "g++", "c++17", ".cc") == want


def test_every_function_of_the_channels_header_is_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lzs_[a-z_]+)\s*\(", text))
    assert set(CALLS) <= declared
    lib = lzs.lib()
    for name in declared:
        assert hasattr(lib, name), name


def test_state_size_agrees_with_the_package():
    text = open(HEADER).read()
    m = re.search(r"#define\s+LZS_CHANNEL_STATE_BYTES\s+(\d+)u", text)
    assert m and int(m.group(1)) == lzs.CHANNEL_STATE_BYTES == lzs.api.CHANNEL_STATE_BYTES


def _call(name, states=0x2000, out_len=0x3000, in_len=0x4000, npackets=4, channel=None):
    A = lzs.api
    fake = ctypes.c_void_p(0x1000)
    return getattr(A.lib(), name)(fake, 128, 100, out_len and ctypes.c_void_p(out_len), fake, 128,
                                  in_len and ctypes.c_void_p(in_len), 64, channel, states and ctypes.c_void_p(states),
                                  None, npackets, None)


@pytest.mark.parametrize("name", CALLS)
def test_argument_errors_are_refused_before_the_device(name):
    A = lzs.api
    rc = _call(name, states=0)
    assert rc == A.LZS_E_ARG and "states is NULL" in A.last_error(), (rc, A.last_error())
    rc = _call(name, out_len=0x3000, in_len=0x3000)
    assert rc == A.LZS_E_ARG and "same array" in A.last_error(), (rc, A.last_error())
    rc = _call(name, npackets=0x80000000)
    assert rc == A.LZS_E_ARG and "too many packets" in A.last_error(), (rc, A.last_error())
    rc = _call(name, out_len=0)
    assert rc == A.LZS_E_ARG and "out_len is NULL" in A.last_error(), (rc, A.last_error())
    rc = _call(name, states=0x2002)
    assert rc == A.LZS_E_ARG and "aligned" in A.last_error(), (rc, A.last_error())
    assert _call(name, npackets=0) == A.LZS_OK            # nothing to do: no device needed


@pytest.mark.parametrize("name", CALLS)
def test_a_valid_call_without_a_device_says_so(name):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    A = lzs.api
    rc = _call(name, channel=ctypes.c_void_p(0x5000))
    assert rc == A.LZS_E_NO_DEVICE and "no HIP device" in A.last_error(), (rc, A.last_error())


def test_make_install_ships_the_channels_header(tmp_path):
    prefix = tmp_path / "prefix"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lzs_compression_amd", "csrc"), "install", f"PREFIX={prefix}"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    installed = prefix / "include" / "lzs" / "lzs_channels.h"
    assert installed.exists() and installed.read_bytes() == open(HEADER, "rb").read()
    assert (prefix / "include" / "lzs" / "lzs_batch.h").exists()
