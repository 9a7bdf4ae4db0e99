"""The size query for long streams without a GPU: csrc/lzs_size_stream.c and the product's unchanged host
sources over the CPU shim (tests/cpu_shim/lzs_cpu_shim.c restates SCAN serially), the finishing kernel compiled as host C++
(tests/cpu_shim/size_stream/kernels_host.cc), as one stand-alone program under the address and undefined-behaviour sanitizers.
Every stream lies in an allocation that ends with the aligned word holding its last byte.

Every directed stream of tests/stream_border_programs.py and every case of tests/test_decoded_size_host.py, in segments of 256 and
of 512 bytes: under the plain rule (size, status) is the bit-by-bit model's at the maximum, the true size and one below, 0, 1, and
a middle and the last reached segment's output start - 1, + 0, + 1 -- and the oracle decoder's length --, under the file rule the
model's total cut at the limit; all directed streams as the blocks of one batch, by segments and by lanes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import stream_border_programs as P
import size_stream_cases as C
from test_decoded_size_host import model, _cases

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HERE = os.path.join(ROOT, "tests", "cpu_shim", "size_stream")
O = C.O


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = tmp_path_factory.mktemp("size_stream")
    r = subprocess.run(["make", "-C", HERE, f"OUT={out}", "-j8", str(out / "size_stream_driver")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return out / "size_stream_driver"


def _run(driver, tmp_path, seg, records, nresults):
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("<I", len(records)))
        for r in records:
            f.write(r)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LZS_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", LZS_DEC_SEG=str(seg))
    r = subprocess.run([str(driver), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=900, env=env)
    assert r.returncode == 0 and f"ok {len(records)} cases" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint32).reshape(-1, 4 if nresults is None else 2)
    return got


def _stream(data, offset, limit, flags=0):
    return struct.pack("<IIIIQ", 0, len(data), offset, flags, limit) + data


@pytest.mark.parametrize("seg", C.SEGS)
def test_directed_streams_under_both_rules(driver, tmp_path, seg):
    records, wants = [], []
    for i, s in enumerate(P.directed_streams()):
        for limit in C.limits(s, seg):
            records.append(_stream(s.data, (i + limit) % 4, limit))
            wants.append((s.name, limit, 0, C.expected(s, limit)))
            if s.file_rule:
                records.append(_stream(s.data, (i + limit + 1) % 4, limit, 1))
                wants.append((s.name, limit, 1, C.expected_file_rule(s, seg, limit)))
    got = _run(driver, tmp_path, seg, records, None)
    assert len(got) == len(wants)
    for row, (name, limit, flags, want) in zip(got, wants):
        size = int(row[0]) | (int(row[1]) << 32)
        assert (size, int(row[2])) == want, (name, seg, limit, flags, size, int(row[2]), want)
        if flags == 0 and want[0] < 100000:                 # (the oracle's decoder needs a buffer of the capacity)
            assert len(O.decompress(C.by_name(name).data, min(limit, 100000))) == want[0], (name, limit)


@pytest.mark.parametrize("seg", C.SEGS)
def test_the_lane_query_s_cases(driver, tmp_path, seg):
    """Compressed blocks of the three classes whole and cut, random bytes, every cut of a short stream, 0xFF x 3000: most of
    them a segment or two, many shorter than a token."""
    cases = _cases()
    got = _run(driver, tmp_path, seg, [_stream(data, offset % 4, limit) for data, offset, limit in cases], None)
    assert len(got) == len(cases)
    for row, (data, offset, limit) in zip(got, cases):
        want = model(data, limit)
        assert (int(row[0]) | (int(row[1]) << 32), int(row[2])) == want, (len(data), offset, limit, row.tolist(), want, data[:16].hex())
        if want[0] < 100000:
            assert len(O.decompress(data, min(limit, 100000))) == want[0], (len(data), limit, want)


@pytest.mark.parametrize("seg", C.SEGS)
def test_all_streams_as_the_blocks_of_one_batch(driver, tmp_path, seg):
    """lzs_decompressed_size_batch_device_sync() by segments and by lanes (the driver holds the two routes to each other)."""
    datas = C.batch_blocks()
    arr, lens = C.rows(datas)
    stride = arr.shape[1]
    extent = max(b * stride + int(n) for b, n in enumerate(lens) if n)
    flat = arr.tobytes()[:extent]
    records = [struct.pack("<IIIIIQ", 1, len(datas), stride, k % 4, extent, limit) + lens.tobytes() + flat
               for k, limit in enumerate(C.BATCH_LIMITS)]
    got = _run(driver, tmp_path, seg, records, 2).reshape(len(C.BATCH_LIMITS), len(datas), 2)
    for k, limit in enumerate(C.BATCH_LIMITS):
        for b, data in enumerate(datas):
            assert tuple(int(v) for v in got[k, b]) == C.model_of(data, limit), (seg, limit, b, len(data))
