"""lzs_compress_batch_device_sync() without a GPU: csrc/lzs_batch_compress.c and the product's unchanged host
sources over the CPU shim, with the two batch launchers stated on the CPU from their contracts
(tests/cpu_shim/batch_compress/launchers_host.c, on the oracle's match finder), as one stand-alone program under the address and
undefined-behaviour sanitizers.  Nothing is preloaded into anything.

The directed inputs of tests/stream_compress_programs.py as ONE ragged batch, in segments of 256 and of 512 bytes, at a capacity
that holds every stream and at two that cut them: every block's length and bytes are lzs_oracle_compress()'s at that capacity, no
byte outside the slots changes, and the "to redo" counts of the entry rounds are the element-wise sums over the blocks of the
rounds lzs_oracle_compress_segments simulates per block.  And each route forced."""
import os
import re
import struct
import subprocess

import pytest

import oracle
import stream_compress_programs as P

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HERE = os.path.join(ROOT, "tests", "cpu_shim", "batch_compress")
O = oracle.oracle()
CAPS = (0, 777, 150)              # 0: the driver takes the longest stream's length; the other two cut most of the 194 streams


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = tmp_path_factory.mktemp("batch_compress")
    r = subprocess.run(["make", "-C", HERE, f"OUT={out}", "-j8", str(out / "batch_compress_driver")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return out / "batch_compress_driver"


@pytest.fixture(scope="module")
def blob(tmp_path_factory):
    datas = [i.data for i in P.directed_inputs()]
    assert len(datas) == 194
    path = tmp_path_factory.mktemp("batch_compress_blob") / "batch.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(datas)))
        f.write(struct.pack(f"<{len(datas)}I", *(len(d) for d in datas)))
        for d in datas:
            f.write(d)
    return path


def _run(driver, blob, **switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LZS_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", LZS_STREAM_DEBUG="1", **switches)
    r = subprocess.run([str(driver), str(blob), *(str(c) for c in CAPS)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and f"ok {2 * len(CAPS)} calls" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    return r.stderr


def _model_rounds(seg):
    expect = []
    for i in P.directed_inputs():
        rounds = [int(v) for v in O.compress_segments(i.data, seg)[2]]
        expect += [0] * (len(rounds) - len(expect))
        for k, v in enumerate(rounds):
            expect[k] += v
    return expect


@pytest.mark.parametrize("seg", (256, 512))
def test_the_directed_batch_by_segments(driver, blob, seg):
    log = _run(driver, blob, LZS_STREAM_SEG=str(seg), LZS_BATCH_COMPRESS_ROUTE="2")
    calls = log.split("== ")[1:]
    assert len(calls) == 2 * len(CAPS) + 1
    expect = _model_rounds(seg)
    for call in calls[:-1]:
        redo = [int(v) for v in re.findall(r"round \d+ compressed \d+ segments in [0-9.]+ ms; (\d+) to redo", call)]
        assert redo == expect, (seg, call.split("\n", 1)[0], redo, expect)
    launches = [int(v) for v in re.search(r"launches: (\d+) compress \((\d+) second passes\), (\d+) stitch", calls[-1]).groups()]
    assert launches[2] == 2 * len(CAPS) and launches[1] == 2 * len(CAPS)        # (family E has segments that do not fit their slots)
    assert launches[0] == 2 * len(CAPS) * (len(expect) + 1)


def test_by_the_rule_and_by_workgroups(driver, blob):
    """The directed batch has no block of the rule's length: unforced it goes by workgroups, like forced to 1 -- no round at all."""
    for switches in ({}, {"LZS_BATCH_COMPRESS_ROUTE": "1"}):
        log = _run(driver, blob, **switches)
        assert "to redo" not in log and "launches: 0 compress (0 second passes), 0 stitch" in log
