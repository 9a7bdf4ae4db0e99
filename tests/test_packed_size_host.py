"""The packed size query's kernel without a GPU: csrc/lzs_decoded_size.hip compiles as host C++ against the stub of the HIP
names (tests/cpu_shim/size_walk, by include path) with tests/cpu_shim/size_walk_packed/driver.cc and runs as a program of its own
under the address and undefined-behaviour sanitizers.  Every stream sits in an allocation that ends at the aligned word holding
its last byte, the offsets cover every residue mod 4 and come in shuffled order with d_in_len, and entries that are not blocks
sit among the others with their memory freed.  Sizes and statuses are those of the CPU oracle's decoder and of the model of the
decoders' rules (tests/test_decoded_size_host.py)."""
import os
import random
import struct
import subprocess

import numpy as np

import oracle
import lzs_compression_amd as lzs
from test_decoded_size_host import CSRC, NONE, WALK, model

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DRIVER = os.path.join(ROOT, "tests", "cpu_shim", "size_walk_packed", "driver.cc")
ERROR = 0x10
O = oracle.oracle()


def _batches():
    """[(limit, [(data, a0, kind)])]: kind 1 is no block with lengths (LZS_BLOCK_MAX + 1), kind 2 no block without (a decreasing pair)"""
    rng = random.Random(11)
    streams = []
    for cls in ("text", "lowent", "random"):
        blk = lzs.workload.fill(cls, 6, 9000)
        for b in range(6):
            c = O.compress(blk[b, :rng.randrange(0, 9001)].tobytes())
            streams += [c, c[:rng.randrange(0, len(c) + 1)]]
    streams += [O.compress(bytes(1000)), O.compress(b"x" * 24), b"", b"\xC0\x00", b"\x20", b"\xC0\x00" + b"\x55" * 40, b"\xFF" * 3000]
    streams += [bytes(rng.randrange(256) for _ in range(rng.randrange(0, 301))) for _ in range(200)]
    short = O.compress(bytes(range(65, 95)) + b"ABCDEFGHIJ" + bytes(range(95, 100)))
    streams += [short[:k] for k in range(len(short) + 1)]
    batches = []
    for limit in (NONE, 4096, 100, 37, 1, 0):
        pick = list(streams)
        rng.shuffle(pick)
        for nb in (1, 63, 64, 65, 129):
            entries = [(pick.pop(), rng.randrange(20), 0) for _ in range(min(nb, len(pick)))]
            if len(entries) > 8:
                for at, kind in ((2, 1), (5, 2), (len(entries) - 1, 1), (len(entries) - 2, 2)):
                    entries[at] = (entries[at][0], entries[at][1], kind)
            batches.append((limit, entries))
    seen = {(a0 % 4) for _, entries in batches for _, a0, _ in entries}
    assert seen == {0, 1, 2, 3}
    return batches


def test_the_packed_kernel_source_on_the_host_under_sanitizers(tmp_path):
    exe = tmp_path / "size_walk_packed"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-x", "c++",
                        f"-I{WALK}", f"-I{CSRC}", DRIVER, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    batches = _batches()
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("<I", len(batches)))
        for limit, entries in batches:
            f.write(struct.pack("<II", limit, len(entries)))
            for data, a0, kind in entries:
                f.write(struct.pack("<III", len(data), a0, kind) + data)
    total = sum(len(entries) for _, entries in batches)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LZS_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and f"ok {total} entries" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint32).reshape(-1, 4)
    assert len(got) == total
    i = 0
    for limit, entries in batches:
        for data, a0, kind in entries:
            want = model(data, limit)
            with_len = (0, ERROR) if kind == 1 else want
            without = (0, ERROR) if kind == 2 else want
            assert (int(got[i, 0]), int(got[i, 1])) == with_len, ("with lengths", i, len(data), a0, kind, limit, got[i].tolist(), want)
            assert (int(got[i, 2]), int(got[i, 3])) == without, ("without lengths", i, len(data), a0, kind, limit, got[i].tolist(), want)
            if want[0] < 100000:                            # (the oracle's decoder needs a buffer of the capacity)
                assert len(O.decompress(data, min(limit, 100000))) == want[0], (i, len(data), limit, want)
            i += 1
