"""The size query's kernel without a GPU: csrc/lzs_decoded_size.hip compiles as host C++ against a stub of the HIP names
(tests/cpu_shim/size_walk) and runs under the address and undefined-behaviour sanitizers, every stream in an allocation that
ends with the aligned word holding its last byte.  Its sizes are those of the CPU oracle's decoder at that capacity, its sizes
and statuses those of a bit-by-bit restatement of the decoders' rules (lzs_burst_parse_kernel's walk), on compressed blocks
of the three classes, whole and cut, on random bytes, on every cut of a short stream, at several limits and alignments."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import oracle
import lzs_compression_amd as lzs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
WALK = os.path.join(ROOT, "tests", "cpu_shim", "size_walk")
CSRC = os.path.join(ROOT, "lzs_compression_amd", "csrc")
NONE = 0xFFFFFFFF
O = oracle.oracle()


def model(data, limit):
    """The decoders' rules, a token at a time: (length, status)."""
    bits = "".join(f"{b:08b}" for b in data)
    p = count = 0
    ext = cut = eos = False
    while True:
        have = len(bits) - p
        top = int((bits[p:p + 32] + "0" * 32)[:32], 2)
        room = limit - count
        if ext:
            e = top >> 28
            if not cut and e == 0 and have >= 13 and ((top >> 19) & 0x1FF) == 0x180:
                eos = True
            if have < 4 or room == 0:
                break
            need, ncopy, ext = 4, e, e == 15
        elif top >> 31 == 0:
            if have < 9 or room == 0:
                break
            need, ncopy = 9, 1
        else:
            shrt = (top >> 30) & 1
            used = 9 if shrt else 13
            o = (top >> 23) & 0x7F if shrt else (top >> 19) & 0x7FF
            if o == 0 and shrt:
                eos = eos or (have >= 9 and not cut)
                break
            if o == 0:
                if have < 13 or room == 0:
                    break
                need, ncopy = 13, 0
            else:
                code = ((top << used) & 0xFFFFFFFF) >> 28
                need = used + (2 if code < 12 else 4)
                if have < need or room == 0:
                    break
                ncopy = (code >> 2) + 2 if code < 12 else code - 7
                ext = ncopy == 8
        p += need
        m = min(ncopy, room)
        cut = cut or m < ncopy
        count += m
    return count, (4 if eos else (8 if count >= limit else 3))


def _cases():
    rng = random.Random(5)
    cases = []

    def add(data, limits):
        for limit in limits:
            cases.append((bytes(data), rng.randrange(20), limit))

    for cls in ("text", "lowent", "random"):
        blk = lzs.workload.fill(cls, 8, 9000)
        for b in range(8):
            raw = blk[b, :rng.randrange(0, 9001)].tobytes()
            c = O.compress(raw)
            S = len(raw)
            add(c, [NONE, S, max(S - 1, 0), S // 2, 1, 0, 100])
            add(c[:rng.randrange(0, len(c) + 1)], [NONE, 100, 4096])
    add(O.compress(bytes(1000)), [NONE, 1000, 999, 500, 16, 15, 1, 0])
    add(O.compress(b"x" * 24), [NONE, 24, 23])
    add(O.compress(b"ab" * 700 + bytes(range(256)) * 3), [NONE, 2168, 2167, 1399, 1400, 1401, 3])
    for _ in range(600):
        add(bytes(rng.randrange(256) for _ in range(rng.randrange(0, 301))), [NONE, 100, rng.randrange(0, 50)])
    short = O.compress(bytes(range(65, 95)) + b"ABCDEFGHIJ" + bytes(range(95, 100)))
    for k in range(len(short) + 1):
        add(short[:k], [NONE, 7])
    add(b"\xC0\x00" + b"\x55" * 40, [NONE, 0])
    add(b"\xFF" * 3000, [NONE, 1000, 37])
    return cases


def test_the_kernel_source_on_the_host_under_sanitizers(tmp_path):
    exe = tmp_path / "size_walk"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-x", "c++",
                        f"-I{WALK}", f"-I{CSRC}", os.path.join(WALK, "driver.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    cases = _cases()
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for data, offset, limit in cases:
            f.write(struct.pack("<III", len(data), offset, limit) + data)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LZS_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and f"ok {len(cases)} cases" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint32).reshape(-1, 2)
    assert len(got) == len(cases)
    for i, (data, offset, limit) in enumerate(cases):
        want = model(data, limit)
        assert (int(got[i, 0]), int(got[i, 1])) == want, (i, len(data), offset, limit, got[i].tolist(), want, data[:16].hex())
        if want[0] < 100000:                                # (the oracle's decoder needs a buffer of the capacity)
            assert len(O.decompress(data, min(limit, 100000))) == want[0], (i, len(data), limit, want)


def test_the_model_knows_the_rules():
    """The restatement itself, against streams whose answers are known."""
    assert model(b"", NONE) == (0, 3) and model(b"\xC0\x00", NONE) == (0, 4) and model(b"\xC0\x00", 0) == (0, 4)
    assert model(b"\x20", NONE) == (0, 3)
    c = O.compress(b"x" * 100)
    assert model(c, NONE) == (100, 4) and model(c, 100) == (100, 4) and model(c, 99) == (99, 8) and model(c[:-2], NONE)[1] == 3
    c = O.compress(bytes(range(200)))
    assert model(c, 200) == (200, 4) and model(c, 199) == (199, 8)
