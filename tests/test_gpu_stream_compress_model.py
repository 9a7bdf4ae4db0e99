"""The segmented stream compressor -- lzs_compress_segments_kernel, lzs_stitch_segments_kernel, lzs_extend_resume_kernel, the entry
rounds, prefix sum and second pass in stream_compress_piece() (csrc/lzs_stream.c), DESIGN.md 3.5 -- on the directed inputs of
tests/stream_compress_programs.py, with the segment size forced to 256 and to 512 bytes: every route that ends in those kernels
must give what the oracle's one-shot compressor gives, in length and bytes.  What the inputs reach is proven on the CPU, by the
model's counters, in tests/test_stream_compress_model.py; nothing here is a sample.
"""
import functools
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle
import lzs_compression_amd as lzs
from lzs_compression_amd import api
import stream_compress_programs as P
from test_stream_compress_model import LONG_PIECE, SHORT_PIECE, feed

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
O = oracle.oracle()
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F = {name: i for i, name in enumerate(oracle.COMPRESS_SEGMENT_FIELDS)}
SEGS = (256, 512)
CHILD_ENV = dict(PYTHONPATH=os.pathsep.join((ROOT, os.path.join(ROOT, "tests"))), LZS_FORCE_STREAM="1", LZS_ROUTE="device")


def inputs(*families):
    return [i for i in P.directed_inputs() if not families or i.family in families]


@functools.lru_cache(maxsize=None)
def _want(name):
    return O.compress(next(i for i in P.directed_inputs() if i.name == name).data)


def want(i):
    return _want(i.name)


@pytest.fixture
def device(monkeypatch):
    monkeypatch.setenv("LZS_ROUTE", "device")
    monkeypatch.setenv("LZS_FORCE_STREAM", "1")
    return monkeypatch


@pytest.fixture(params=SEGS)
def seg(request, device):
    device.setenv("LZS_STREAM_SEG", str(request.param))
    return request.param


def test_host_buffers(seg):
    """lzs_compress() from host buffers: every directed input whole, and on one input a family cut at the stream's length, one and
    two bytes less, and at the byte of a middle segment's first bit - 1, + 0, + 1: the oracle's prefix."""
    for i in inputs():
        got = lzs.compress(i.data)
        assert len(got) == len(want(i)) and got == want(i), i.name
    for family in "ABCDEFG":
        i = inputs(family)[0]
        total = len(want(i))
        _, rec, _ = O.compress_segments(i.data, seg)
        full = np.flatnonzero(rec[:, F["empty"]] == 0)
        middle = int(rec[full[len(full) // 2], F["bit_at"]]) // 8
        for cap in (total, total - 1, total - 2, middle - 1, middle, middle + 1):
            assert lzs.compress(i.data, cap) == want(i)[:cap], (i.name, cap)


def test_without_the_switch_at_the_routes_own_threshold(monkeypatch):
    """6144 and 6145 bytes without LZS_FORCE_STREAM: the last length one workgroup takes and the first that goes by segments."""
    monkeypatch.setenv("LZS_ROUTE", "device")
    for i in inputs("F"):
        if len(i.data) in (6144, 6145):
            assert lzs.compress(i.data) == want(i), i.name


def test_device_pointers_at_four_alignments(seg):
    """lzs_compress_stream_device() with the input at byte offsets 0, 1, 4 and 16 of a larger tensor (the kernel's 16-byte, 4-byte
    and byte loads) and the output a 4-aligned slice of exactly compressed_max(n) + 1024 bytes inside a buffer of 0xA5: the oracle's
    stream, zeros behind it to the end of the slice, and not one byte changed either side of it."""
    most = max(len(i.data) for i in inputs())
    src = torch.empty(most + 64, dtype=torch.uint8, device="cuda")
    for i in inputs():
        n, w = len(i.data), want(i)
        room = api.compressed_max(n) + 1024
        data = torch.from_numpy(np.frombuffer(i.data, dtype=np.uint8).copy())
        for at in (0, 1, 4, 16):
            x = src[at:at + n]
            x.copy_(data)
            buf = torch.full((room + 72,), 0xA5, dtype=torch.uint8, device="cuda")
            lead = 20 + 4 * (at % 3)
            out, got = lzs.compress_stream(x, out=buf[lead:lead + room])
            assert x.data_ptr() % 16 == at % 16 and out.data_ptr() % 4 == 0 and out.numel() == room
            host = buf.cpu().numpy()
            assert got == len(w) and host[lead:lead + got].tobytes() == w, (i.name, at)
            assert not host[lead + got:lead + room].any(), (i.name, at)
            assert (host[:lead] == 0xA5).all() and (host[lead + room:] == 0xA5).all(), (i.name, at)


def test_one_workgroup_is_a_second_implementation(device):
    """LZS_ONE_WORKGROUP=1: the unsegmented kernel, which knows no slots, rounds or stitch, gives the same bytes on every input."""
    device.setenv("LZS_ONE_WORKGROUP", "1")
    for i in inputs():
        assert lzs.compress(i.data) == want(i), i.name


def _digest(datas):
    h = hashlib.sha256()
    for d in datas:
        h.update(len(d).to_bytes(4, "little") + d)
    return h.hexdigest()


def test_chain_safe_form_in_a_process_of_its_own():
    """LZS_CHAIN_FALLBACK=1 (decided once per process): the order-independent CHAIN form of the segment kernel on the whole directed
    set, at both segment sizes; a digest of all streams against the oracle's."""
    code = (
        "import hashlib, lzs_compression_amd as lzs, stream_compress_programs as P\n"
        "h = hashlib.sha256()\n"
        "for i in P.directed_inputs():\n"
        "    s = lzs.compress(i.data)\n"
        "    h.update(len(s).to_bytes(4, 'little') + s)\n"
        "print(h.hexdigest())\n")
    expect = _digest([want(i) for i in inputs()])
    for size in SEGS:
        env = dict(os.environ, **CHILD_ENV, LZS_CHAIN_FALLBACK="1", LZS_STREAM_SEG=str(size))
        env.pop("LZS_ONE_WORKGROUP", None)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.strip() == expect, size


def test_rounds_are_the_models():
    """The entry rounds of the family-C inputs, read from the LZS_STREAM_DEBUG lines of a process of its own, in 256-byte segments:
    as many "round N compressed" lines as the model has rounds, and the same number to redo after each -- the host's rule is
    deterministic (csrc/lzs_stream.c), and lzs_oracle_compress_segments simulates it on its own walks.  No time is asserted."""
    code = (
        "import sys, hashlib, lzs_compression_amd as lzs, stream_compress_programs as P\n"
        "by_name = {i.name: i for i in P.directed_inputs()}\n"
        "for name in sys.argv[1:]:\n"
        "    sys.stderr.write('== ' + name + '\\n'); sys.stderr.flush()\n"
        "    print(hashlib.sha256(lzs.compress(by_name[name].data)).hexdigest())\n")
    group = inputs("C")
    env = dict(os.environ, **CHILD_ENV, LZS_STREAM_DEBUG="1", LZS_STREAM_SEG="256")
    env.pop("LZS_ONE_WORKGROUP", None)
    r = subprocess.run([sys.executable, "-c", code, *(i.name for i in group)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [hashlib.sha256(want(i)).hexdigest() for i in group]
    parts = {part.split("\n", 1)[0]: part for part in r.stderr.split("== ")[1:]}
    for i in group:
        redo = [int(v) for v in re.findall(r"round \d+ compressed \d+ segments in [0-9.]+ ms; (\d+) to redo", parts[i.name])]
        _, _, rounds = O.compress_segments(i.data, 256)
        print(i.name, redo)
        assert redo == rounds, (i.name, redo, rounds)


@functools.lru_cache(maxsize=None)
def _cuts(name, least):
    i = next(i for i in P.directed_inputs() if i.name == name)
    return P.piece_cuts(O.compress_segments(i.data, 256, trace=True)[3], len(i.data), least)


@pytest.mark.parametrize("name, least, simple", [("G-short-pieces", SHORT_PIECE, True), ("G-long-pieces", LONG_PIECE, False)])
def test_pieces_of_the_incremental_interface(seg, name, least, simple):
    """lzs_compress_incremental() fed at the family-G cuts -- inside a long match at every residue of its nibbles, at every bit of
    the output byte, with a match open across three pieces, 1 .. 15 bytes past a decided token: short pieces through the low-memory
    block (every call with 16 bytes and more to decide reaches the device), long ones through the full block (it collects 10 KiB
    before it asks).  The one-shot oracle's stream; and once more in one call with the end marker in an empty call of its own."""
    i = next(i for i in inputs("G") if i.name == name)
    for label, at in _cuts(name, least).items():
        assert feed(i.data, at, simple) == want(i), (name, label, at)
    assert feed(i.data, [], simple, marker_separately=True) == want(i), name
    assert feed(i.data, [len(i.data) // 2], simple, marker_separately=True) == want(i), name
