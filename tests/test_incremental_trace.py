"""What every call of the incremental interface does, held against a record (tests/golden/inc_call_traces.json).

The other incremental tests compare the bytes of a whole stream.  A change to lzs_incremental.c can leave those alone and
still alter how much a call consumes, which flags it reports or what it leaves in the caller's parameter block.  So here a
scenario is a *call trace*: for every call one line -- bytes produced, how far both lengths and both pointers moved, and
the caller's block from offset 32 to its end (the status byte and reserved_: every private byte, "dead" ones included;
the pointers and lengths in front are left out as values because addresses differ) -- and a scenario's digest is the
SHA-256 over its lines.  The record was made by tests/golden/make_inc_call_traces.py from a build of the commit BEFORE the
stages of lzs_incremental.c became functions (LZS_LIBRARY), never from the code under test: the `host` section anywhere,
the `device` section on the MI355X.

This module holds the scenarios and replays the `host` section (LZS_ROUTE=host: the calling thread's own codec, no device
needed); tests/test_gpu_incremental_trace.py replays the `device` section."""
import ctypes
import functools
import hashlib
import random
import struct

import numpy as np
import pytest

from conftest import golden_json
import lzs_compression_amd as lzs
from lzs_compression_amd import api, workload

ERROR, END_MARKER, STARVED = api.STATUS_ERROR, api.STATUS_END_MARKER, api.STATUS_INPUT_STARVED
MIB = 1 << 20


@functools.lru_cache(maxsize=None)
def sample(kind, n, first_block):
    blocks = workload.fill(workload.CLASS_NAMES.index(kind), (n + 65535) // 65536, 65536, first_block=first_block, seed=workload.DEFAULT_SEED)
    return np.asarray(blocks).tobytes()[:n]


@functools.lru_cache(maxsize=None)
def three_streams():
    """Three streams back to back, each with its end marker: text; 60 000 zeros, then text; random bytes."""
    t = sample("text", 60000, 70)
    plains = [t[:40000], bytes(60000) + t[40000:], sample("random", 30000, 71)]
    return b"".join(plains), b"".join(lzs.compress(x) for x in plains)


@functools.lru_cache(maxsize=None)
def long_stream():
    """About 3 MiB of compressed text: the smallest at which pieces of 1.5 - 3 MiB double the pass size of the many-wavefront
    path twice from 1 MiB."""
    plain = sample("text", 5600000, 80)
    return plain, lzs.compress(plain)


class Trace:
    def __init__(self, block):
        self.block, self.sha, self.calls, self.bytes = block, hashlib.sha256(), 0, 0

    def call(self, fn, *extra):
        p = self.block
        before = (p.inLength, p.outLength, p.inPtr or 0, p.outPtr or 0)
        made = fn(ctypes.addressof(p), *extra)
        after = (p.inLength, p.outLength, p.inPtr or 0, p.outPtr or 0)
        self.sha.update(struct.pack("<5Q", made, before[0] - after[0], before[1] - after[1], after[2] - before[2], after[3] - before[3]))
        self.sha.update(bytes(p)[32:])
        self.calls += 1
        self.bytes += made
        return made

    def result(self):
        return {"calls": self.calls, "bytes": self.bytes, "digest": self.sha.hexdigest()}


def _buffer(data):
    return ctypes.create_string_buffer(bytes(data), max(len(data), 1))


def compress_trace(data, seed, in_range, out_range, simple=False):
    """The reference tool's loop (utils/lzs-compress.c:91-134) with seeded piece sizes: unread input offered again,
    add_end_marker once the input is used up, until END_MARKER.  Returns the trace and the stream."""
    rng, L = random.Random(seed), lzs.lib()
    p = api.SimpleCompressParameters() if simple else api.CompressParameters()
    (L.lzs_simple_compress_init if simple else L.lzs_compress_init_full)(ctypes.addressof(p))
    fn = L.lzs_simple_compress_incremental if simple else L.lzs_compress_incremental
    src, dst = _buffer(data), ctypes.create_string_buffer(lzs.compressed_max(len(data)) + 64)
    tr, pos, at, pending, made, finish = Trace(p), 0, 0, 0, 0, False
    while not (p.status & END_MARKER):
        if not pending and not finish:
            at, pending = pos, min(rng.randint(*in_range), len(data) - pos)
            pos += pending
            finish = pending == 0
        room = min(rng.randint(*out_range), len(dst) - made)
        p.inPtr, p.inLength, p.outPtr, p.outLength = ctypes.addressof(src) + at, pending, ctypes.addressof(dst) + made, room
        made += tr.call(fn, finish)
        at, pending = at + pending - p.inLength, p.inLength
        assert not (p.status & ERROR), lzs.last_error()
        assert tr.calls < 200000, "no progress"
    return tr, dst.raw[:made]


def decompress_trace(stream, seed, in_range, out_range, room_for, tr=None):
    """The loop of test-lzs-decompression.c with seeded piece sizes, through every end marker, until the input is used up
    and STARVED is reported.  Returns the trace and the output.  `tr`: a trace to go on with, on its block as it was left."""
    rng, L = random.Random(seed), lzs.lib()
    if tr is None:
        tr = Trace(api.DecompressParameters())
        L.lzs_decompress_init(ctypes.addressof(tr.block))
    p, src, dst = tr.block, _buffer(stream), ctypes.create_string_buffer(room_for + 64)
    pos, at, pending, made = 0, 0, 0, 0
    while True:
        if not pending and pos < len(stream):
            at, pending = pos, min(rng.randint(*in_range), len(stream) - pos)
            pos += pending
        room = min(rng.randint(*out_range), len(dst) - made)
        p.inPtr, p.inLength, p.outPtr, p.outLength = ctypes.addressof(src) + at, pending, ctypes.addressof(dst) + made, room
        made += tr.call(L.lzs_decompress_incremental)
        at, pending = at + pending - p.inLength, p.inLength
        assert not (p.status & ERROR), lzs.last_error()
        if not pending and pos >= len(stream) and (p.status & STARVED):
            break
        assert tr.calls < 200000, "no progress"
    return tr, dst.raw[:made]


def _full(in_range, out_range):
    """The full block on 90 000 bytes of text: compress, then decode the result with room up to three times the piece."""
    text = sample("text", 90000, 60)

    def compress():
        tr, stream = compress_trace(text, 101, in_range, out_range)
        assert stream == lzs.compress(text)
        return tr

    def decode():
        tr, out = decompress_trace(lzs.compress(text), 102, in_range, (out_range[0], 3 * out_range[1]), len(text))
        assert out == text
        return tr
    return compress, decode


def _simple():
    """The low-memory block, 1 - 12 bytes of room: the token-counted take, `stop`, the marker waiting behind parked output."""
    text = sample("text", 20000, 60)
    tr, stream = compress_trace(text, 103, (1, 300), (1, 12), simple=True)
    assert stream == lzs.compress(text)
    return tr


def _parked():
    """The full block with room smaller than the output: parked in the block, several calls draining it, marker_waiting."""
    low = sample("lowent", 200000, 61)
    tr, stream = compress_trace(low, 104, (30000, 60000), (1, 200))
    assert stream == lzs.compress(low)
    return tr


def _three(in_range, out_range):
    """Markers inside pieces, a copy still running at a piece border.  (The streams are short: the pass size stays as it was.)"""
    def run():
        plain, stream = three_streams()
        tr, out = decompress_trace(stream, 105, in_range, out_range, len(plain))
        assert out == plain
        return tr
    return run


def _long():
    """The pass size of the many-wavefront path going up, and remembered in the block."""
    plain, stream = long_stream()
    tr, out = decompress_trace(stream, 106, (3 * MIB // 2, 3 * MIB), (8 * MIB, 8 * MIB), len(plain))
    assert out == plain
    return tr


def _shrink():
    """The pass size going down again, on the block that learnt it: after the long stream, a buffer of the three short streams
    and then the long one, whole -- a grown pass meets an end marker in its first quarter, three times over -- and the long
    stream makes it grow once more."""
    plain, stream = long_stream()
    short_plain, short_stream = three_streams()
    tr, out = decompress_trace(stream, 107, (3 * MIB // 2, 3 * MIB), (8 * MIB, 8 * MIB), len(plain))
    assert out == plain
    tr, out = decompress_trace(short_stream + stream, 108, (16 * MIB, 16 * MIB), (8 * MIB, 8 * MIB), len(short_plain) + len(plain), tr)
    assert out == short_plain + plain
    return tr


def _fail_decode():
    """A good call, a NULL input pointer with a length, a call after that ERROR: status, the pointers at the end, the lengths zeroed."""
    stream, L = lzs.compress(sample("text", 90000, 60)), lzs.lib()
    p = api.DecompressParameters()
    L.lzs_decompress_init(ctypes.addressof(p))
    src, dst, tr = _buffer(stream), ctypes.create_string_buffer(600), Trace(p)
    for k, (ptr, n) in enumerate(((ctypes.addressof(src), 100), (None, 77), (ctypes.addressof(src) + 100, 100))):
        p.inPtr, p.inLength, p.outPtr, p.outLength = ptr, n, ctypes.addressof(dst), len(dst)
        tr.call(L.lzs_decompress_incremental)
        assert bool(p.status & ERROR) == (k == 1) and p.inLength == 0, (k, p.status)
    return tr


def _fail_not_initialised():
    """A full block whose reserved_ is 0xFF throughout: ERROR next to END_MARKER, the input dropped."""
    text, L = sample("text", 3000, 60), lzs.lib()
    p = api.CompressParameters()
    ctypes.memset(ctypes.addressof(p), 0xFF, ctypes.sizeof(p))
    src, dst, tr = _buffer(text), ctypes.create_string_buffer(600), Trace(p)
    p.inPtr, p.inLength, p.outPtr, p.outLength = ctypes.addressof(src), len(text), ctypes.addressof(dst), len(dst)
    assert tr.call(L.lzs_compress_incremental, False) == 0
    assert p.status == ERROR | END_MARKER | STARVED | api.STATUS_INPUT_FINISHED and p.inLength == 0 and p.inPtr == ctypes.addressof(src) + len(text)
    return tr


SCENARIOS = {}
for _in, _out in (((1, 60), (3, 60)), ((100, 5000), (100, 5000)), ((512, 512), (512, 512)), ((20000, 90000), (20000, 90000))):
    _c, _d = _full(_in, _out)
    SCENARIOS[f"full/compress {_in[0]}..{_in[1]}"], SCENARIOS[f"full/decode {_in[0]}..{_in[1]}"] = _c, _d
SCENARIOS.update({
    "simple/compress 1..300 into 1..12": _simple,
    "full/compress 30000..60000 into 1..200": _parked,
    "three/decode 16384 into 1 MiB": _three((16384, 16384), (MIB, MIB)),
    "three/decode 20000..90000 into 5000..400000": _three((20000, 90000), (5000, 400000)),
    "long/decode 1.5..3 MiB into 8 MiB": _long,
    "shrink/decode the long stream, then three short ones and the long one in one piece": _shrink,
    "fail/decode: NULL input, then a call after the ERROR": _fail_decode,
    "fail/compress: a block that was not initialised": _fail_not_initialised,
})


def replay(section, name):
    record = golden_json("inc_call_traces.json")
    assert section in record, f"tests/golden/inc_call_traces.json has no `{section}` section: it was never recorded"
    assert SCENARIOS[name]().result() == record[section][name]


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_every_call_on_the_host_route_does_what_was_recorded(monkeypatch, name):
    monkeypatch.setenv("LZS_ROUTE", "host")
    replay("host", name)
