"""The many-wavefront stream decoders -- SCAN / DECODE / RESOLVE, csrc/kernels/decompress_stream.inc, the host rounds in
csrc/lzs_stream.c, DESIGN.md 3.6 -- on the directed streams of tests/stream_border_programs.py, with the segment size forced to 256
and to 512 bytes: every route that ends in those kernels must give what the oracle's one-shot decoder gives, in length and bytes, at
capacities that send a stream through each of the DECODE kernels.  What the streams reach is proven on the CPU, by the model's
counters, in tests/test_stream_border_model.py; nothing here is a sample.
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
import stream_border_programs as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
O = oracle.oracle()
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BIG = 1 << 22
F = {name: i for i, name in enumerate(oracle.SEGMENT_FIELDS)}
SEGS = (256, 512)


def streams(*families):
    return [s for s in P.directed_streams() if not families or s.family in families]


@functools.lru_cache(maxsize=None)
def _want(name, cap):
    return O.decompress(next(s for s in P.directed_streams() if s.name == name).data, cap)


def want(s, cap):
    return _want(s.name, cap)


def total_of(s):
    return len(want(s, BIG))


def band(produce, n):
    """Which DECODE kernel lzs_hip_launch_decode_stream picks for a stream of n bytes that produces ``produce`` (the host hands it
    min(total, capacity)): its own inequalities."""
    if produce > 6 * n:
        return "wave"                                                  # one wavefront a segment: lzs_decode_stream_kernel
    if 4 * n > produce and 10 * n < 9 * produce:
        return "two"                                                   # lzs_decode_stream_g8_kernel<TWO>
    if 10 * n >= 9 * produce:
        return "wide"                                                  # <WIDE>
    return "g8"                                                        # the plain one


def capacities(s):
    """One capacity in each of the launcher's four bands, and the exact output length."""
    n = len(s.data)
    caps = {"wide": 10 * n // 9, "two": 2 * n, "g8": 5 * n, "wave": 6 * n + 1}
    assert all(band(c, n) == b for b, c in caps.items())
    return sorted(set(caps.values()) | {max(total_of(s), 1)})


@pytest.fixture
def device(monkeypatch):
    monkeypatch.setenv("LZS_ROUTE", "device")
    monkeypatch.setenv("LZS_FORCE_STREAM", "1")
    return monkeypatch


@pytest.fixture(params=SEGS)
def seg(request, device):
    device.setenv("LZS_DEC_SEG", str(request.param))
    return request.param


def test_host_buffers_at_capacities_in_every_band(seg):
    """lzs_decompress() from host buffers: every directed stream at five capacities -- one in each band of the DECODE launcher, and
    the exact length -- and, on one stream a family, at a segment's output start - 1, + 0, + 1.  Between them the streams are decoded
    by all four non-CONCAT kernels."""
    ran = set()
    for s in streams():
        for cap in capacities(s):
            got = lzs.decompress(s.data, cap)
            assert len(got) == len(want(s, cap)) and got == want(s, cap), (s.name, cap)
            ran.add(band(min(cap, total_of(s)), len(s.data)))
    assert ran == {"wave", "two", "wide", "g8"}
    for family in "ABCDEF":
        s = streams(family)[0]
        _, rec = O.scan_segments(s.data, seg, BIG)
        reached = np.flatnonzero(rec[:, F["entry_bit"]] != oracle.SEGMENT_NEVER)
        for k in (int(reached[len(reached) // 2]), int(reached[-1])):
            for d in (-1, 0, 1):
                cap = int(rec[k, F["out_start"]]) + d
                assert lzs.decompress(s.data, cap) == want(s, cap), (s.name, k, d)


def test_device_pointers_at_every_alignment(seg):
    """lzs_decompress_stream_device() with the output at byte offsets 0, 1, 2, 3 of a larger tensor -- from 1 on RESOLVE goes without
    chunks and tails -- and the input at an odd offset: the oracle's bytes, and not one byte written either side of the slice."""
    most = max(len(s.data) for s in streams())
    src = torch.empty(most + 8, dtype=torch.uint8, device="cuda")
    for s in streams():
        n, total = len(s.data), total_of(s)
        x = src[1:1 + n]
        x.copy_(torch.from_numpy(np.frombuffer(s.data, dtype=np.uint8).copy()))
        caps = capacities(s)
        for at in range(4):
            cap = caps[at] if at % 2 else total + 5                    # (two capacities that cut it, too)
            buf = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            out, got = lzs.decompress_stream(x, cap, out=buf[16 + at:16 + at + cap])
            assert out.data_ptr() % 4 == at
            host = buf.cpu().numpy()
            assert got == len(want(s, cap)) and host[16 + at:16 + at + got].tobytes() == want(s, cap), (s.name, at, cap)
            assert (host[:16 + at] == 0xA5).all() and (host[16 + at + got:] == 0xA5).all(), (s.name, at, cap)


@functools.lru_cache(maxsize=None)
def _one_wave_concat(name, cap):
    s = next(s for s in P.directed_streams() if s.name == name)
    os.environ["LZS_ONE_WAVE"] = "1"
    try:
        return lzs.decompress_concat(s.data, cap)
    finally:
        del os.environ["LZS_ONE_WAVE"]


def test_file_rule_against_one_wavefront(seg):
    """lzs_decompress_concat() -- the file rule: on behind every end marker, from the next byte, history kept -- by many wavefronts
    gives what the one wavefront gives (LZS_ONE_WAVE=1), at the capacities of every band (here they pick the CONCAT kernels); the
    length is the model's under that rule, and where a stream has no marker but a last one the bytes are the oracle's."""
    ran = set()
    for s in streams():
        if not s.file_rule:
            continue
        total, _, steps = O.scan_segments(s.data, seg, BIG, file_rule=True, trace=True)
        markers = np.flatnonzero(steps[:, 1] == oracle.STEP_KINDS.index("marker"))
        n = len(s.data)
        caps = sorted({10 * n // 9, 2 * n, 5 * n, 6 * n + 1, max(total, 1)})
        if s.family == "F" and "-phase-" in s.name:
            caps = caps[-1:]                                           # (many and short: the exact length will do)
        for cap in caps:
            got = lzs.decompress_concat(s.data, cap)
            assert len(got) == min(total, cap), (s.name, cap)
            assert got == _one_wave_concat(s.name, cap), (s.name, cap)
            if len(markers) == 0 or markers[0] == len(steps) - 1:
                assert got == want(s, cap), (s.name, cap)
            ran.add(band(min(cap, total), n))
    assert ran == {"wave", "two", "wide", "g8"}


def _rows(datas):
    stride = (max(len(d) for d in datas) + 63) // 64 * 64
    arr = np.zeros((len(datas), stride), dtype=np.uint8)
    for i, d in enumerate(datas):
        arr[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    return arr, np.array([len(d) for d in datas], dtype=np.uint32)


def test_all_streams_as_the_blocks_of_one_batch(seg):
    """The batch-by-segments route: all directed streams as the blocks of one lzs_decompress_batch() call and of one
    lzs_decompress_batch_device_sync() call, at a capacity that holds most of them whole and at two that cut them all."""
    all_streams = streams()
    arr, lens = _rows([s.data for s in all_streams])
    x = torch.from_numpy(arr).cuda()
    for cap in (300_000, 20_001, 999):
        # (the route: under 4096 blocks, at most 64 MiB of output slots, 1 KiB a block and more -- host_batch_route, csrc/lzs_host.c)
        assert len(all_streams) * cap <= 64 << 20 and int(lens.sum()) // len(lens) >= 1024
        out, out_len = lzs.decompress_batch(arr, lens, cap)
        dev, dev_len = lzs.decompress_blocks_sync(x, lens, cap)
        dev = dev.cpu().numpy()
        for i, s in enumerate(all_streams):
            w = want(s, cap)
            assert out_len[i] == len(w) and out[i, :len(w)].tobytes() == w, (s.name, cap, "host buffers")
            assert dev_len[i] == len(w) and dev[i, :len(w)].tobytes() == w, (s.name, cap, "device buffers")


def _feed(pieces, room):
    d = lzs.IncrementalDecompressor()
    out, first, calls = bytearray(), None, 0
    for piece in pieces:
        pending = piece
        while pending:
            got, used, status = d.step(pending, room)
            assert not (status & lzs.STATUS_ERROR)
            out += got
            pending = pending[used:]
            if first is None and (status & api.STATUS_END_MARKER):
                first = len(out)
            calls += 1
            assert calls < 10000, "no progress"
    return bytes(out), first


def test_incremental_decoder_takes_over_inside_tokens_extensions_and_behind_markers(seg):
    """The incremental decoder on the device route, every long enough stream in two pieces, the second of 16 KiB and more with room
    for 1 MiB (it goes to many wavefronts: INC_DEC_STREAM_MIN, csrc/lzs_incremental.c), begun inside a token, inside an extension,
    and right behind an end marker and its pad bits.  It goes on behind markers with the history kept: all of its output is the one
    wavefront's under the file rule, and what it has at its first marker is the oracle's."""
    kinds = oracle.STEP_KINDS
    done = {"token": 0, "extension": 0, "marker": 0}
    for s in streams():
        n = len(s.data)
        if n < 16384 + 600:
            continue
        _, _, steps = O.scan_segments(s.data, seg, BIG, file_rule=True, trace=True)
        last = n - 16384                                               # the second piece begins here at the latest
        cuts = {}
        for i in range(len(steps) - 1):
            bit, kind = int(steps[i, 0]), kinds[int(steps[i, 1])]
            nxt = int(steps[i + 1, 0])
            byte = bit // 8 + 1                                         # the first byte boundary strictly inside the step, if any
            if byte > last:
                break
            if kind == "nib15" and kinds[int(steps[i + 1, 1])] == "nib15" and bit >= 8:
                cuts.setdefault("extension", (bit + 7) // 8)           # at or inside a nibble with another behind it
            if kind == "marker" and nxt % 8 == 0 and nxt // 8 <= last:
                cuts.setdefault("marker", nxt // 8)
            if 8 * byte < nxt and kind in ("short2", "long2", "short4", "long4", "lit", "long8"):
                cuts["token"] = byte                                   # (the last one in reach)
        whole = _one_wave_concat(s.name, BIG)
        for what, at in cuts.items():
            got, first = _feed((s.data[:at], s.data[at:]), 1 << 20)
            assert got == whole, (s.name, what, at)
            if first is not None:
                assert got[:first] == want(s, BIG), (s.name, what, at)
            done[what] += 1
    assert done["token"] >= 20 and done["extension"] >= 4 and done["marker"] >= 4, done


@pytest.mark.parametrize("switch", ["LZS_NO_MARKS", "LZS_NO_ONES", "LZS_NO_CHUNKS", "LZS_NO_TAILS"])
def test_shortcuts_are_shortcuts(seg, switch, device):
    """The streams of extensions, of phantom markers and walks that never merge, and of origins once more with one shortcut off: the
    merge marks of repeated walks, the all-0xFF segments the host works out itself, RESOLVE's chunks, its tails."""
    device.setenv(switch, "1")
    for s in streams("B", "C", "D"):
        cap = total_of(s) + 3
        assert lzs.decompress(s.data, cap) == want(s, cap), (s.name, switch)
        if s.file_rule and switch in ("LZS_NO_MARKS", "LZS_NO_ONES"):
            assert lzs.decompress_concat(s.data, cap) == _one_wave_concat(s.name, cap), (s.name, switch)


def test_rounds_arrive_where_a_full_walk_arrives():
    """LZS_VERIFY_SCAN=1 in a process of its own: after the rounds every segment is walked in full from its final entry, and a line
    on stderr says where that disagrees with what the rounds -- merged walks, noted end markers, the host's all-0xFF shortcut --
    arrived at.  No such line on the streams of families B, C and D, under either rule, and the oracle's bytes."""
    code = (
        "import hashlib, oracle, lzs_compression_amd as lzs, stream_border_programs as P\n"
        "h = hashlib.sha256()\n"
        "for s in P.directed_streams():\n"
        "    if s.family in 'BCD':\n"
        "        h.update(lzs.decompress(s.data, 1 << 22)); h.update(lzs.decompress_concat(s.data, 1 << 22))\n"
        "print(h.hexdigest())\n")
    h = hashlib.sha256()
    for s in streams("B", "C", "D"):
        h.update(want(s, BIG))
        h.update(_one_wave_concat(s.name, BIG))
    for size in SEGS:
        env = dict(os.environ, PYTHONPATH=os.pathsep.join((ROOT, os.path.join(ROOT, "tests"))), LZS_VERIFY_SCAN="1",
                   LZS_FORCE_STREAM="1", LZS_ROUTE="device", LZS_DEC_SEG=str(size))
        env.pop("LZS_ONE_WAVE", None)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "liblzs verify:" not in r.stderr, r.stderr[:2000]
        assert r.stdout.strip() == h.hexdigest(), size


def test_scan_rounds_where_reasoning_gives_their_number():
    """The SCAN rounds of two streams, counted from the LZS_STREAM_DEBUG lines of a process of its own, in 256-byte segments.
    (1) C-isolated-phantoms: every guessed walk falls in step inside its segment, and in every third segment it reads three end
    markers first.  Round 0 walks all segments from their guessed bit; every segment behind one without phantoms then has its true
    entry, and a segment behind one with phantoms keeps its guess -- the end its predecessor reports comes from a walk that was
    itself entered at a guess, and settle_entries() does not believe it.  Round 1 walks them from those entries, so now the segments
    with phantoms leave in their true state too; round 2 walks the segments behind them.  Three rounds; a rule that believed the
    phantom ends would need one per segment with phantoms, 22 here.
    (2) C-zeros-64-segments: a round settles at least the first segment that is not settled yet, so the rounds are at most the
    segments -- and here no guessed walk falls in step, so they are about that many (the cost DESIGN.md 3.6 records).  No time is
    asserted."""
    code = (
        "import sys, hashlib, lzs_compression_amd as lzs, stream_border_programs as P\n"
        "by_name = {s.name: s for s in P.directed_streams()}\n"
        "for name in sys.argv[1:]:\n"
        "    sys.stderr.write('== ' + name + '\\n'); sys.stderr.flush()\n"
        "    print(hashlib.sha256(lzs.decompress(by_name[name].data, 1 << 22)).hexdigest())\n")
    names = ("C-isolated-phantoms", "C-zeros-64-segments")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join((ROOT, os.path.join(ROOT, "tests"))), LZS_STREAM_DEBUG="1",
               LZS_FORCE_STREAM="1", LZS_ROUTE="device", LZS_DEC_SEG="256")
    r = subprocess.run([sys.executable, "-c", code, *names], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    by_name = {s.name: s for s in streams()}
    assert r.stdout.split() == [hashlib.sha256(want(by_name[n], BIG)).hexdigest() for n in names]
    parts = r.stderr.split("== ")[1:]
    rounds = {part.split("\n", 1)[0]: len(re.findall(r"round \d+ scanned", part)) for part in parts}
    print(rounds)
    assert 1 <= rounds["C-isolated-phantoms"] <= 3, rounds
    assert 1 <= rounds["C-zeros-64-segments"] <= 64, rounds
