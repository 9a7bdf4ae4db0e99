"""lzs_compress_batch_device_sync() -- a batch in device memory compressed by segments over all blocks at once
(csrc/lzs_batch_compress.c, lzs_compress_segments_batch_kernel, lzs_stitch_segments_batch_kernel) -- on the
directed inputs of tests/stream_compress_programs.py as ONE ragged batch, with the segment size forced to 256 and to 512 bytes.
A block of a batch is a stream of its own, so what the model's counters prove per input (tests/test_stream_compress_model.py)
holds per block; every block must be the oracle's one-shot stream, and what the workgroup-per-block kernel gives.
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

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
O = oracle.oracle()
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F = {name: i for i, name in enumerate(oracle.COMPRESS_SEGMENT_FIELDS)}
SEGS = (256, 512)
CHILD_ENV = dict(PYTHONPATH=os.pathsep.join((ROOT, os.path.join(ROOT, "tests"))), LZS_BATCH_COMPRESS_ROUTE="2")
PLAN = open(os.path.join(ROOT, "lzs_compression_amd", "csrc", "lzs_launch_plan.h")).read()
MIN_LONGEST = int(re.search(r"#define LZS_PLAN_BC_SEG_MIN_LONGEST (\d+)u", PLAN).group(1))


def inputs(*families):
    return [i for i in P.directed_inputs() if not families or i.family in families]


@functools.lru_cache(maxsize=None)
def _want(data):
    return O.compress(data)


def want(i):
    return _want(i.data)


def ragged(datas, stride=None, at=0, fill=0):
    """The datas as rows of one device tensor (row stride: the longest rounded up to 16, or `stride`), the first row `at` bytes
    into the allocation; (x, lengths)."""
    stride = stride or (max(len(d) for d in datas) + 15) // 16 * 16
    host = np.full(at + stride * len(datas) + 16, fill, dtype=np.uint8)
    for b, d in enumerate(datas):
        host[at + b * stride:at + b * stride + len(d)] = np.frombuffer(d, dtype=np.uint8)
    flat = torch.from_numpy(host).cuda()
    x = flat[at:at + stride * len(datas)].view(len(datas), stride)
    return x, np.array([len(d) for d in datas], dtype=np.uint32)


def check(out, lens, datas, cap=None, label=""):
    host = out.cpu().numpy()
    for b, d in enumerate(datas):
        w = _want(d) if cap is None else _want(d)[:cap]
        assert lens[b] == len(w) and host[b, :lens[b]].tobytes() == w, (label, b, len(d), int(lens[b]), len(w))


@pytest.fixture
def segments(monkeypatch):
    monkeypatch.setenv("LZS_BATCH_COMPRESS_ROUTE", "2")
    return monkeypatch


@pytest.fixture(params=SEGS)
def seg(request, segments):
    segments.setenv("LZS_STREAM_SEG", str(request.param))
    return request.param


def test_the_directed_set_as_one_ragged_batch(seg):
    """All directed inputs in one call: lengths and bytes are the oracle's, and those of the asynchronous compress_blocks() on the
    same tensor -- one workgroup a block, which knows no slots, rounds or stitch."""
    datas = [i.data for i in inputs()]
    x, n = ragged(datas)
    assert x.shape[1] == (max(len(d) for d in datas) + 15) // 16 * 16
    out, lens = lzs.compress_blocks_sync(x, n)
    check(out, lens, datas, label=seg)
    other, other_len = lzs.compress_blocks(x, torch.from_numpy(n.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    other, other_len, mine = other.cpu().numpy(), other_len.cpu().numpy(), out.cpu().numpy()
    assert (other_len == lens.astype(np.int64)).all()
    for b in range(len(datas)):
        assert mine[b, :lens[b]].tobytes() == other[b, :lens[b]].tobytes(), b


def test_cuts(seg):
    """One input of each family A-F with its two neighbours in the directed list, at the capacities of test_host_buffers for that
    input: its stream's length, one and two bytes less, the byte of a middle segment's first bit - 1, + 0, + 1.  The slots are as
    long as the capacity rounded up to 4, so neighbours touch; every block is the oracle's prefix."""
    everything = inputs()
    for family in "ABCDEF":
        i = inputs(family)[0]
        k = everything.index(i)
        datas = [j.data for j in everything[max(k - 1, 0):k + 2]]
        total = len(want(i))
        _, rec, _ = O.compress_segments(i.data, seg)
        full = np.flatnonzero(rec[:, F["empty"]] == 0)
        middle = int(rec[full[len(full) // 2], F["bit_at"]]) // 8
        x, n = ragged(datas)
        for cap in (total, total - 1, total - 2, middle - 1, middle, middle + 1):
            out, lens = lzs.compress_blocks_sync(x, n, out_capacity=cap)
            assert out.shape[1] == (cap + 3) // 4 * 4
            check(out, lens, datas, cap, (i.name, cap))


def test_containment_and_alignment(seg):
    """The output a 4-aligned slice inside a buffer of 0xA5, the input rows at byte offsets 0, 1, 4 and 16 of a larger tensor: the
    oracle's bytes in [0, out_len[b]) and not one byte changed outside the slots.  Then slots 24 bytes longer than the capacity:
    the last four bytes of every slot's gap stay 0xA5."""
    datas = [i.data for i in inputs("A", "E")] + [b"", b"x"]
    cap = max(len(_want(d)) for d in datas)
    for gap in (0, 24):
        stride = (cap + 3) // 4 * 4 + gap
        for at in (0, 1, 4, 16):
            x, n = ragged(datas, at=at)
            assert x.data_ptr() % 16 == at % 16
            lead = 20 + 4 * (at % 3)
            buf = torch.full((lead + stride * len(datas) + 52,), 0xA5, dtype=torch.uint8, device="cuda")
            out = buf[lead:lead + stride * len(datas)].view(len(datas), stride)
            assert out.data_ptr() % 4 == 0
            got, lens = lzs.compress_blocks_sync(x, n, out_capacity=cap, out=out)
            check(got, lens, datas, cap, (gap, at))
            host = buf.cpu().numpy()
            assert (host[:lead] == 0xA5).all() and (host[lead + stride * len(datas):] == 0xA5).all(), (gap, at)
            if gap:
                slots = host[lead:lead + stride * len(datas)].reshape(len(datas), stride)
                assert (slots[:, -4:] == 0xA5).all(), at
    # a capacity that cuts most blocks, slots that touch: a store past a block's capacity would land in its neighbour's stream
    cap = 301
    x, n = ragged(datas)
    out, lens = lzs.compress_blocks_sync(x, n, out_capacity=cap)
    check(out, lens, datas, cap, "touching")


def test_corners(seg):
    """An empty block between two others; uniform rows without lengths; one block against compress_stream(); blocks of 1, 2 and
    520 bytes; two identical blocks side by side; a run over many segments with a block right behind it that continues the run."""
    rng = np.random.default_rng(24)
    text = bytes(rng.choice(np.frombuffer(b"abcdefgh ", dtype=np.uint8), 3000))
    datas = [text[:700], b"", text[700:1500]]
    x, n = ragged(datas)
    out, lens = lzs.compress_blocks_sync(x, n)
    check(out, lens, datas, label="empty")
    assert out[1, :2].cpu().numpy().tobytes() == b"\xC0\x00" and lens[1] == 2
    # uniform rows, no lengths
    rows = [text[k * 752:(k + 1) * 752] for k in range(3)]
    x, _ = ragged(rows, stride=752)
    out, lens = lzs.compress_blocks_sync(x)
    check(out, lens, rows, label="uniform")
    # one block
    x, n = ragged([text])
    out, lens = lzs.compress_blocks_sync(x, n)
    check(out, lens, [text], label="one")
    one, got = lzs.compress_stream(x[0, :len(text)].contiguous())
    assert got == lens[0] and one[:got].cpu().numpy().tobytes() == out[0, :lens[0]].cpu().numpy().tobytes()
    # the shortest blocks
    datas = [text[:1], text[:2], text[:520]]
    x, n = ragged(datas)
    out, lens = lzs.compress_blocks_sync(x, n)
    check(out, lens, datas, label="short")
    # identical neighbours, nothing between them: a segment reaching back into the block before would find matches there
    datas = [text[:1024], text[:1024]]
    x, n = ragged(datas, stride=1024)
    out, lens = lzs.compress_blocks_sync(x, n)
    check(out, lens, datas, label="twins")
    assert out[0, :lens[0]].cpu().numpy().tobytes() == out[1, :lens[1]].cpu().numpy().tobytes()
    # one match over many segments, and the same byte pattern going on in the next block, right behind in memory
    run = (b"abc" * 2000)[:4096]
    datas = [b"q" + run[:4095], run[1:] + b"a"]
    x, n = ragged(datas, stride=4096)
    out, lens = lzs.compress_blocks_sync(x, n)
    check(out, lens, datas, label="run")


def test_the_routes_agree(monkeypatch):
    """The same batch by the rule, by workgroups and by segments, one batch either side of the rule's thresholds
    (lzs_plan_batch_compress_route(): the longest block one byte short of LZS_PLAN_BC_SEG_MIN_LONGEST, and at it): the same
    lengths and bytes in all three."""
    rng = np.random.default_rng(8)
    for longest in (MIN_LONGEST - 1, MIN_LONGEST):
        datas = [bytes(rng.choice(np.frombuffer(b"the quick brown fox ", dtype=np.uint8), n)) for n in (longest, longest // 3)]
        x, n = ragged(datas)
        seen = []
        for forced in (None, "1", "2"):
            if forced:
                monkeypatch.setenv("LZS_BATCH_COMPRESS_ROUTE", forced)
            else:
                monkeypatch.delenv("LZS_BATCH_COMPRESS_ROUTE", raising=False)
            out, lens = lzs.compress_blocks_sync(x, n)
            host = out.cpu().numpy()
            seen.append([host[b, :lens[b]].tobytes() for b in range(len(datas))])
        assert seen[0] == seen[1] == seen[2], longest
        assert seen[0] == [_want(d) for d in datas], longest


def _digest(datas):
    h = hashlib.sha256()
    for d in datas:
        h.update(len(d).to_bytes(4, "little") + d)
    return h.hexdigest()


BATCH_CHILD = (
    "import sys, hashlib, numpy as np, torch, lzs_compression_amd as lzs, stream_compress_programs as P\n"
    "datas = [i.data for i in P.directed_inputs() if not sys.argv[1:] or i.family in sys.argv[1:]]\n"
    "stride = (max(len(d) for d in datas) + 15) // 16 * 16\n"
    "host = np.zeros((len(datas), stride), dtype=np.uint8)\n"
    "for b, d in enumerate(datas): host[b, :len(d)] = np.frombuffer(d, dtype=np.uint8)\n"
    "out, lens = lzs.compress_blocks_sync(torch.from_numpy(host).cuda(), np.array([len(d) for d in datas], dtype=np.uint32))\n"
    "out = out.cpu().numpy()\n"
    "h = hashlib.sha256()\n"
    "for b in range(len(datas)): h.update(int(lens[b]).to_bytes(4, 'little') + out[b, :lens[b]].tobytes())\n"
    "print(h.hexdigest())\n")


def test_chain_safe_form_in_a_process_of_its_own():
    """LZS_CHAIN_FALLBACK=1 (decided once per process): the order-independent CHAIN form of the batch segment kernel on the whole
    directed batch, at both segment sizes; a digest of all streams against the oracle's."""
    expect = _digest([want(i) for i in inputs()])
    for size in SEGS:
        env = dict(os.environ, **CHILD_ENV, LZS_CHAIN_FALLBACK="1", LZS_STREAM_SEG=str(size))
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", BATCH_CHILD], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.strip() == expect, size


def test_rounds_are_the_models_summed_over_blocks():
    """The entry rounds of a batch made of the family-C inputs, in 256-byte segments, from the LZS_STREAM_DEBUG lines of a process
    of its own: after every round as many segments to redo as the model's rounds of every block give in sum -- the host's rule is
    deterministic, and a round runs over all blocks at once.  No time is asserted."""
    group = inputs("C")
    env = dict(os.environ, **CHILD_ENV, LZS_STREAM_DEBUG="1", LZS_STREAM_SEG="256")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", BATCH_CHILD, "C"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == _digest([want(i) for i in group])
    redo = [int(v) for v in re.findall(r"round \d+ compressed \d+ segments in [0-9.]+ ms; (\d+) to redo", r.stderr)]
    expect = []
    for i in group:
        _, _, rounds = O.compress_segments(i.data, 256)
        rounds = list(rounds)
        expect += [0] * (len(rounds) - len(expect))
        for k, v in enumerate(rounds):
            expect[k] += int(v)
    print(redo, expect)
    assert redo == expect
