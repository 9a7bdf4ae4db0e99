"""One case of tests/test_gpu_compress_variants.py, in a process of its own (LZS_VARIANT and LZS_CHAIN_FALLBACK are read once per
process): `text`, `few`, `lit` (LZS_VARIANT), `safe` (LZS_CHAIN_FALLBACK=1) or `by-class` (neither).  The process first proves which
variant it runs, then compresses every built content of its table shape (tests/compress_variant_programs.py) at every cut
length through the strided and the packed entry, truncates four contents at eight capacities, and compares every block itself
with the oracle.  Its last line of output is one JSON object: {"case", "failures": [...], "blocks", "seconds"}; `failures` is empty
when every block was the oracle's.
"""
import ctypes
import json
import os
import sys
import time

T0 = time.time()
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.abspath(os.path.join(HERE, "..", "..")), os.path.abspath(os.path.join(HERE, ".."))]

import numpy as np                                  # noqa: E402
import torch                                        # noqa: E402

import oracle                                       # noqa: E402
import lzs_compression_amd as lzs                   # noqa: E402
from lzs_compression_amd import workload            # noqa: E402
import compress_variant_programs as P               # noqa: E402

from test_gpu_search_hop_end import LENGTHS         # noqa: E402

ROOMS = (0, 1, 2, 255, 256, 257)                    # ... and full - 1, full
CAPACITY_CLASS_CHANGES = ("text, then random", "zeros, then text", "random, then a run")     # one of each leading class
FORCED = {"text": 1, "few": 2, "lit": 3}
MOST_FAILURES = 40

O = oracle.oracle()
failures, blocks_checked = [], 0


def fail(**what):
    if len(failures) < MOST_FAILURES:
        failures.append(what)


def compare(got: bytes, got_len: int, want: bytes, **what):
    global blocks_checked
    blocks_checked += 1
    if got_len != len(want):
        fail(why=f"length {got_len}, the oracle's {len(want)}", **what)
    elif got != want:
        first = next(i for i in range(len(want)) if got[i] != want[i])
        fail(why=f"byte {first} of {len(want)} differs", **what)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def strided(rows, lens, cap=None, out=None):
    x, n = dev(rows), dev(lens.astype(np.int32))
    slots, got = lzs.compress_blocks(x, n, cap, out)
    torch.cuda.synchronize()
    return slots.cpu().numpy(), got.cpu().numpy()


def packed(datas, rooms=None):
    """One packed launch: block b is datas[b]; its room rooms[b], or -- None -- what compressed_bounds_packed says.  Returns the
    whole output (prefilled with 0xA5), the rooms' offsets and the lengths."""
    sizes = np.array([len(d) for d in datas], dtype=np.int64)
    in_off = np.concatenate(([0], np.cumsum(sizes)))
    data = dev(np.frombuffer(b"".join(datas), dtype=np.uint8))
    d_in_off = dev(in_off)
    if rooms is None:
        bound = lzs.compressed_bounds_packed(d_in_off)
        torch.cuda.synchronize()
        assert bound.cpu().numpy().tolist() == [oracle.compressed_max(len(d)) for d in datas]
    else:
        bound = dev(np.array(rooms, dtype=np.int32))
    out_off = lzs.offsets_from_sizes(bound, 1)
    torch.cuda.synchronize()
    off = out_off.cpu().numpy()
    out = torch.full((int(off[-1]) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    _, got = lzs.compress_packed(data, d_in_off, out, out_off)
    torch.cuda.synchronize()
    return out.cpu().numpy(), off, got.cpu().numpy()


def classify(rows, lens):
    L = lzs.lib()
    L.lzs_hip_classify_blocks.restype = ctypes.c_int
    L.lzs_hip_classify_blocks.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    x, n = dev(rows), dev(lens.astype(np.int32))
    codes = torch.zeros(len(rows), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert L.lzs_hip_classify_blocks(codes.data_ptr(), x.data_ptr(), rows.shape[1], n.data_ptr(), rows.shape[1], len(rows), None) == 0
    torch.cuda.synchronize()
    return (codes.cpu().numpy().astype(np.int64) & 0xF).tolist()


def rows_of(datas, stride):
    rows = np.zeros((len(datas), stride), dtype=np.uint8)
    for b, d in enumerate(datas):
        rows[b, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    return rows, np.array([len(d) for d in datas], dtype=np.uint32)


def prove_what_runs(case):
    forced = lzs.lib().lzs_hip_forced_variant
    forced.restype, forced.argtypes = ctypes.c_int, []
    info = lzs.backend_info()
    assert "gfx950" in info, info
    assert forced() == FORCED.get(case, 0), (case, forced())
    if case == "safe":
        assert "order-independent fallback" in info, info
    else:
        assert "ordered LDS exchange" in info, info      # (a device on the fallback runs wgv_safe whatever LZS_VARIANT says)


def by_class_first_launches(shape):
    """The first compress launch of the process -- nothing is known of earlier launches, all three variants run -- over 66 blocks:
    the class-change blocks, then twenty of each seeded class.  The classifier gives each class-change block the code its first
    2100 bytes were built for; a second launch, under what the first one's classifier left, gives the same bytes."""
    names = list(P.CLASS_CHANGES)
    stride = 40 * 1024
    datas = [P.class_change(n) for n in names]
    labels = [("class change", n) for n in names]
    want_codes = [P.CLASS_CHANGES[n][0] for n in names]
    for code, cls in enumerate(workload.CLASS_NAMES, 1):
        blk = workload.fill(cls, 20, stride, first_block=2000)
        datas += [blk[b].tobytes() for b in range(20)]
        labels += [(cls, b) for b in range(20)]
        want_codes += [code] * 20
    rows, lens = rows_of(datas, stride)
    assert len(rows) == 66
    codes = classify(rows, lens)
    if codes != want_codes:
        fail(shape=shape.name, what="classifier", why=f"codes {codes}, built for {want_codes}")
    want = [O.compress(d) for d in datas]
    for launch in (1, 2):
        out, n = strided(rows, lens)
        for b, w in enumerate(want):
            compare(out[b, :n[b]].tobytes(), int(n[b]), w, shape=shape.name, what=f"by-class launch {launch}", content=list(labels[b]), length=len(datas[b]))


def every_content_at_every_length(shape):
    cut = []                                           # (content, length, bytes)
    for name, built in P.contents(shape.name).items():
        cut += [(name, ln, built.data[:ln]) for ln in LENGTHS]
    for name in P.CLASS_CHANGES:
        d = P.class_change(name)
        cut += [("class change: " + name, ln, d[:ln]) for ln in (len(d),) + P.CLASS_CHANGE_LENGTHS]
    datas = [d for _, _, d in cut]
    want = [O.compress(d) for d in datas]
    rows, lens = rows_of(datas, P.BLOCK)
    out, n = strided(rows, lens)
    for b, (name, ln, _) in enumerate(cut):
        compare(out[b, :n[b]].tobytes(), int(n[b]), want[b], shape=shape.name, what="strided", content=name, length=ln)
    out, off, n = packed(datas)
    for b, (name, ln, _) in enumerate(cut):
        compare(out[off[b]:off[b] + n[b]].tobytes(), int(n[b]), want[b], shape=shape.name, what="packed", content=name, length=ln)
    if not (out[off[-1]:] == 0xA5).all():
        fail(shape=shape.name, what="packed", why="bytes behind the last room were written")


def capacities(shape):
    """The stream is the oracle's cut to the room, and every byte outside what was written is still 0xA5."""
    named = [("ladder", P.contents(shape.name)["ladder"].data)]
    named += [("class change: " + n, P.class_change(n)) for n in CAPACITY_CLASS_CHANGES]
    full = [O.compress(d) for _, d in named]
    # packed: one launch, a room each
    rooms = [r for w in full for r in ROOMS + (len(w) - 1, len(w))]
    datas = [d for _, d in named for _ in range(len(ROOMS) + 2)]
    out, off, n = packed(datas, rooms)
    written = np.zeros(len(out), dtype=bool)
    for b, room in enumerate(rooms):
        k = b // (len(ROOMS) + 2)
        assert off[b + 1] - off[b] == room
        compare(out[off[b]:off[b] + n[b]].tobytes(), int(n[b]), full[k][:room], shape=shape.name, what=f"packed, room {room}", content=named[k][0], length=len(named[k][1]))
        written[off[b]:off[b] + min(int(n[b]), room)] = True
    if not (out[~written] == 0xA5).all():
        bad = int(np.flatnonzero((out != 0xA5) & ~written)[0])
        b = min(int(np.searchsorted(off, bad, side="right")) - 1, len(rooms) - 1)
        fail(shape=shape.name, what=f"packed, room {rooms[b]}", content=named[b // (len(ROOMS) + 2)][0], length=len(datas[b]),
             why=f"byte {bad - int(off[b])} of the room, outside what was written, changed")
    # strided: a launch per capacity
    stride = max(len(d) for _, d in named)
    rows, lens = rows_of([d for _, d in named], stride)
    width = max(len(w) for w in full) + 64
    launches = [(cap, list(range(len(named)))) for cap in ROOMS]
    launches += [(len(w) - d, [k]) for k, w in enumerate(full) for d in (1, 0)]
    for cap, which in launches:
        out = torch.full((len(which), width), 0xA5, dtype=torch.uint8, device="cuda")
        got, n = strided(rows[which], lens[which], cap, out)
        for j, k in enumerate(which):
            compare(got[j, :n[j]].tobytes(), int(n[j]), full[k][:cap], shape=shape.name, what=f"strided, capacity {cap}", content=named[k][0], length=len(named[k][1]))
            if not (got[j, min(int(n[j]), cap):] == 0xA5).all():
                fail(shape=shape.name, what=f"strided, capacity {cap}", content=named[k][0], why="a byte past what was written changed")


def main(case):
    shape = P.SHAPES.get(case, P.DEFAULT)
    assert case in ("text", "few", "lit", "safe", "by-class"), case
    assert torch.cuda.is_available(), "needs a GPU (no fallback exists)"
    prove_what_runs(case)
    if case == "by-class":
        by_class_first_launches(shape)
    every_content_at_every_length(shape)
    capacities(shape)
    print(json.dumps({"case": case, "failures": failures, "blocks": blocks_checked, "seconds": round(time.time() - T0, 2)}))


if __name__ == "__main__":
    main(sys.argv[1])
