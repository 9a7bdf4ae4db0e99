"""The size query for long streams against the two ways a caller had before it:

    (a) the lane-per-stream query of the same library (lzs_decompressed_size_batch_device), and
    (b) decoding into scratch memory of the known size (lzs_decompress_stream_device / lzs_decompress_batch_device_sync).

Rows: ONE stream of 64 KiB, 1 MiB, 64 MiB and 1 GiB of text and of 1 GiB of low and of high entropy; then a batch of a constant
64 MiB of compressed bytes in blocks of 1.5, 4, 16, 64, 256 KiB and 1 MiB (raw), every class, lzs_decompressed_size_batch_device_sync
with either route forced (LZS_SIZE_ROUTE) -- the sweep that gives lzs_plan_size_route() its threshold: the smallest swept average
compressed length from which the route by segments is faster on all three classes.

Data from the device generator, compressed on the device.  The calls synchronise, so the clock is the host's around the call, the
device idle before it; two warm-up calls, then best, median and worst of --reps.  The lane query of one stream is one lane's serial
walk -- 0.27 s a compressed MB, minutes for a GiB of text -- so from --lane-once-from bytes of raw data on it is timed once, without
a warm-up, and above --lane-max compressed bytes not at all: the table says "not run" there.  Every timed answer is checked (the raw size, END_MARKER).  One JSON line a row, and a table, to --out.

    python tools/size_stream_bench.py --out profiles/r20/size_stream.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STREAMS = (("text", 64 << 10), ("text", 1 << 20), ("text", 64 << 20), ("text", 1 << 30), ("lowent", 1 << 30), ("random", 1 << 30))
BLOCKS = (1536, 4 << 10, 16 << 10, 64 << 10, 256 << 10, 1 << 20)


def timed(fn, reps, warmup=2):
    """(best, median, worst) milliseconds of fn(), which ends synchronised."""
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return [round(v, 4) for v in (min(ms), statistics.median(ms), max(ms))]


def one_stream(cls, nbytes, a, device):
    import torch
    import lzs_compression_amd as lzs
    block = min(nbytes, 65536)
    raw = lzs.workload.fill_device(cls, nbytes // block, block).view(-1)
    buf, n = lzs.compress_stream(raw)
    del raw
    stream = buf[:n]
    line = {"tool": "size_stream_bench", "row": "one stream", "class": cls, "raw": nbytes, "compressed": n, **device}
    assert lzs.decompressed_size_stream(stream) == (nbytes, lzs.STATUS_END_MARKER)
    line["size_stream_ms"] = timed(lambda: lzs.decompressed_size_stream(stream), a.reps)
    assert lzs.decompressed_size_stream(stream, concat=True) == (nbytes, 3)
    line["size_stream_concat_ms"] = timed(lambda: lzs.decompressed_size_stream(stream, concat=True), a.reps)
    out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert lzs.decompress_stream(stream, nbytes, out=out)[1] == nbytes
    line["decode_ms"] = timed(lambda: lzs.decompress_stream(stream, nbytes, out=out), a.reps)
    del out
    if n <= a.lane_max:
        size = torch.empty(1, dtype=torch.int32, device="cuda")
        status = torch.empty(1, dtype=torch.uint8, device="cuda")

        def lanes():
            lzs.decompressed_sizes(stream.view(1, -1), None, None, size=size, status=status)
            torch.cuda.synchronize()

        once = nbytes >= a.lane_once_from
        line["lanes_ms"] = timed(lanes, 1 if once else a.reps, 0 if once else 2)
        line["lanes_runs"] = 1 if once else a.reps
        assert (int(size.item()), int(status.item())) == (nbytes, lzs.STATUS_END_MARKER)
    return line


def batch(cls, block, a, device):
    import numpy as np
    import torch
    import lzs_compression_amd as lzs
    probe, probe_lens = lzs.compress_blocks(lzs.workload.fill_device(cls, 64, block))
    mean = max(int(probe_lens.sum().item()) // 64, 1)
    nblocks = max(a.batch_bytes // mean, 1)
    del probe, probe_lens
    raw = lzs.workload.fill_device(cls, nblocks, block)
    slots, lens = lzs.compress_blocks(raw)
    torch.cuda.synchronize()
    del raw
    h_lens = lens.cpu().numpy().astype(np.uint32)
    line = {"tool": "size_stream_bench", "row": "batch", "class": cls, "raw": block, "blocks": nblocks,
            "compressed": int(h_lens.sum()), "mean_compressed": int(h_lens.sum()) // nblocks, **device}
    for route in ("lanes", "segments"):
        os.environ["LZS_SIZE_ROUTE"] = route
        size, status = lzs.decompressed_sizes_sync(slots, h_lens)
        assert (size == block).all() and (status == lzs.STATUS_END_MARKER).all(), (cls, block, route)
        line[route + "_ms"] = timed(lambda: lzs.decompressed_sizes_sync(slots, h_lens), a.reps)
    del os.environ["LZS_SIZE_ROUTE"]
    out = torch.empty((nblocks, block), dtype=torch.uint8, device="cuda")
    _, out_len = lzs.decompress_blocks_sync(slots, h_lens, block, out=out)
    assert (out_len == block).all()
    line["decode_ms"] = timed(lambda: lzs.decompress_blocks_sync(slots, h_lens, block, out=out), a.reps)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", default="streams,batch")
    ap.add_argument("--classes", default="text,lowent,random")
    ap.add_argument("--max-stream", type=int, default=1 << 30, help="skip one-stream rows above this many raw bytes")
    ap.add_argument("--batch-bytes", type=int, default=64 << 20, help="compressed bytes of every batch of the sweep")
    ap.add_argument("--lane-once-from", type=int, default=16 << 20)
    ap.add_argument("--lane-max", type=int, default=64 << 20, help="COMPRESSED bytes above which one stream's lane query is not run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "size_stream.txt"))
    a = ap.parse_args()
    import torch
    import lzs_compression_amd as lzs
    torch.cuda.set_device(0)
    lzs.backend_info()
    props = torch.cuda.get_device_properties(0)
    device = {"device": props.name, "cus": props.multi_processor_count}
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    if "streams" in a.rows:
        for cls, nbytes in STREAMS:
            if nbytes <= a.max_stream and cls in a.classes.split(","):
                emit(one_stream(cls, nbytes, a, device))
                lzs.release_thread_cache()
    if "batch" in a.rows:
        for cls in a.classes.split(","):
            for block in BLOCKS:
                emit(batch(cls, block, a, device))
                lzs.release_thread_cache()
    text = f"# tools/size_stream_bench.py on {device['device']} ({device['cus']} CUs): host clock around synchronous calls, 2 warm-up calls,\n" \
           f"# best / median / worst of {a.reps}, ms (lanes of one stream from {a.lane_once_from} raw bytes on: one call, no warm-up)\n"
    rows = [r for r in lines if r["row"] == "one stream"]
    if rows:
        text += "# one stream: class, raw bytes, compressed | size_stream | size_stream, file rule | (a) lanes | (b) decode into scratch\n"
        for r in rows:
            text += "# %-7s %11d %11d | %s | %s | %s | %s\n" % (r["class"], r["raw"], r["compressed"], r["size_stream_ms"], r["size_stream_concat_ms"],
                                                              r.get("lanes_ms", "not run (one lane, > %d compressed bytes)" % a.lane_max), r["decode_ms"])
    rows = [r for r in lines if r["row"] == "batch"]
    if rows:
        text += "# batch: class, raw block, blocks, mean compressed | by lanes (a) | by segments | (b) decode into scratch\n"
        for r in rows:
            text += "# %-7s %8d %8d %8d | %s | %s | %s\n" % (r["class"], r["raw"], r["blocks"], r["mean_compressed"], r["lanes_ms"], r["segments_ms"],
                                                           r["decode_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n".join(json.dumps(r) for r in lines) + "\n")
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
