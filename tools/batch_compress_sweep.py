"""lzs_compress_batch_device_sync() against the two ways a caller had before it, the sweep that gives
lzs_plan_batch_compress_route() its thresholds:

    (a) lzs_compress_batch_device, one workgroup a block, plus the copy of the lengths and a synchronise -- timed as such, and
        as the new call with LZS_BATCH_COMPRESS_ROUTE=1, which must agree with it;
    (b) the new call with LZS_BATCH_COMPRESS_ROUTE=2, every block cut into segments, at half, once and twice the segment size
        stream_seg() chooses for the batch's total input (LZS_STREAM_SEG);
    (c) a loop of lzs_compress_stream_device over the blocks;
    and the new call with nothing forced.

Rows, for each class of the seeded generators: 1, 8 and 64 blocks of 16 MiB; 64, 256 and 1024 of 1 MiB; 256, 1024, 1536 and 4096
of 64 KiB.  Data generated on the device.  Every row is warmed up once and timed with device events around the whole call, the
device idle before it: best / median / worst of --reps, ms.  Every timed result is compared with (a)'s lengths.  One JSON line a
row and a table to --out; run it twice for the run-to-run spread.

    python tools/batch_compress_sweep.py --out profiles/r24/batch_compress.txt
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("LZS_DEV_ENV", "1")          # the switches are read afresh at every call

SHAPES = ((1, 16 << 20), (8, 16 << 20), (64, 16 << 20), (64, 1 << 20), (256, 1 << 20), (1024, 1 << 20),
          (256, 64 << 10), (1024, 64 << 10), (1536, 64 << 10), (4096, 64 << 10))


def stream_seg(n):
    """csrc/lzs_stream.c: stream_seg(), restated (the tool only uses it to choose the sizes it forces)."""
    seg = 512 if n <= 256 << 10 else 1024 if n <= 1 << 20 else 2048 if n <= 4 << 20 else 4096 if n <= 32 << 20 else (n // 512 + 4095) & ~4095
    return max(256, min(seg, 65536)) & ~63


def timed(fn, reps):
    import torch
    fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return [round(v, 3) for v in (min(ms), statistics.median(ms), max(ms))]


def forced(route=None, seg=None):
    for name, value in (("LZS_BATCH_COMPRESS_ROUTE", route), ("LZS_STREAM_SEG", seg)):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(value)


def row(cls, nblocks, block, a, device):
    import numpy as np
    import torch
    import lzs_compression_amd as lzs
    x = lzs.workload.fill_device(cls, nblocks * block // 65536, 65536).view(nblocks, block)
    cap = lzs.compressed_max(block)
    out = torch.empty((nblocks, (cap + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
    d_len = torch.empty(nblocks, dtype=torch.int32, device="cuda")
    line = {"tool": "batch_compress_sweep", "class": cls, "blocks": nblocks, "block": block, **device}

    def parent():
        lzs.compress_blocks(x, None, cap, out=out, out_len=d_len)
        return d_len.cpu().numpy()

    want = parent().astype(np.uint32)
    line["compressed"] = int(want.sum())
    forced()
    line["a_async_ms"] = timed(parent, a.reps)

    def sync():
        got = lzs.compress_blocks_sync(x, None, cap, out=out)[1]
        assert (got == want).all(), (cls, nblocks, block, dict(os.environ))

    forced(route=1)
    line["a_route1_ms"] = timed(sync, a.reps)
    choice = stream_seg(nblocks * block)
    line["seg_choice"] = choice
    for seg in sorted({max(256, choice // 2), choice, min(65536, choice * 2)}):
        forced(route=2, seg=seg)
        line[f"b_seg{seg}_ms"] = timed(sync, a.reps)
    forced()
    line["unforced_ms"] = timed(sync, a.reps)

    def loop():
        for b in range(nblocks):
            lzs.compress_stream(x[b], out=out[b])

    if nblocks <= a.loop_max:
        line["c_loop_ms"] = timed(loop, a.reps)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--classes", default="text,lowent,random")
    ap.add_argument("--max-bytes", type=int, default=1 << 30, help="skip rows above this much input")
    ap.add_argument("--loop-max", type=int, default=1024, help="column (c) only up to this many blocks")
    ap.add_argument("--label", default="", help="a word for the table's head, such as the commit the library was built from")
    ap.add_argument("--only-a", action="store_true", help="column (a) alone: what a library without the new call can be asked")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "batch_compress.txt"))
    a = ap.parse_args()
    import torch
    import lzs_compression_amd as lzs
    torch.cuda.set_device(0)
    lzs.backend_info()
    props = torch.cuda.get_device_properties(0)
    device = {"device": props.name, "cus": props.multi_processor_count}
    lines = []
    for cls in a.classes.split(","):
        for nblocks, block in SHAPES:
            if nblocks * block > a.max_bytes:
                continue
            if a.only_a:
                x = lzs.workload.fill_device(cls, nblocks * block // 65536, 65536).view(nblocks, block)
                cap = lzs.compressed_max(block)
                out = torch.empty((nblocks, (cap + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
                d_len = torch.empty(nblocks, dtype=torch.int32, device="cuda")
                line = {"tool": "batch_compress_sweep", "class": cls, "blocks": nblocks, "block": block, **device}
                line["a_async_ms"] = timed(lambda: (lzs.compress_blocks(x, None, cap, out=out, out_len=d_len), d_len.cpu()), a.reps)
                del x, out
            else:
                line = row(cls, nblocks, block, a, device)
            print(json.dumps(line), flush=True)
            lines.append(line)
            lzs.release_thread_cache()
    text = f"# tools/batch_compress_sweep.py {a.label} on {device['device']} ({device['cus']} CUs): device events around the whole call, one warm-up,\n" \
           f"# best / median / worst of {a.reps}, ms\n" \
           "# class, blocks x bytes | (a) async + lengths + sync | (a) route 1 | (b) route 2 at seg ... | unforced | (c) loop of one-stream calls\n"
    for r in lines:
        b = "  ".join(f"{k[5:-3]}: {v}" for k, v in r.items() if k.startswith("b_seg"))
        text += "# %-7s %5d x %8d | %s | %s | %s | %s | %s\n" % (r["class"], r["blocks"], r["block"], r["a_async_ms"], r.get("a_route1_ms", "-"), b or "-",
                                                                r.get("unforced_ms", "-"), r.get("c_loop_ms", "-"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n".join(json.dumps(r) for r in lines) + "\n")
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
