"""Packed bursts (lzs_*_channels_burst_packed_device) against the best route a caller had before them: the strided
burst calls on the same packets already scattered into slots of the largest size (the scatter is not charged), plus lzs_compact_device
for compression.  16 384 channels, packets of 40 to 1500 bytes of the device generator's classes, the three shapes of a drained queue
of DESIGN.md 3.11:

    a   4 packets per channel, every channel (65 536 packets)
    b   65 536 packets with Zipf(1.1) channel ids
    c   one channel with 300 packets among 16 383 single packets

Timed, each between two device events, two warm-up calls, the best of --reps:

    (i)   the strided route, in a process of its own that loads --parent-library (LZS_LIBRARY): the parent commit's build.  The whole
          measurement is made --spread times; its lowest and highest best-of are the run-to-run spread the other is read against.
    (ii)  the packed route of this tree: compress_channels_burst_packed into rooms of the bounds + compact_packed; decompress_channels_
          burst_packed into rooms of exactly the packets' sizes, with the split-size work area (as the strided decoder has)

and the bytes of device memory each route holds while it runs: packets, outputs, work area and the small arrays.  Both routes are
checked against the raw data.  Each worker process runs under its own time limit.  Prints one JSON line per class, shape and
direction, and writes them with a table to --out.

    python tools/packed_burst_bench.py --parent-library /path/to/parent/liblzs.so --out profiles/r19/packed_burst.txt
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LO, HI = 40, 1500


def _event_ms(fn, reps, warmup=2):
    """Milliseconds of one fn() between two device events: the best of `reps` after `warmup` untimed calls."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        t = t0.elapsed_time(t1)
        best = t if best is None else min(best, t)
    return best


def _ids(shape, nch, rng):
    import numpy as np
    if shape == "a":
        return np.tile(np.arange(nch), 4)
    if shape == "b":
        return (rng.zipf(1.1, 4 * nch) - 1) % nch
    return rng.permutation(np.concatenate([np.zeros(300, dtype=np.int64), np.arange(1, nch)]))


def _bytes(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors)


def worker(a):
    """One process, one library: --worker slots (the route before) or --worker packed."""
    import numpy as np
    import torch
    import lzs_compression_amd as lzs
    torch.cuda.set_device(0)
    lzs.backend_info()
    props = torch.cuda.get_device_properties(0)
    device = {"device": props.name, "cus": props.multi_processor_count}
    nch = a.channels
    for cls in a.classes.split(","):
        for shape in a.shapes.split(","):
            ids = _ids(shape, nch, np.random.default_rng(1))
            n = ids.size
            x = lzs.workload.fill_device(cls, n, HI)
            g = torch.Generator(device="cpu").manual_seed(n + LO)
            raw_len = torch.randint(LO, HI + 1, (n,), generator=g, dtype=torch.int32).cuda()
            keep = torch.arange(HI, device="cuda")[None, :] < raw_len[:, None]
            flat = x[keep]
            total = flat.numel()
            ch = torch.from_numpy(ids.astype(np.int32)).cuda()
            states = lzs.new_channel_states(nch)
            line = {"tool": "packed_burst_bench", "worker": a.worker, "class": cls, "shape": shape, "packets": n, "channels": nch,
                    "raw_mb": round(total / 1e6, 2), "library": os.environ.get("LZS_LIBRARY", "this tree"), **device}
            if a.worker == "slots":
                cap = lzs.compressed_max(HI)
                out = torch.empty((n, (cap + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
                out_len = torch.empty(n, dtype=torch.int32, device="cuda")
                status = torch.empty(n, dtype=torch.uint8, device="cuda")
                dense = torch.empty(out.numel(), dtype=torch.uint8, device="cuda")
                offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
                work = torch.empty(lzs.channels_burst_work_bytes(n, nch), dtype=torch.uint8, device="cuda")

                def compress():
                    states.zero_()
                    lzs.compress_channels_burst(x, raw_len, ch, states, cap, out=out, out_len=out_len, status=status, work=work)
                    lzs.compact(out, out_len, dense=dense, offsets=offsets)

                line["compress_ms"] = [round(_event_ms(compress, a.reps), 4) for _ in range(a.spread)]
                comp = int(offsets[-1].item())
                # (a dense result of the bytes it turns out to need: compact() itself asks for as much as the slots)
                line["compress_bytes"] = _bytes(x, raw_len, ch, out, out_len, status, offsets, work) + comp
                y, yl = out.clone(), out_len.clone()
                back = torch.empty((n, (HI + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
                large = torch.empty(lzs.channels_burst_split_work_bytes(n, nch, HI), dtype=torch.uint8, device="cuda")

                def decompress():
                    states.zero_()
                    lzs.decompress_channels_burst(y, yl, ch, states, HI, out=back, out_len=out_len, status=status, work=large)

                line["decompress_ms"] = [round(_event_ms(decompress, a.reps), 4) for _ in range(a.spread)]
                assert torch.equal(out_len, raw_len) and torch.equal(back[:, :HI][keep], flat)
                line["decompress_bytes"] = _bytes(y, yl, ch, back, out_len, status, large)
            else:
                in_off = lzs.offsets_from_sizes(raw_len, 1)
                bound = lzs.compressed_bounds_packed(in_off)
                room_off = lzs.offsets_from_sizes(bound, 16)
                rooms = torch.empty(int(room_off[-1].item()), dtype=torch.uint8, device="cuda")
                out_len = torch.empty(n, dtype=torch.int32, device="cuda")
                status = torch.empty(n, dtype=torch.uint8, device="cuda")
                offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
                dense = torch.empty(rooms.numel(), dtype=torch.uint8, device="cuda")
                work = torch.empty(lzs.channels_burst_work_bytes(n, nch), dtype=torch.uint8, device="cuda")

                def compress():
                    states.zero_()
                    lzs.compress_channels_burst_packed(flat, in_off, ch, states, rooms, room_off, out_len=out_len, status=status, work=work)
                    lzs.compact_packed(rooms, room_off, out_len, dense=dense, offsets=offsets)

                line["compress_ms"] = round(_event_ms(compress, a.reps), 4)
                comp = int(offsets[-1].item())
                assert bool((status == 0x07).all())
                line["compress_bytes"] = _bytes(flat, in_off, ch, rooms, room_off, out_len, status, offsets, work) + comp
                y, y_off = dense[:comp].clone(), offsets.clone()
                del rooms, dense
                back = torch.empty(total, dtype=torch.uint8, device="cuda")
                large = torch.empty(lzs.channels_burst_packed_split_work_bytes(n, nch, total), dtype=torch.uint8, device="cuda")

                def decompress():
                    states.zero_()
                    lzs.decompress_channels_burst_packed(y, y_off, ch, states, back, in_off, out_len=out_len, status=status, work=large)

                line["decompress_ms"] = round(_event_ms(decompress, a.reps), 4)
                assert torch.equal(out_len, raw_len) and torch.equal(back, flat) and bool((status == lzs.STATUS_END_MARKER).all())
                line["decompress_bytes"] = _bytes(y, y_off, ch, back, in_off, out_len, status, large)
            line["compressed_mb"] = round(comp / 1e6, 2)
            print(json.dumps(line), flush=True)


def _run_worker(kind, a, library):
    env = dict(os.environ)
    if library:
        env["LZS_LIBRARY"] = library
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--classes", a.classes, "--shapes", a.shapes,
           "--channels", str(a.channels), "--reps", str(a.reps), "--spread", str(a.spread)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.timeout)
    sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit(f"packed_burst_bench: the {kind} worker failed with status {r.returncode}")
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--channels", type=int, default=16384)
    ap.add_argument("--classes", default="text,lowent,random")
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spread", type=int, default=3, help="how many times route (i) is measured")
    ap.add_argument("--parent-library", default="", help="the liblzs.so of the parent commit: route (i)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "packed_burst.txt"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds, for each worker process")
    ap.add_argument("--worker", choices=("slots", "packed"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    old = _run_worker("slots", a, a.parent_library)
    new = _run_worker("packed", a, "")
    rows = []
    for s in new:
        o = next(o for o in old if (o["class"], o["shape"]) == (s["class"], s["shape"]))
        for direction in ("compress", "decompress"):
            low, high = min(o[direction + "_ms"]), max(o[direction + "_ms"])
            row = {"tool": "packed_burst_bench", "class": s["class"], "shape": s["shape"], "direction": direction, "packets": s["packets"],
                   "channels": s["channels"], "raw_mb": s["raw_mb"], "compressed_mb": s["compressed_mb"], "slots_ms_low": low,
                   "slots_ms_high": high, "packed_ms": s[direction + "_ms"], "slots_bytes": o[direction + "_bytes"],
                   "packed_bytes": s[direction + "_bytes"], "slower_than_the_spread": s[direction + "_ms"] - low > high - low, "slots_library": o["library"], "device": s["device"], "cus": s["cus"]}
            print(json.dumps(row), flush=True)
            rows.append(row)
    head = f"# tools/packed_burst_bench.py, one session on {rows[0]['device']} ({rows[0]['cus']} CUs): device events, 2 warm-up calls, best of\n" \
           f"# {a.reps}; (i) strided burst calls on slots (+ compact): {a.parent_library or 'this tree (no --parent-library)'}, measured {a.spread} times\n" \
           "# (low - high); (ii) packed burst calls of this tree (+ compact_packed).  MB: device memory each route holds.\n" \
           "# class   shape direction  packets  raw MB    (i) low - high      (ii)   MB (i)  MB (ii)  (ii) slower than (i) by more than its spread\n"
    table = ""
    for r in rows:
        table += f"# {r['class']:7s} {r['shape']:5s} {r['direction']:10s} {r['packets']:7d} {r['raw_mb']:7.2f} {r['slots_ms_low']:9.4f} - {r['slots_ms_high']:7.4f} " \
                 f"{r['packed_ms']:9.4f} {r['slots_bytes'] / 1e6:8.1f} {r['packed_bytes'] / 1e6:8.1f}  {'yes' if r['slower_than_the_spread'] else 'no'}\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(head + table + "\n".join(json.dumps(r) for r in rows) + "\n")
    sys.stdout.write(head + table)


if __name__ == "__main__":
    main()
