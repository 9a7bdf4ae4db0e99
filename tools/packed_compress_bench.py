"""Packed compression (lzs_compress_batch_packed_device) against the route a caller had before it: scatter the
packed blocks into slots of the largest size, lzs_compress_batch_device into slots of LZS_COMPRESSED_MAX(largest), then
lzs_compact_device.  Workloads per class of the device generator (text, low entropy, high entropy), the blocks back to back:

    A    16 384 blocks of 64 KiB
    B    65 536 packets of 1500 bytes
    Bv   65 536 packets of 40 to 1500 bytes

Timed, each between two device events, two warm-up calls, the best of --reps:

    (i)    scatter + compress_blocks + compact, in a process of its own that loads --parent-library (LZS_LIBRARY): the parent
           commit's build.  The whole measurement is made --spread times; its lowest and highest best-of are the run-to-run
           spread the others are read against.  (On A and B the blocks already lie at a stride: the scatter is a view and costs
           nothing.)
    (ii)   the device work of compress_dense at align 16: bounds, rooms' offsets, compress_packed, scan, compact_packed, into
           buffers made beforehand
    (iii)  compress_packed alone (rooms at align 16) and the parent's compress_blocks alone, measured --spread times like (i)

and the bytes of device memory each route needs beside its input.  Every timed result is decoded and checked against the raw
data.  Each worker process runs under its own time limit.  Prints one JSON line per class and workload, and writes them with a
table to --out.

    python tools/packed_compress_bench.py --parent-library /path/to/parent/liblzs.so --out profiles/r14/packed_compress.txt
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORKLOADS = {"A": (16384, 65536, 65536), "B": (65536, 1500, 1500), "Bv": (65536, 40, 1500)}


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


def _workload(cls, name):
    """(the raw bytes back to back, in_off int64 [n + 1], raw lengths int32, the mask of the rows' bytes or None for one length)"""
    import torch
    import lzs_compression_amd as lzs
    n, lo, hi = WORKLOADS[name]
    x = lzs.workload.fill_device(cls, n, hi)
    g = torch.Generator(device="cpu").manual_seed(n + lo)
    raw_len = (torch.randint(lo, hi + 1, (n,), generator=g, dtype=torch.int32) if lo != hi else torch.full((n,), hi, dtype=torch.int32)).cuda()
    mask = torch.arange(hi, device="cuda")[None, :] < raw_len[:, None] if lo != hi else None
    flat = x[mask] if lo != hi else x.reshape(-1)
    in_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    in_off[1:] = torch.cumsum(raw_len.to(torch.int64), 0)
    torch.cuda.synchronize()
    return flat, in_off, raw_len, mask


def worker(a):
    """One process, one library: --worker slots (the route before) or --worker packed."""
    import torch
    import lzs_compression_amd as lzs
    torch.cuda.set_device(0)
    lzs.backend_info()
    props = torch.cuda.get_device_properties(0)
    device = {"device": props.name, "cus": props.multi_processor_count, "clock_mhz": getattr(props, "clock_rate", 0) // 1000}
    for cls in a.classes.split(","):
        for name in a.workloads.split(","):
            n, lo, hi = WORKLOADS[name]
            flat, in_off, raw_len, mask = _workload(cls, name)
            total = flat.numel()
            line = {"tool": "packed_compress_bench", "worker": a.worker, "class": cls, "workload": name, "blocks": n, "raw_mb": round(total / 1e6, 2),
                    "library": os.environ.get("LZS_LIBRARY", "this tree"), **device}
            if a.worker == "slots":
                cap = lzs.compressed_max(hi)
                stride = (cap + 15) // 16 * 16
                rows = torch.zeros((n, hi), dtype=torch.uint8, device="cuda") if mask is not None else flat.view(n, hi)
                out = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
                out_len = torch.empty(n, dtype=torch.int32, device="cuda")
                dense = torch.empty(n * stride, dtype=torch.uint8, device="cuda")
                offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")

                def route():
                    if mask is not None:
                        rows[mask] = flat                          # the scatter into input slots
                    lzs.compress_blocks(rows, raw_len, cap, out=out, out_len=out_len)
                    lzs.compact(out, out_len, dense=dense, offsets=offsets)

                line["slots_ms"] = [round(_event_ms(route, a.reps), 4) for _ in range(a.spread)]
                line["blocks_alone_ms"] = [round(_event_ms(lambda: lzs.compress_blocks(rows, raw_len, cap, out=out, out_len=out_len), a.reps), 4)
                                           for _ in range(a.spread)]
                back, back_len = lzs.decompress_blocks(out, out_len, hi)
                torch.cuda.synchronize()
                assert torch.equal(back_len, raw_len) and torch.equal(back[:, :hi][mask] if mask is not None else back[:, :hi].reshape(-1), flat)
                result = int(offsets[-1].item())
                line["compressed_mb"] = round(result / 1e6, 2)
                # (input slots where the blocks had to be scattered, output slots, and a dense result of the bytes it turns out
                # to need: compact() itself asks for as much as the slots again)
                line["slots_bytes"] = (n * hi if mask is not None else 0) + n * stride + result + 4 * n + 8 * (n + 1)
                del rows, out, dense, back
            else:
                bound = torch.empty(n, dtype=torch.int32, device="cuda")
                lzs.compressed_bounds_packed(in_off, bound=bound)
                room_off = lzs.offsets_from_sizes(bound, 16)
                rooms = torch.empty(int(room_off[-1].item()), dtype=torch.uint8, device="cuda")
                offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
                dense = torch.empty(rooms.numel(), dtype=torch.uint8, device="cuda")     # (the timed loop cannot size it by a host read)

                def route():
                    lzs.compressed_bounds_packed(in_off, bound=bound)
                    lzs.offsets_from_sizes(bound, 16, offsets=room_off)
                    lzs.compress_packed(flat, in_off, rooms, room_off, out_len=bound)
                    lzs.offsets_from_sizes(bound, 1, offsets=offsets)
                    lzs.compact_packed(rooms, room_off, bound, dense=dense, offsets=offsets)

                line["dense_ms"] = round(_event_ms(route, a.reps), 4)
                out_len = torch.empty(n, dtype=torch.int32, device="cuda")
                line["packed_alone_ms"] = [round(_event_ms(lambda: lzs.compress_packed(flat, in_off, rooms, room_off, out_len=out_len), a.reps), 4)
                                           for _ in range(a.spread)]
                result = int(offsets[-1].item())
                back, back_off = lzs.decompress_dense(dense[:result], offsets)
                torch.cuda.synchronize()
                assert torch.equal(back, flat) and torch.equal(back_off, in_off) and torch.equal(out_len, bound)
                line["compressed_mb"] = round(result / 1e6, 2)
                line["dense_bytes"] = rooms.numel() + result + 4 * n + 2 * 8 * (n + 1)
                del rooms, dense, back
            print(json.dumps(line), flush=True)
            del flat, mask


def _run_worker(kind, a, library):
    env = dict(os.environ)
    if library:
        env["LZS_LIBRARY"] = library
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--classes", a.classes, "--workloads", a.workloads,
           "--reps", str(a.reps), "--spread", str(a.spread)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.timeout)
    sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit(f"packed_compress_bench: the {kind} worker failed with status {r.returncode}")
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--classes", default="text,lowent,random")
    ap.add_argument("--workloads", default="A,B,Bv")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spread", type=int, default=3, help="how many times route (i) and the kernels alone are measured")
    ap.add_argument("--parent-library", default="", help="the liblzs.so of the parent commit: route (i)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "packed_compress.txt"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds, for each worker process")
    ap.add_argument("--worker", choices=("slots", "packed"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    old = _run_worker("slots", a, a.parent_library)
    new = _run_worker("packed", a, "")
    rows = []
    for s in new:
        line = {k: v for k, v in s.items() if k not in ("worker", "library")}
        o = next((o for o in old if (o["class"], o["workload"]) == (s["class"], s["workload"])), None)
        if o:
            assert o["compressed_mb"] == s["compressed_mb"], (o, s)
            line.update({"slots_ms_low": min(o["slots_ms"]), "slots_ms_high": max(o["slots_ms"]), "blocks_alone_ms_low": min(o["blocks_alone_ms"]),
                         "blocks_alone_ms_high": max(o["blocks_alone_ms"]), "slots_bytes": o["slots_bytes"], "slots_library": o["library"]})
        line["packed_alone_ms_low"], line["packed_alone_ms_high"] = min(s["packed_alone_ms"]), max(s["packed_alone_ms"])
        print(json.dumps(line), flush=True)
        rows.append(line)
    nan = float("nan")
    head = f"# tools/packed_compress_bench.py, one session on {rows[0]['device']} ({rows[0]['cus']} CUs, {rows[0]['clock_mhz']} MHz): device events,\n" \
           f"# 2 warm-up calls, best of {a.reps}; (i) scatter + compress_blocks + compact and compress_blocks alone: {a.parent_library or 'this tree (no --parent-library)'};\n" \
           f"# (i) and both kernels alone measured {a.spread} times (low - high)\n" \
           "# ms: (i) the route before | (ii) compress_dense's device work, align 16 | (iii) compress_packed alone | the parent's compress_blocks alone;  MB beside the input: (i) | (ii)\n" \
           "# class   wl  blocks  raw MB       (i) low - high      (ii)    (iii) packed low - high    blocks low - high    MB (i)   MB (ii)\n"
    table = ""
    for r in rows:
        table += f"# {r['class']:7s} {r['workload']:3s} {r['blocks']:6d} {r['raw_mb']:8.2f} {r.get('slots_ms_low', nan):9.4f} - {r.get('slots_ms_high', nan):8.4f} " \
                 f"{r['dense_ms']:9.4f} {r['packed_alone_ms_low']:15.4f} - {r['packed_alone_ms_high']:8.4f} {r.get('blocks_alone_ms_low', nan):9.4f} - " \
                 f"{r.get('blocks_alone_ms_high', nan):8.4f} {r.get('slots_bytes', 0) / 1e6:9.1f} {r['dense_bytes'] / 1e6:9.1f}\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(head + table + "\n".join(json.dumps(r) for r in rows) + "\n")
    sys.stdout.write(head + table)


if __name__ == "__main__":
    main()
