"""Packed decode (lzs_decompress_batch_packed_device) against the route a caller had before it: decode into
slots of the largest size with lzs_decompress_batch_device, then lzs_compact_device.  Workloads per class of the device generator
(text, low entropy, high entropy), compressed on the device:

    A    16 384 blocks of 64 KiB
    B    65 536 packets of 1500 bytes
    Bv   65 536 packets of 40 to 1500 bytes

Timed, each between two device events, two warm-up calls, the best of --reps:

    (i)    slots + compact, in a process of its own that loads --parent-library (LZS_LIBRARY): the parent commit's build.  The
           whole measurement is made --spread times; its lowest and highest best-of are the run-to-run spread the others are
           read against.
    (ii)   packed decode, outputs packed at align 1
    (iii)  packed decode, outputs packed at align 16
    (iv)   the packed size query and the strided one on the same streams
    (v)    with --byte-drain-library (a build with -DLZS_PACKED_BYTE_DRAIN): (ii) with the strided calls' drain, which stores a
           block byte by byte when it does not start on a 16-byte boundary

and the bytes of device memory each route needs for its output.  Every timed result is checked against the raw data.  Each worker
process runs under its own time limit.  Prints one JSON line per class and workload, and writes them with a table to --out.

    python tools/packed_decode_bench.py --parent-library /path/to/parent/liblzs.so --out profiles/r11/packed_decode.txt
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
    """(raw rows, raw lengths, compressed slots, compressed lengths, the raw bytes back to back)"""
    import torch
    import lzs_compression_amd as lzs
    n, lo, hi = WORKLOADS[name]
    x = lzs.workload.fill_device(cls, n, hi)
    g = torch.Generator(device="cpu").manual_seed(n + lo)
    raw_len = (torch.randint(lo, hi + 1, (n,), generator=g, dtype=torch.int32) if lo != hi else torch.full((n,), hi, dtype=torch.int32)).cuda()
    slots, lens = lzs.compress_blocks(x, raw_len)
    torch.cuda.synchronize()
    flat = x[torch.arange(hi, device="cuda")[None, :] < raw_len[:, None]] if lo != hi else x.reshape(-1)
    return x, raw_len, slots, lens, flat


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
            x, raw_len, slots, lens, flat = _workload(cls, name)
            total = int(raw_len.sum().item())
            line = {"tool": "packed_decode_bench", "worker": a.worker, "class": cls, "workload": name, "blocks": n, "raw_mb": round(total / 1e6, 2),
                    "compressed_mb": round(int(lens.sum().item()) / 1e6, 2), "library": os.environ.get("LZS_LIBRARY", "this tree"), **device}
            if a.worker == "slots":
                stride = (hi + 15) // 16 * 16
                out = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
                out_len = torch.empty(n, dtype=torch.int32, device="cuda")
                dense = torch.empty(n * stride, dtype=torch.uint8, device="cuda")
                offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")

                def route():
                    lzs.decompress_blocks(slots, lens, hi, out=out, out_len=out_len)
                    lzs.compact(out, out_len, dense=dense, offsets=offsets)

                line["slots_ms"] = [round(_event_ms(route, a.reps), 4) for _ in range(a.spread)]
                assert int(offsets[-1].item()) == total and torch.equal(dense[:total], flat)
                # (the slots, and a dense result of the bytes it turns out to need: compact() itself asks for as much again)
                line["slots_bytes"] = n * stride + total + 4 * n + 8 * (n + 1)
                del out, dense
            else:
                packed, in_off = lzs.compact(slots, lens)
                torch.cuda.synchronize()
                packed = packed[:int(in_off[-1].item())].clone()
                size = torch.empty(n, dtype=torch.int32, device="cuda")
                status = torch.empty(n, dtype=torch.uint8, device="cuda")
                line["size_packed_ms"] = round(_event_ms(lambda: lzs.decompressed_sizes_packed(packed, in_off, size=size, status=status), a.reps), 4)
                assert torch.equal(size, raw_len) and bool((status == lzs.STATUS_END_MARKER).all())
                line["size_strided_ms"] = round(_event_ms(lambda: lzs.decompressed_sizes(slots, lens, size=size, status=status), a.reps), 4)
                out_len = torch.empty(n, dtype=torch.int32, device="cuda")
                for align in (1, 16):
                    off = lzs.offsets_from_sizes(size, align)
                    line[f"offsets_ms_align{align}"] = round(_event_ms(lambda: lzs.offsets_from_sizes(size, align, offsets=off), a.reps), 4)
                    out = torch.empty(int(off[-1].item()), dtype=torch.uint8, device="cuda")
                    line[f"packed_ms_align{align}"] = round(_event_ms(lambda: lzs.decompress_packed(packed, in_off, out, off, out_len=out_len), a.reps), 4)
                    assert torch.equal(out_len, raw_len)
                    if align == 1:
                        assert torch.equal(out, flat)
                    elif lo == hi:
                        assert torch.equal(out.view(n, -1)[:, :hi].reshape(-1), flat)
                    else:
                        idx = off[:-1, None] + torch.arange(hi, device="cuda")[None, :]
                        assert torch.equal(out[idx[torch.arange(hi, device="cuda")[None, :] < raw_len[:, None]]], flat)
                        del idx
                    line[f"packed_bytes_align{align}"] = int(off[-1].item()) + 4 * n + 8 * (n + 1)
                    del out
            print(json.dumps(line), flush=True)
            del x, slots, lens, flat


def _run_worker(kind, a, library):
    env = dict(os.environ)
    if library:
        env["LZS_LIBRARY"] = library
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--classes", a.classes, "--workloads", a.workloads,
           "--reps", str(a.reps), "--spread", str(a.spread)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.timeout)
    sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit(f"packed_decode_bench: the {kind} worker failed with status {r.returncode}")
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--classes", default="text,lowent,random")
    ap.add_argument("--workloads", default="A,B,Bv")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spread", type=int, default=3, help="how many times route (i) is measured")
    ap.add_argument("--parent-library", default="", help="the liblzs.so of the parent commit: route (i)")
    ap.add_argument("--byte-drain-library", default="", help="a build with -DLZS_PACKED_BYTE_DRAIN: row (v)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "packed_decode.txt"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds, for each worker process")
    ap.add_argument("--worker", choices=("slots", "packed"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    old = _run_worker("slots", a, a.parent_library)
    new = _run_worker("packed", a, "")
    drain = _run_worker("packed", a, a.byte_drain_library) if a.byte_drain_library else []
    rows = []
    for s in new:
        key = (s["class"], s["workload"])
        line = {k: v for k, v in s.items() if k not in ("worker", "library")}
        o = next((o for o in old if (o["class"], o["workload"]) == key), None)
        if o:
            line.update({"slots_ms_low": min(o["slots_ms"]), "slots_ms_high": max(o["slots_ms"]), "slots_bytes": o["slots_bytes"],
                         "slots_library": o["library"]})
        d = next((d for d in drain if (d["class"], d["workload"]) == key), None)
        if d:
            line["byte_drain_ms_align1"] = d["packed_ms_align1"]
        print(json.dumps(line), flush=True)
        rows.append(line)
    nan = float("nan")
    head = f"# tools/packed_decode_bench.py, one session on {rows[0]['device']} ({rows[0]['cus']} CUs, {rows[0]['clock_mhz']} MHz): device events,\n" \
           f"# 2 warm-up calls, best of {a.reps}; (i) slots + compact: {a.parent_library or 'this tree (no --parent-library)'}, measured {a.spread} times (low - high)\n" \
           "# ms: (i) slots+compact | (ii) packed align 1 | (iii) packed align 16 | (v) align 1, byte drain | (iv) size packed / strided;  MB of output memory: (i) | (ii)\n" \
           "# class   wl  blocks  raw MB       (i) low - high     (ii)    (iii)      (v)   (iv) packed  strided    MB (i)   MB (ii)\n"
    table = ""
    for r in rows:
        table += f"# {r['class']:7s} {r['workload']:3s} {r['blocks']:6d} {r['raw_mb']:8.2f} {r.get('slots_ms_low', nan):9.4f} - {r.get('slots_ms_high', nan):7.4f} " \
                 f"{r['packed_ms_align1']:8.4f} {r['packed_ms_align16']:8.4f} {r.get('byte_drain_ms_align1', nan):8.4f} {r['size_packed_ms']:13.4f} " \
                 f"{r['size_strided_ms']:8.4f} {r.get('slots_bytes', 0) / 1e6:9.1f} {r['packed_bytes_align1'] / 1e6:9.1f}\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(head + table + "\n".join(json.dumps(r) for r in rows) + "\n")
    sys.stdout.write(head + table)


if __name__ == "__main__":
    main()
