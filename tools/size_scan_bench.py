"""The size query (lzs_decompressed_size_batch_device) against the only other way to learn the decoded sizes:
decoding into a scratch buffer of the known size with lzs_decompress_batch_device.  Two workloads per class of the device
generator (text, low entropy, high entropy), compressed on the device:

    A   16 384 blocks of 64 KiB
    B   65 536 packets of 1500 bytes

Device events around one call, two warm-up calls, the best of --reps; the device's name and clock are noted.  The query is
timed at limit = 0xFFFFFFFF (size_ms), and one block of 1 MiB of text alone.  Every timed result is checked: the sizes are the raw
lengths, the status END_MARKER.

The decoder is timed in a process of its own that loads --decoder-library (LZS_LIBRARY): give it the library built from the
parent commit to compare against the decoder as it was, in the same session.  Without it this tree's decoder is timed, and the
output says so.  Prints one JSON line per class and workload, and writes them with a table to --out.

    python tools/size_scan_bench.py --decoder-library /path/to/parent/liblzs.so --out profiles/r10/size_scan.txt
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORKLOADS = {"A": (16384, 65536), "B": (65536, 1500)}


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


def _compressed(cls, n, length):
    import torch
    import lzs_compression_amd as lzs
    x = lzs.workload.fill_device(cls, n, length)
    slots, lens = lzs.compress_blocks(x)
    torch.cuda.synchronize()
    del x
    return slots, lens


def worker(a):
    """One process, one library: --worker size (this tree's query) or --worker decode (the decoder of the library loaded)."""
    import torch
    import lzs_compression_amd as lzs
    torch.cuda.set_device(0)
    lzs.backend_info()
    props = torch.cuda.get_device_properties(0)
    device = {"device": props.name, "cus": props.multi_processor_count, "clock_mhz": getattr(props, "clock_rate", 0) // 1000}
    for cls in a.classes.split(","):
        for name in a.workloads.split(","):
            n, length = WORKLOADS[name]
            slots, lens = _compressed(cls, n, length)
            line = {"tool": "size_scan_bench", "worker": a.worker, "class": cls, "workload": name, "blocks": n, "raw": length,
                    "compressed_mb": round(int(lens.sum().item()) / 1e6, 2), **device}
            if a.worker == "decode":
                out = torch.empty((n, (length + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
                out_len = torch.empty(n, dtype=torch.int32, device="cuda")
                line["decode_ms"] = round(_event_ms(lambda: lzs.decompress_blocks(slots, lens, length, out=out, out_len=out_len), a.reps), 4)
                assert bool((out_len == length).all())
                line["library"] = os.environ.get("LZS_LIBRARY", "this tree")
                del out
            else:
                size = torch.empty(n, dtype=torch.int32, device="cuda")
                status = torch.empty(n, dtype=torch.uint8, device="cuda")

                def query():
                    return lzs.decompressed_sizes(slots, lens, None, size=size, status=status)

                line["size_ms"] = round(_event_ms(query, a.reps), 4)
                assert bool((size == length).all()) and bool((status == lzs.STATUS_END_MARKER).all())
            print(json.dumps(line), flush=True)
            del slots, lens
    if a.worker == "size":                                 # one block of 1 MiB of text alone: one lane's serial walk
        slots, lens = _compressed("text", 1, 1 << 20)
        size, _ = lzs.decompressed_sizes(slots, lens)
        ms = _event_ms(lambda: lzs.decompressed_sizes(slots, lens), a.reps)
        assert int(size.item()) == 1 << 20
        print(json.dumps({"tool": "size_scan_bench", "worker": "size", "class": "text", "workload": "one block of 1 MiB",
                          "blocks": 1, "raw": 1 << 20, "compressed_mb": round(int(lens.sum().item()) / 1e6, 3),
                          "size_ms": round(ms, 4), **device}), flush=True)


def _run_worker(kind, a, library):
    env = dict(os.environ)
    if library:
        env["LZS_LIBRARY"] = library
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--classes", a.classes, "--workloads", a.workloads,
           "--reps", str(a.reps)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.timeout)
    sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit(f"size_scan_bench: the {kind} worker failed with status {r.returncode}")
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--classes", default="text,lowent,random")
    ap.add_argument("--workloads", default="A,B")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--decoder-library", default="", help="the liblzs.so whose decoder is the yardstick (the parent commit's build)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "size_scan.txt"))
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--worker", choices=("size", "decode"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    dec = _run_worker("decode", a, a.decoder_library)
    siz = _run_worker("size", a, "")
    rows, lines = [], []
    for s in siz:
        d = next((d for d in dec if (d["class"], d["workload"]) == (s["class"], s["workload"])), None)
        line = dict(s)
        line.pop("worker")
        if d:
            line.update({"decode_ms": d["decode_ms"], "decoder_library": d["library"],
                         "decode_over_size": round(d["decode_ms"] / s["size_ms"], 2)})
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        rows.append(line)
    head = f"# tools/size_scan_bench.py, one session on {rows[0]['device']} ({rows[0]['cus']} CUs, {rows[0]['clock_mhz']} MHz): device events,\n" \
           f"# 2 warm-up calls, best of {a.reps}; decoder: {a.decoder_library or 'this tree (no --decoder-library)'}\n" \
           "# class   workload             blocks  compressed MB   size ms   decode ms   decode / size\n"
    table = ""
    for r in rows:
        table += f"# {r['class']:7s} {r['workload']:20s} {r['blocks']:6d} {r['compressed_mb']:14.2f} {r['size_ms']:9.4f} " \
                 f"{r.get('decode_ms', float('nan')):11.4f} {r.get('decode_over_size', float('nan')):15.2f}"
        table += "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(head + table + "\n".join(lines) + "\n")
    sys.stdout.write(head + table)


if __name__ == "__main__":
    main()
