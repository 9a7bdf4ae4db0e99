#!/usr/bin/env python3
"""Wall time per call of the many-wavefront decompression's host paths, of the host-buffer batches and of the incremental
interface, this build against another build of liblzs.so.

    python tools/stream_host_ab.py --other path/to/other/liblzs.so [--reps 10] [--shapes dec-1m,dec-64m,dev-1g,batch-256] [--out FILE]

Shapes (text): dec-1m / dec-64m  lzs_decompress of a stream that decodes to 1 / 64 MiB, host buffers;
               dev-1g            lzs_decompress_stream_device of 1 GiB;
               comp-1m / comp-64m  lzs_compress of 1 / 64 MiB, host buffers (one stream in segments);
               cdev-1g           lzs_compress_stream_device of 1 GiB;
               batch-256        lzs_decompress_batch of 256 blocks of 64 KiB, host buffers (goes by segments);
               cbatch-2597 / dbatch-2597  lzs_compress_batch / lzs_decompress_batch of 2597 blocks of 64 KiB, host buffers
                                 (the overlapped route, lzs_pipeline.c);
               cbatch-64         lzs_compress_batch of 64 blocks of 64 KiB, host buffers (one after the other);
               inc-c-512 / inc-d-512  4 MiB through lzs_compress_incremental / lzs_decompress_incremental in calls of 512 bytes,
                                 LZS_ROUTE=device (every call a launch: the pinned box, the collecting);
               inc-c-1m          64 MiB through lzs_compress_incremental in pieces of 1 MiB;
               inc-d-256k        the stream of 24 MiB of tests/test_gpu_incremental.py's
                                 test_no_large_piece_is_left_to_one_wavefront in pieces of 256 KiB;
               inc-d-4m          40 MiB through lzs_decompress_incremental in pieces of 4 MiB (one "call" of these five is the
                                 whole stream, its block initialised first).
Every shape gets two worker processes -- one per build, chosen by LZS_LIBRARY, each with its data made, checked and three calls
warm -- and the two are timed in turn, one call each, `--reps` times: what one build sees of the machine the other sees too.
The verdict per shape: this build's median is no more than the other's median plus the other's own spread (max - min).
Exit code 1 if a shape misses that."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SHAPES = {"dec-1m": 16, "dec-64m": 1024, "dev-1g": 16384, "batch-256": 256,          # 64 KiB blocks of text
          "comp-1m": 16, "comp-64m": 1024, "cdev-1g": 16384,
          "cbatch-2597": 2597, "dbatch-2597": 2597, "cbatch-64": 64,
          "inc-c-512": 64, "inc-d-512": 64, "inc-c-1m": 1024, "inc-d-256k": 384, "inc-d-4m": 640}
INC_PIECE = {"inc-c-512": 512, "inc-d-512": 512, "inc-c-1m": 1 << 20, "inc-d-256k": 256 << 10, "inc-d-4m": 4 << 20}


def worker(shape):
    """Prepare, check, warm up; then one timed call per line read from stdin, its milliseconds on stdout."""
    sys.path.insert(0, ROOT)
    if shape.endswith("-512"):
        os.environ["LZS_ROUTE"] = "device"
    import numpy as np
    import lzs_compression_amd as lzs
    from lzs_compression_amd import workload
    L = lzs.lib()
    x = workload.fill("text", SHAPES[shape])
    if shape.startswith("cbatch-"):
        want, want_len = lzs.compress_batch(x)
        out, out_len = np.zeros_like(want), np.zeros(len(x), dtype=np.uint32)

        def call():
            assert L.lzs_compress_batch(out.ctypes.data, out.shape[1], out.shape[1], out_len.ctypes.data, x.ctypes.data, x.shape[1],
                                        None, x.shape[1], len(x)) == 0
        check = lambda: np.array_equal(out_len, want_len) and all(np.array_equal(out[b, :out_len[b]], want[b, :out_len[b]]) for b in range(len(x)))
    elif shape in ("batch-256", "dbatch-2597"):
        comp, lens = lzs.compress_batch(x)
        out, out_len = np.zeros_like(x), np.zeros(len(x), dtype=np.uint32)

        def call():
            assert L.lzs_decompress_batch(out.ctypes.data, out.shape[1], out.shape[1], out_len.ctypes.data, comp.ctypes.data,
                                          comp.shape[1], lens.ctypes.data, comp.shape[1], len(x)) == 0
        check = lambda: bool((out_len == x.shape[1]).all()) and np.array_equal(out, x)
    elif shape.startswith("inc-"):
        # (ctypes calls on buffers made beforehand, as tests/dev/inc_time.py drives the interface)
        from lzs_compression_amd import api
        if shape == "inc-d-256k":
            x = workload.fill("text", 1, 24 << 20, first_block=5)
        plain, piece, got, addr = x.tobytes(), INC_PIECE[shape], [0], ctypes.addressof
        if shape.startswith("inc-c-"):
            want, src, dst = lzs.compress(plain), ctypes.create_string_buffer(plain, len(plain)), ctypes.create_string_buffer(lzs.compressed_max(len(plain)) + 64)

            def call():
                p, out = api.CompressParameters(), 0
                L.lzs_compress_init_full(addr(p))
                p.outPtr, p.outLength = addr(dst), len(dst)
                for pos in range(0, len(plain), piece):
                    p.inPtr, p.inLength = addr(src) + pos, min(piece, len(plain) - pos)
                    out += L.lzs_compress_incremental(addr(p), False)
                    assert p.inLength == 0 and not (p.status & api.STATUS_ERROR)
                p.inLength = 0
                got[0] = out + L.lzs_compress_incremental(addr(p), True)
                assert p.status & api.STATUS_END_MARKER
            check = lambda: dst.raw[:got[0]] == want
        else:
            comp = lzs.compress(plain)
            src, dst = ctypes.create_string_buffer(comp, len(comp)), ctypes.create_string_buffer(len(plain) + 64)

            def call():
                p, out = api.DecompressParameters(), 0
                L.lzs_decompress_init(addr(p))
                p.outPtr, p.outLength = addr(dst), len(dst)
                for pos in range(0, len(comp), piece):
                    p.inPtr, p.inLength = addr(src) + pos, min(piece, len(comp) - pos)
                    while p.inLength:
                        out += L.lzs_decompress_incremental(addr(p))
                        assert not (p.status & api.STATUS_ERROR)
                got[0] = out
            check = lambda: got[0] == len(plain) and dst.raw[:len(plain)] == plain
    elif shape.startswith("comp-"):
        plain = x.reshape(-1)
        want = np.frombuffer(lzs.compress(plain.tobytes()), dtype=np.uint8)
        out, got = np.zeros(lzs.compressed_max(plain.size), dtype=np.uint8), [0]

        def call():
            got[0] = L.lzs_compress(out.ctypes.data, out.size, plain.ctypes.data, plain.size)
        check = lambda: got[0] == want.size and np.array_equal(out[:got[0]], want)
    elif shape == "cdev-1g":
        import torch
        plain = torch.from_numpy(x.reshape(-1)).cuda()
        want, want_len = lzs.compress_stream(plain)
        out, got = torch.empty_like(want), ctypes.c_size_t(0)
        torch.cuda.synchronize()

        def call():
            assert L.lzs_compress_stream_device(out.data_ptr(), out.numel(), ctypes.byref(got), plain.data_ptr(), plain.numel()) == 0
        check = lambda: got.value == want_len and bool(torch.equal(out[:got.value], want[:want_len]))
    elif shape == "dev-1g":
        import torch
        plain = torch.from_numpy(x.reshape(-1)).cuda()
        buf, nbytes = lzs.compress_stream(plain)
        comp, out, got = buf[:nbytes].clone(), torch.empty(plain.numel() + 64, dtype=torch.uint8, device="cuda"), ctypes.c_size_t(0)
        torch.cuda.synchronize()

        def call():
            assert L.lzs_decompress_stream_device(out.data_ptr(), out.numel(), ctypes.byref(got), comp.data_ptr(), comp.numel()) == 0
        check = lambda: got.value == plain.numel() and bool(torch.equal(out[:got.value], plain))
    else:
        import torch
        buf, nbytes = lzs.compress_stream(torch.from_numpy(x.reshape(-1)).cuda())
        comp = buf[:nbytes].cpu().numpy().copy()
        out, got = np.zeros(x.size + 64, dtype=np.uint8), [0]

        def call():
            got[0] = L.lzs_decompress(out.ctypes.data, out.size, comp.ctypes.data, comp.size)
        check = lambda: got[0] == x.size and np.array_equal(out[:x.size], x.reshape(-1))
    for _ in range(3):
        call()
    assert check(), f"{shape}: wrong result"
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        t = time.perf_counter()
        call()
        print(f"{(time.perf_counter() - t) * 1e3:.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--other", help="the liblzs.so to compare with")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", help="also write the report here")
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    assert a.other and os.path.exists(a.other), "--other: the build to compare with"
    lines, failed = [], False

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/stream_host_ab.py: this build against {os.path.basename(os.path.dirname(os.path.abspath(a.other)))}/{os.path.basename(a.other)}; "
        f"{a.reps} calls each, in turn, after 3 warm calls; ms a call")
    table = []
    for shape in a.shapes.split(","):
        procs = {}
        for who, so in (("other", os.path.abspath(a.other)), ("this", None)):
            env = {k: v for k, v in os.environ.items() if k != "LZS_LIBRARY"}
            if so:
                env["LZS_LIBRARY"] = so
            procs[who] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", shape], env=env, text=True,
                                          stdin=subprocess.PIPE, stdout=subprocess.PIPE)
        times = {"other": [], "this": []}
        try:
            for who, p in procs.items():
                line = p.stdout.readline().strip()
                assert line == "ready", f"{shape}: the worker of {who} build said {line!r}"
            for _ in range(a.reps):
                for who, p in procs.items():
                    p.stdin.write("go\n")
                    p.stdin.flush()
                    times[who].append(float(p.stdout.readline()))
        finally:
            for p in procs.values():
                p.stdin.close()
                p.wait(timeout=120)
        for who in ("other", "this"):
            say(f"{shape:12} {who:5} " + " ".join(f"{t:9.3f}" for t in times[who]))
        med = {w: statistics.median(times[w]) for w in times}
        spread = max(times["other"]) - min(times["other"])
        ok = med["this"] <= med["other"] + spread
        failed |= not ok
        table.append(f"{shape:12} {med['other']:12.3f} {min(times['other']):9.3f} {max(times['other']):9.3f} {med['this']:12.3f} {min(times['this']):9.3f} "
                     f"{max(times['this']):9.3f}   {'ok' if ok else 'SLOWER'} (this <= {med['other'] + spread:.3f})")
    say("")
    say(f"{'shape':12} {'other median':>12} {'min':>9} {'max':>9} {'this median':>12} {'min':>9} {'max':>9}   this median <= other median + (other max - min)")
    for row in table:
        say(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
