"""History resets inside a burst (lzs_*_channels_burst*_flags_device): what a reset costs and what it buys, and
whether the calls without flags pay for it.  One MI355X, device events around one call, two warm-up calls, the best of --reps; every
measurement is made --spread times in its process and given as lowest - highest.  Each worker process runs under its own time limit.

    resets   4096 text packets of 1500 bytes, both directions:
               (a) all on one channel, no flags          (the decoder: one run of 4096 -- with the plain work area one decoder stream,
                                                          with the split-size area PARSE + RESOLVE)
               (b) the same, every packet flagged        (4096 runs of one packet)
               (c) the same packets on 4096 channels, through the entries without flags of --parent-library: the yardstick for (b)
    rows     the burst calls without flags on the queues of DESIGN.md 3.11 (16 384 channels: a = 4 packets a channel, b = Zipf(1.1),
             c = 1 x 300 + 16 383 x 1), strided (1500-byte packets; the decoder with the plain and with the split-size work area) and
             packed (40 to 1500 bytes), with --parent-library and with this tree: the same rows from both builds.  The parent's
             build is measured in --parent-runs processes of its own, one after the other: their lowest and highest best-of are
             the run-to-run spread this tree's figures are read against

    python tools/burst_reset_bench.py --parent-library /path/to/parent/liblzs.so --out profiles/r22/burst_reset.txt
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

P, LO = 1500, 40


def _event_ms(fn, reps, warmup=2):
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


def _times(fn, a):
    return [round(_event_ms(fn, a.reps), 4) for _ in range(a.spread)]


def _ids(shape, nch, rng):
    import numpy as np
    if shape == "a":
        return np.tile(np.arange(nch), 4)
    if shape == "b":
        return (rng.zipf(1.1, 4 * nch) - 1) % nch
    return rng.permutation(np.concatenate([np.zeros(300, dtype=np.int64), np.arange(1, nch)]))


def _emit(a, **line):
    print(json.dumps({"tool": "burst_reset_bench", "worker": a.worker, "library": os.environ.get("LZS_LIBRARY", "this tree"), **line}), flush=True)


def resets(a):
    """Rows (a), (b), (c); with a parent library only (c), the rest needs the flags entries."""
    import torch
    import lzs_compression_amd as lzs
    n = a.packets
    new = hasattr(lzs.lib(), "lzs_compress_channels_burst_flags_device")
    x = lzs.workload.fill_device("text", n, P)
    one, many = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.arange(n, dtype=torch.int32, device="cuda")
    flags = torch.full((n,), 1, dtype=torch.uint8, device="cuda")
    cap = lzs.compressed_max(P)
    out = torch.empty((n, (cap + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
    out_len, status = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    back = torch.empty((n, (P + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
    small = torch.empty(lzs.channels_burst_work_bytes(n, n), dtype=torch.uint8, device="cuda")
    large = torch.empty(lzs.channels_burst_split_work_bytes(n, n, P), dtype=torch.uint8, device="cuda")
    cases = [("c", many, None, n)] + ([("a", one, None, 1), ("b", one, flags, 1)] if new else [])
    for row, ch, fl, nch in cases:
        states = lzs.new_channel_states(nch)
        kw = {} if fl is None else {"flags": fl}

        def compress():
            states.zero_()
            lzs.compress_channels_burst(x, None, ch, states, cap, out=out, out_len=out_len, status=status, work=small, **kw)

        t = _times(compress, a)
        assert bool((status == 0x07).all())
        y, yl = out.clone(), out_len.clone()
        _emit(a, row=row, direction="compress", packets=n, channels=nch, flagged=fl is not None, ms=t, compressed_mb=round(int(yl.sum()) / 1e6, 3))
        for area, work in (("plain", small), ("split", large)):
            def decompress():
                states.zero_()
                lzs.decompress_channels_burst(y, yl, ch, states, P, out=back, out_len=out_len, status=status, work=work, **kw)

            t = _times(decompress, a)
            assert torch.equal(back[:, :P], x) and bool((status == lzs.STATUS_END_MARKER).all())
            _emit(a, row=row, direction="decompress", work_area=area, packets=n, channels=nch, flagged=fl is not None, ms=t)


def rows(a):
    """The burst calls without flags on the queues of DESIGN.md 3.11, strided and packed."""
    import numpy as np
    import torch
    import lzs_compression_amd as lzs
    nch = a.channels
    for cls in a.classes.split(","):
        for shape in a.shapes.split(","):
            ids = _ids(shape, nch, np.random.default_rng(1))
            n = ids.size
            x = lzs.workload.fill_device(cls, n, P)
            ch = torch.from_numpy(ids.astype(np.int32)).cuda()
            states = lzs.new_channel_states(nch)
            cap = lzs.compressed_max(P)
            out = torch.empty((n, (cap + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
            out_len, status = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
            small = torch.empty(lzs.channels_burst_work_bytes(n, nch), dtype=torch.uint8, device="cuda")

            def compress():
                states.zero_()
                lzs.compress_channels_burst(x, None, ch, states, cap, out=out, out_len=out_len, status=status, work=small)

            t = _times(compress, a)
            _emit(a, form="strided", cls=cls, shape=shape, direction="compress", packets=n, ms=t)
            y, yl = out.clone(), out_len.clone()
            back = torch.empty((n, (P + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
            large = torch.empty(lzs.channels_burst_split_work_bytes(n, nch, P), dtype=torch.uint8, device="cuda")
            for area, work in (("plain", small), ("split", large)):
                def decompress():
                    states.zero_()
                    lzs.decompress_channels_burst(y, yl, ch, states, P, out=back, out_len=out_len, status=status, work=work)

                t = _times(decompress, a)
                assert torch.equal(back[:, :P], x)
                _emit(a, form="strided", cls=cls, shape=shape, direction="decompress", work_area=area, packets=n, ms=t)
            del out, y, back, large
            # packed: lengths of 40 to 1500 bytes, the rooms of the bounds at 16, decoded into rooms of exactly the sizes
            g = torch.Generator(device="cpu").manual_seed(n + LO)
            raw_len = torch.randint(LO, P + 1, (n,), generator=g, dtype=torch.int32).cuda()
            keep = torch.arange(P, device="cuda")[None, :] < raw_len[:, None]
            flat = x[keep]
            in_off = lzs.offsets_from_sizes(raw_len, 1)
            room_off = lzs.offsets_from_sizes(lzs.compressed_bounds_packed(in_off), 16)
            rooms = torch.empty(int(room_off[-1].item()), dtype=torch.uint8, device="cuda")
            offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            dense = torch.empty(rooms.numel(), dtype=torch.uint8, device="cuda")

            def compress_packed():
                states.zero_()
                lzs.compress_channels_burst_packed(flat, in_off, ch, states, rooms, room_off, out_len=out_len, status=status, work=small)

            t = _times(compress_packed, a)
            _emit(a, form="packed", cls=cls, shape=shape, direction="compress", packets=n, ms=t)
            lzs.compact_packed(rooms, room_off, out_len, dense=dense, offsets=offsets)
            comp = int(offsets[-1].item())
            y, y_off = dense[:comp].clone(), offsets.clone()
            del rooms, dense
            back = torch.empty(flat.numel(), dtype=torch.uint8, device="cuda")
            large = torch.empty(lzs.channels_burst_packed_split_work_bytes(n, nch, flat.numel()), dtype=torch.uint8, device="cuda")

            def decompress_packed():
                states.zero_()
                lzs.decompress_channels_burst_packed(y, y_off, ch, states, back, in_off, out_len=out_len, status=status, work=large)

            t = _times(decompress_packed, a)
            assert torch.equal(out_len, raw_len) and torch.equal(back, flat)
            _emit(a, form="packed", cls=cls, shape=shape, direction="decompress", work_area="split", packets=n, ms=t)
            del back, large, y, flat


def _run_worker(kind, a, library):
    env = dict(os.environ)
    env.pop("LZS_LIBRARY", None)
    if library:
        env["LZS_LIBRARY"] = library
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--classes", a.classes, "--shapes", a.shapes, "--channels", str(a.channels),
           "--packets", str(a.packets), "--reps", str(a.reps), "--spread", str(a.spread)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.timeout)
    sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        raise SystemExit(f"burst_reset_bench: the {kind} worker ({library or 'this tree'}) ended with status {r.returncode}")
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--channels", type=int, default=16384)
    ap.add_argument("--packets", type=int, default=4096)
    ap.add_argument("--classes", default="text,lowent,random")
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spread", type=int, default=3)
    ap.add_argument("--parent-library", required=False, default="", help="the liblzs.so of the parent commit")
    ap.add_argument("--parent-runs", type=int, default=3, help="processes that measure the parent's build for `rows`")
    ap.add_argument("--parts", default="resets,rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "burst_reset.txt"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds, for each worker process")
    ap.add_argument("--worker", choices=("resets", "rows"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        import torch
        import lzs_compression_amd as lzs
        torch.cuda.set_device(0)
        lzs.backend_info()
        return resets(a) if a.worker == "resets" else rows(a)
    if not a.parent_library:
        raise SystemExit("burst_reset_bench: --parent-library is the yardstick; build the parent commit's liblzs.so and name it")
    text = f"# tools/burst_reset_bench.py: device events, 2 warm-up calls, best of {a.reps}, each measured {a.spread} times (low - high), ms\n"
    lines = []
    if "resets" in a.parts.split(","):
        got = _run_worker("resets", a, a.parent_library) + _run_worker("resets", a, "")
        lines += got
        text += f"# {a.packets} text packets of {P} bytes.  (a) one channel, no flags; (b) one channel, every packet flagged; (c) {a.packets} channels, no flags\n"
        text += "# row direction   work area  library      low - high\n"
        for g in got:
            lib = "this tree" if g["library"] == "this tree" else "parent"
            text += f"# ({g['row']}) {g['direction']:10s}  {g.get('work_area', '-'):9s}  {lib:10s} {min(g['ms']):9.4f} - {max(g['ms']):7.4f}\n"
    if "rows" in a.parts.split(","):
        olds = [_run_worker("rows", a, a.parent_library) for _ in range(a.parent_runs)]
        new = _run_worker("rows", a, "")
        old = [dict(o[0], ms=[t for run in o for t in run["ms"]]) for o in zip(*olds)]
        lines += old + new
        text += f"# the calls without flags, {a.channels} channels: the parent's build in {a.parent_runs} processes, this tree in one; outside: this tree's lowest above the parent's highest\n"
        text += "# form    class   shape direction   work area     parent low - high      this tree low - high   outside the parent's spread\n"
        for o, s in zip(old, new):
            assert all(o[k] == s[k] for k in ("form", "cls", "shape", "direction"))
            text += f"# {o['form']:7s} {o['cls']:7s} {o['shape']:5s} {o['direction']:10s}  {o.get('work_area', '-'):9s} {min(o['ms']):9.4f} - {max(o['ms']):7.4f}   " \
                    f"{min(s['ms']):9.4f} - {max(s['ms']):7.4f}   {'yes' if min(s['ms']) > max(o['ms']) else 'no'}\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n".join(json.dumps(g) for g in lines) + "\n")
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
