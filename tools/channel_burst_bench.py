"""Many packets per channel in one call (include/lzs/lzs_channels.h, the burst calls) against ChannelCodec, which splits the
same batch into one call of the one-packet-per-channel entries per rank.  16 384 channels, 1500-byte packets of the device
generator's classes, three shapes of a drained queue:

    a   4 packets per channel, every channel (65 536 packets)
    b   65 536 packets with Zipf(1.1) channel ids
    c   one channel with 300 packets among 16 383 single packets

Wall time per call including host work (the ids live on the device: ChannelCodec fetches them to the host), GB/s of raw
bytes, and library calls (ChannelCodec: one per rank).  Both sides are checked against each other before timing.  Prints one
JSON line per class, shape and direction, and writes them to --out.

The decoder is timed twice: with a work area of lzs_channels_burst_work_bytes() (burst_ms: one decoder stream a run) and with
one of lzs_channels_burst_split_work_bytes() (split_ms: long runs split over the device).  --sweep times both
on queues of shape c with a long run of 2 ... 300 packets, the threshold set so that only that run is split: where the
default of LZS_BURST_SPLIT_MIN comes from.  LZS_LIBRARY=<an older liblzs.so> gives that build's figures (no split there).

    python tools/channel_burst_bench.py --out profiles/r09/channel_burst_split.txt
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("LZS_DEV_ENV", "1")          # --sweep sets LZS_BURST_SPLIT_MIN between calls

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lzs_compression_amd as lzs  # noqa: E402
from lzs_compression_amd import api as A  # noqa: E402


def _ids(shape, nch, rng, run=300):
    if shape == "a":
        return np.tile(np.arange(nch), 4)
    if shape == "b":
        return (rng.zipf(1.1, 4 * nch) - 1) % nch
    return rng.permutation(np.concatenate([np.zeros(run, dtype=np.int64), np.arange(1, nch)]))


def _wall(fn, reps):
    """Seconds of one fn() ending in a device synchronise (the best of `reps`, after one untimed call)."""
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--channels", type=int, default=16384)
    ap.add_argument("--packet", type=int, default=1500)
    ap.add_argument("--classes", default="text,lowent,random")
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "channel_burst_split.txt"))
    ap.add_argument("--no-codec", action="store_true", help="do not time ChannelCodec (checked against it all the same)")
    ap.add_argument("--sweep", action="store_true", help="shape c with a long run of 2 ... 300 packets, decoder only, both routes")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    nch, P = a.channels, a.packet
    lines = []
    has_split = hasattr(lzs.lib(), "lzs_channels_burst_split_work_bytes")
    cases = [(cls, shape, 300) for cls in a.classes.split(",") for shape in a.shapes.split(",")]
    if a.sweep:
        cases = [(cls, "c", run) for cls in a.classes.split(",") for run in (2, 3, 4, 6, 8, 12, 16, 32, 64, 128, 300)]
    if True:
        for cls, shape, run in cases:
            rng = np.random.default_rng(1)
            ids = _ids(shape, nch, rng, run)
            n = ids.size
            x = lzs.workload.fill_device(cls, n, P)             # packet b: block b of the class (no history shared by design)
            ch = torch.from_numpy(ids.astype(np.int32)).cuda()
            ranks = int(A._occurrence_rank(ids).max()) + 1
            cap = lzs.compressed_max(P)
            torch.cuda.synchronize()

            def burst_c():
                return lzs.compress_channels_burst(x, None, ch, lzs.new_channel_states(nch), out_capacity=cap)

            def codec_c():
                codec = lzs.ChannelCodec(nch)
                return codec.compress(x, None, ch.cpu().numpy(), out_capacity=cap)

            got, want = burst_c(), codec_c()
            torch.cuda.synchronize()
            assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), f"{cls}/{shape}: compress differs"
            y, yl = got[0], got[1]
            comp = int(yl.sum().item())

            small = torch.empty(lzs.channels_burst_work_bytes(n, nch), dtype=torch.uint8, device="cuda")
            large = torch.empty(lzs.channels_burst_split_work_bytes(n, nch, P), dtype=torch.uint8, device="cuda")
            if a.sweep:                                         # only the long run is split: the others are one packet each
                os.environ["LZS_BURST_SPLIT_MIN"] = str(int(yl[ch != 0].max().item()) + 1)

            def burst_d():
                return lzs.decompress_channels_burst(y, yl, ch, lzs.new_channel_states(nch), P, work=small)

            def split_d():
                return lzs.decompress_channels_burst(y, yl, ch, lzs.new_channel_states(nch), P, work=large)

            def codec_d():
                codec = lzs.ChannelCodec(nch)
                return codec.decompress(y, yl, ch.cpu().numpy(), P)

            back, want_d = burst_d(), codec_d()
            torch.cuda.synchronize()
            assert torch.equal(back[0][:, :P], x) and torch.equal(back[1], want_d[1]), f"{cls}/{shape}: decompress differs"
            back = split_d()
            torch.cuda.synchronize()
            assert torch.equal(back[0][:, :P], x) and torch.equal(back[1], want_d[1]) and torch.equal(back[2], want_d[2]), \
                f"{cls}/{shape}: decompress with the larger work area differs"
            for direction, fb, fc in (("compress", burst_c, codec_c), ("decompress", burst_d, codec_d)):
                if a.sweep and direction == "compress":
                    continue
                tb = _wall(fb, a.reps)
                line = {"tool": "channel_burst_bench", "class": cls, "shape": shape, "direction": direction, "packets": n,
                        "channels": nch, "packet": P, "ranks": ranks, "ratio": round(comp / (n * P), 4),
                        "burst_ms": round(tb * 1e3, 3), "burst_GBps": round(n * P / tb / 1e9, 2), "burst_calls": 1,
                        "device": torch.cuda.get_device_name(0)}
                if direction == "decompress" and has_split:
                    ts = _wall(split_d, a.reps)
                    line.update({"split_ms": round(ts * 1e3, 3), "split_GBps": round(n * P / ts / 1e9, 2),
                                 "split_speedup": round(tb / ts, 2)})
                if not a.no_codec and not a.sweep:
                    tc = _wall(fc, a.reps)
                    line.update({"codec_ms": round(tc * 1e3, 3), "codec_GBps": round(n * P / tc / 1e9, 2), "codec_calls": ranks,
                                 "speedup": round(tc / tb, 2)})
                if a.sweep:
                    line.update({"long_run": run, "split_min": int(os.environ["LZS_BURST_SPLIT_MIN"])})
                print(json.dumps(line), flush=True)
                lines.append(json.dumps(line))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
