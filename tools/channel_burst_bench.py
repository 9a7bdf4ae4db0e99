"""Many packets per channel in one call (include/lzs/lzs_channels.h, the burst calls) against ChannelCodec, which splits the
same batch into one call of the one-packet-per-channel entries per rank.  16 384 channels, 1500-byte packets of the device
generator's classes, three shapes of a drained queue:

    a   4 packets per channel, every channel (65 536 packets)
    b   65 536 packets with Zipf(1.1) channel ids
    c   one channel with 300 packets among 16 383 single packets

Wall time per call including host work (the ids live on the device: ChannelCodec fetches them to the host), GB/s of raw
bytes, and library calls (ChannelCodec: one per rank).  Both sides are checked against each other before timing.  Prints one
JSON line per class, shape and direction, and writes them to --out.

    python tools/channel_burst_bench.py --out profiles/r08/channel_burst.txt
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lzs_compression_amd as lzs  # noqa: E402
from lzs_compression_amd import api as A  # noqa: E402


def _ids(shape, nch, rng):
    if shape == "a":
        return np.tile(np.arange(nch), 4)
    if shape == "b":
        return (rng.zipf(1.1, 4 * nch) - 1) % nch
    return rng.permutation(np.concatenate([np.zeros(300, dtype=np.int64), np.arange(1, nch)]))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "channel_burst.txt"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    nch, P = a.channels, a.packet
    lines = []
    for cls in a.classes.split(","):
        for shape in a.shapes.split(","):
            rng = np.random.default_rng(1)
            ids = _ids(shape, nch, rng)
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

            def burst_d():
                return lzs.decompress_channels_burst(y, yl, ch, lzs.new_channel_states(nch), P)

            def codec_d():
                codec = lzs.ChannelCodec(nch)
                return codec.decompress(y, yl, ch.cpu().numpy(), P)

            back, want_d = burst_d(), codec_d()
            torch.cuda.synchronize()
            assert torch.equal(back[0][:, :P], x) and torch.equal(back[1], want_d[1]), f"{cls}/{shape}: decompress differs"
            for direction, fb, fc in (("compress", burst_c, codec_c), ("decompress", burst_d, codec_d)):
                tb, tc = _wall(fb, a.reps), _wall(fc, a.reps)
                line = {"tool": "channel_burst_bench", "class": cls, "shape": shape, "direction": direction, "packets": n,
                        "channels": nch, "packet": P, "ranks": ranks, "ratio": round(comp / (n * P), 4),
                        "burst_ms": round(tb * 1e3, 3), "burst_GBps": round(n * P / tb / 1e9, 2), "burst_calls": 1,
                        "codec_ms": round(tc * 1e3, 3), "codec_GBps": round(n * P / tc / 1e9, 2), "codec_calls": ranks,
                        "speedup": round(tc / tb, 2), "device": torch.cuda.get_device_name(0)}
                print(json.dumps(line), flush=True)
                lines.append(json.dumps(line))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
