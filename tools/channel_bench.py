"""Many channels, one packet each (include/lzs/lzs_channels.h): `channels` histories, `rounds` packets of `packet` bytes on each.
Channel c's packets are consecutive slices of block c of the device generator's class (lzs_compression_amd/workload.py), so
the history matters.  Prints one JSON line: compression (input GB/s, packets/s), decompression (output GB/s), the ratio, and
the same packets through the stateless lzs_compress_batch_device / lzs_decompress_batch_device beside them.

    python tools/channel_bench.py --cls text --channels 16384 --packet 1500 --rounds 8
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import lzs_compression_amd as lzs  # noqa: E402


def _timed(fn, reps):
    """Seconds of one fn() (the best of `reps`: each run fn() once between two events)."""
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t = a.elapsed_time(b) / 1e3
        best = t if best is None else min(best, t)
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cls", default="text", choices=["text", "lowent", "random"])
    ap.add_argument("--channels", type=int, default=16384)
    ap.add_argument("--packet", type=int, default=1500)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3, help="timed passes over all rounds (best kept)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    nch, P, R = a.channels, a.packet, a.rounds
    blocks = lzs.workload.fill_device(a.cls, nch, P * R)
    torch.cuda.synchronize()
    xs = [blocks[:, r * P:(r + 1) * P] for r in range(R)]          # round r: every channel's r-th packet (rows of stride P * R)
    cap = lzs.compressed_max(P)
    slot = (cap + 15) // 16 * 16
    outs = [torch.empty((nch, slot), dtype=torch.uint8, device="cuda") for _ in range(R)]
    lens = [torch.empty(nch, dtype=torch.int32, device="cuda") for _ in range(R)]
    status = torch.empty(nch, dtype=torch.uint8, device="cuda")
    back = torch.empty((nch, P), dtype=torch.uint8, device="cuda")
    back_len = torch.empty(nch, dtype=torch.int32, device="cuda")

    def channels_compress():
        states = lzs.new_channel_states(nch)                    # (a zeroed array: part of what a caller pays for fresh channels)
        for r in range(R):
            lzs.compress_channels(xs[r], None, None, states, out_capacity=cap, out=outs[r], out_len=lens[r], status=status)

    def channels_decompress():
        states = lzs.new_channel_states(nch)
        for r in range(R):
            lzs.decompress_channels(outs[r], lens[r], None, states, P, out=back, out_len=back_len, status=status)

    def blocks_compress():
        for r in range(R):
            lzs.compress_blocks(xs[r], None, out_capacity=cap, out=outs[r], out_len=lens[r])

    def blocks_decompress():
        for r in range(R):
            lzs.decompress_blocks(outs[r], lens[r], P, out=back, out_len=back_len)

    total = nch * P * R
    # correctness of what is timed: every packet comes back through the channel decoder, round by round
    channels_compress()
    states = lzs.new_channel_states(nch)
    for r in range(R):
        lzs.decompress_channels(outs[r], lens[r], None, states, P, out=back, out_len=back_len, status=status)
        torch.cuda.synchronize()
        assert torch.equal(back, xs[r]) and bool((back_len == P).all()) and bool(((status & 4) != 0).all()), f"round {r}: round trip"
    t_c = _timed(channels_compress, a.reps)
    comp_bytes = sum(int(l.sum().item()) for l in lens)
    t_d = _timed(channels_decompress, a.reps)
    t_bc = _timed(blocks_compress, a.reps)
    blk_bytes = sum(int(l.sum().item()) for l in lens)
    t_bd = _timed(blocks_decompress, a.reps)
    print(json.dumps({
        "tool": "channel_bench", "class": a.cls, "channels": nch, "packet": P, "rounds": R,
        "compress_GBps": round(total / t_c / 1e9, 2), "compress_packets_per_s": round(nch * R / t_c),
        "decompress_out_GBps": round(total / t_d / 1e9, 2), "ratio": round(comp_bytes / total, 4),
        "stateless_compress_GBps": round(total / t_bc / 1e9, 2), "stateless_decompress_out_GBps": round(total / t_bd / 1e9, 2),
        "stateless_ratio": round(blk_bytes / total, 4),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
