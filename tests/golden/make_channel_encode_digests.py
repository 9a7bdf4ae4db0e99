#!/usr/bin/env python3
"""Mint channel_encode_digests.json from the REAL reference (oracle/_ref/liblzs_ref.so, built by `make -C oracle ref`; build
container only): the scenarios of tests/test_channel_encode_model.py through the reference's lzs_compress_incremental(), one
parameter block a channel (its starting history fed first, as a packet of its own), every packet finished with an end marker.

  channel_encode_digests.json   {scenario: [one SHA-256 per round over every packet's length and stream]}; a packet that the
                                channel calls answer with ERROR (no state, no such channel) counts with length 0

Results only: the packets themselves are made again, from their seeds, by whoever checks against the digests.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_channel_encode_model as M  # noqa: E402


def main():
    digests = {}
    for sc in M.gpu_scenarios():
        rounds = M.through_parameter_blocks(sc, M.RefCompressor)
        digests[sc.name] = [M.digest([s or b"" for s in streams]) for streams in rounds]
        print(sc.name, [len(streams) for streams in rounds])
    with open(os.path.join(HERE, "channel_encode_digests.json"), "w") as f:
        json.dump(digests, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
