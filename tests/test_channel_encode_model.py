"""The plain CPU model of channel compression (oracle/lzs_oracle.c: lzs_oracle_compress_channel, the block rule on the view
[history | packet] with the first token at the border) held against everything else that states a part of the same rule: its own
brute-force form, the compiled reference's incremental compressor where it was built and digests minted from it where it was
not, the reference-made golden packets of one channel, the stateless oracle compressor, the model of channel decoding, the cut
law, and the library's own small-call codec (lzs_hostcodec.c through A.IncrementalCompressor under LZS_ROUTE=host).

The module is also the home of the generators and of the packet sets the GPU tests compress
(tests/test_gpu_channel_encode_model.py imports them).  Natural data rarely puts a winning match, a comparison or a refill on the
border between a channel's history and its packet, so histories and packets are built on purpose: packets spliced from pieces of
the history at view bytes 0 and 1 and at its last bytes, runs and periods that continue the history, long copies across the
border, history and view lengths on both sides of every size at which the kernels change path.
test_the_gpu_sets_reach_every_edge proves, here on the CPU, that those sets reach every edge the model counts; a later change to
a generator cannot silently empty a case."""
import ctypes
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

import oracle
from lzs_compression_amd import api as A
from conftest import golden_bytes, golden_json

O = oracle.oracle()
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "liblzs_ref.so")
WINDOW = 2047
DONE, CUT, ERROR = 0x07, 0x0B, A.STATUS_ERROR
HIST_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 2046, 2047)
PIECES = (2, 3, 8, 9, 22, 23, 24, 38)
SMALL_LENS = (0, 1, 2, 3, 7, 8, 9, 23)
VIEW_ENDS = (16, 32, 64, 128, 512, 1024, 2048, 4096)       # multiples of 16 and 64, the pool, the ring
MAX_PACKET = 9000


# ------------------------------------------------------------------ histories and packets, built on purpose
def make_history(rng, h, kind):
    """`h` bytes: random, over 2 or 3 symbols, one byte value, or random with a period-2 or period-3 tail."""
    if kind == "alpha2" or kind == "alpha3":
        return rng.choice(rng.integers(0, 256, int(kind[-1])), h).astype(np.uint8).tobytes()
    if kind == "uniform":
        return bytes([int(rng.integers(256))]) * h
    data = bytearray(rng.integers(0, 256, h, dtype=np.uint8).tobytes())
    if kind.startswith("period") and h:
        p = int(kind[-1])
        unit = rng.integers(0, 256, p, dtype=np.uint8).tobytes()
        tail = min(h, int(rng.integers(p, 40)))
        data[h - tail:] = (unit * (tail // p + 2))[-tail:] if tail else b""
    return bytes(data)


HIST_KINDS = ("random", "random", "random", "alpha2", "alpha3", "uniform", "period2", "period3")


def start_slots(rng, nch, bad=()):
    """Starting histories: the lengths of HIST_LENS in turn, the kinds of HIST_KINDS in turn; None for the channels in `bad` (their
    slot gets hist_len 4000: not a state)."""
    return [None if c in bad else make_history(rng, HIST_LENS[c % len(HIST_LENS)], HIST_KINDS[(c // len(HIST_LENS)) % len(HIST_KINDS)])
            for c in range(nch)]


def pick_length(rng, h):
    """A packet length for a history of `h` bytes: the small ones, one that ends the view 1 below, at or 1 above a multiple of
    16, 64, 512 or 4096, about 6000 bytes of view, or random (mostly short: every packet also goes through the brute finder)."""
    u = rng.random()
    if u < 0.2:
        return int(rng.choice(SMALL_LENS))
    if u < 0.45:
        end = int(rng.choice(VIEW_ENDS[:6])) + int(rng.integers(-1, 2))
        return end - h if end > h else int(rng.choice(SMALL_LENS))
    if u < 0.47:
        return int(rng.choice((2048, 4096))) + int(rng.integers(-1, 2)) - h
    if u < 0.475:
        return 6000 - h + int(rng.integers(-40, 40))
    if u < 0.49:
        return int(rng.choice((2046, 2047, 2048)))
    return int(rng.integers(0, 3001)) if u < 0.52 else int(rng.integers(0, 200))


def splice(rng, hist, n):
    """`n` bytes made of pieces of the view [hist | the packet so far]: each piece is read from a chosen place -- view bytes 0
    and 1, the history's last byte and last two bytes (such a piece runs on into the packet itself), or 127, 128 or 2047 bytes
    back -- with a fresh literal between two pieces or none."""
    h = len(hist)
    view = bytearray(hist)
    while len(view) - h < n:
        place = int(rng.integers(7))
        at = (0, 1, h - 1, h - 2, len(view) - 127, len(view) - 128, len(view) - WINDOW)[place]
        if h == 0 or at < 0 or len(view) - at > WINDOW:
            at = max(len(view) - WINDOW, 0) if h else -1
        if at < 0 or at >= len(view):
            view.append(int(rng.integers(256)))
            continue
        for i in range(int(rng.choice(PIECES))):
            view.append(view[at + i])
        if rng.random() < 0.5:
            view.append(int(rng.integers(256)))
    return bytes(view[h:h + n])


def make_packet(rng, hist, n, kind):
    """`n` bytes of the kind: "random"; "alpha2", "alpha3" (the symbols of the history's end, so that matches start there);
    "uniform"; "run" (the history's last byte, continued); "period2", "period3" (the history's last 2 or 3 bytes, continued);
    "splice"; "copy" (600 bytes or more from 300 bytes before the border: the source crosses it); "mixed" (random with runs
    and pieces in it)."""
    h = len(hist)
    if n == 0:
        return b""
    if kind in ("alpha2", "alpha3"):
        k = int(kind[-1])
        symbols = list(dict.fromkeys(hist[-64:]))[:k] or [int(v) for v in rng.integers(0, 256, k)]
        return bytes(rng.choice(symbols, n).astype(np.uint8))
    if kind == "uniform":
        return bytes([int(rng.integers(256))]) * n
    if kind == "run":
        return (hist[-1:] or b"r") * n
    if kind in ("period2", "period3"):
        p = int(kind[-1])
        unit = hist[-p:] if h >= p else rng.integers(0, 256, p, dtype=np.uint8).tobytes()
        return (unit * (n // p + 1))[:n]
    if kind == "splice":
        return splice(rng, hist, n)
    if kind == "copy" and h >= 2:
        back = min(h, 300)
        view = bytearray(hist)
        for i in range(n):
            view.append(view[h - back + i])
        return bytes(view[h:])
    if kind == "mixed":
        out = bytearray()
        while len(out) < n:
            u = rng.random()
            if u < 0.4:
                out += rng.integers(0, 256, int(rng.integers(1, 30)), dtype=np.uint8).tobytes()
            elif u < 0.6:
                out += bytes([int(rng.integers(256))]) * int(rng.choice((2, 8, 9, 23, 24, 40, 300)))
            else:
                out += splice(rng, (hist + bytes(out))[-WINDOW:], int(rng.integers(2, 60)))
        return bytes(out[:n])
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


PACKET_KINDS = ("splice", "splice", "splice", "random", "mixed", "mixed", "alpha2", "alpha3", "uniform", "run", "run", "period2",
                "period3", "copy")


def next_packet(rng, hist):
    """A packet for a channel whose history is `hist`: kind and length by chance, a copy across the border now and then."""
    kind = str(rng.choice(PACKET_KINDS))
    if kind == "copy":
        n = int(rng.integers(600, 1200)) if rng.random() < 0.3 else int(rng.integers(2, 200))
    else:
        n = pick_length(rng, len(hist))
    return make_packet(rng, hist, max(0, min(n, MAX_PACKET)), kind)


def advance(hist, packet):
    return (hist + packet)[-WINDOW:]


# ------------------------------------------------------------------ the model over a call
class Modelled:
    """What a call must give: per packet the stream (cut at the capacity), its uncut length, the status and the history it
    started from (None: ERROR); per channel the final history."""

    def __init__(self, outs, totals, status, before, hists):
        self.outs, self.totals, self.status, self.before, self.hists = outs, totals, status, before, hists


def run_model(packets, ids, hists, cap=None, counters=None, brute=False):
    """Compress `packets` in order, packet b on channel ids[b], each channel's history carried; every packet at `cap` (None: with
    room for all of it).  A channel whose history is None is no state, and an id >= len(hists) names no channel: those packets
    get ERROR and length 0, and nothing changes."""
    hists = list(hists)
    outs, totals, status, before = [], [], [], []
    for data, c in zip(packets, ids):
        h = hists[c] if 0 <= c < len(hists) else None
        before.append(h)
        if h is None:
            outs.append(b"")
            totals.append(0)
            status.append(ERROR)
            continue
        out, total, st, hists[c] = O.compress_channel(h, data, cap, brute, counters)
        outs.append(out)
        totals.append(total)
        status.append(st)
    return Modelled(outs, np.array(totals), np.array(status, dtype=np.uint8), before, hists)


class Scenario:
    """Rounds of packets on the same slots.  rounds: [(packets, ids)]; slots: starting histories (None: no state); caps: the
    capacities each round is compressed at (a history does not depend on the capacity, so every capacity starts each round from
    the same slots)."""

    def __init__(self, name, rounds, slots, caps):
        self.name, self.rounds, self.slots, self.caps = name, rounds, slots, caps

    @property
    def nch(self):
        return len(self.slots)

    def modelled(self, cap, counters=None, brute=False):
        """[Modelled] per round at `cap`, histories carried."""
        got, hists = [], self.slots
        for packets, ids in self.rounds:
            got.append(run_model(packets, ids, hists, cap, counters, brute))
            hists = got[-1].hists
        return got


def roomy(rounds):
    return A.compressed_max(max(max(len(p) for p in packets) for packets, _ in rounds))


def _fill_rounds(rng, slots, id_rounds):
    """[(packets, ids)] for the given ids: each channel's packets made one after the other, each for the history the ones before
    it leave (in row order within a round, and round after round)."""
    hists = list(slots)
    rounds = []
    for ids in id_rounds:
        packets = []
        for c in ids:
            h = hists[c] if 0 <= c < len(hists) else None
            if h is None:
                packets.append(rng.integers(0, 256, int(rng.integers(0, 100)), dtype=np.uint8).tobytes())
                continue
            packets.append(next_packet(rng, h))
            hists[c] = advance(h, packets[-1])
        rounds.append((packets, np.asarray(ids)))
    return rounds


CUT_CAP = 40          # the second capacity of every scenario: about half of the packets are longer


@functools.lru_cache(maxsize=None)
def single_scenario(n, seed=51):
    """The one-packet call: `n` packets on `n` channels (+ 3 idle ones), ids permuted, three rounds on the same slots; one slot is
    no state."""
    rng = np.random.default_rng([seed, n])
    nch = n + 3
    bad = (nch // 2,) if n > 1 else ()
    id_rounds = [rng.permutation(nch)[:n] for _ in range(3)]
    if bad and not any(bad[0] in ids for ids in id_rounds):
        id_rounds[0][0] = bad[0]
    slots = start_slots(rng, nch, bad)
    rounds = _fill_rounds(rng, slots, id_rounds)
    return Scenario(f"single{n}", rounds, slots, (roomy(rounds), CUT_CAP))


SINGLE_BATCHES = (1, 64, 257, 1500)


def _exact_run(rng, hist, total):
    """Packets for one channel: three whose lengths add up to exactly `total`, then three that see them as history."""
    a = int(rng.integers(1, total - 2))
    b = int(rng.integers(1, total - a))
    packets, h = [], hist
    for n in (a, b, total - a - b):
        packets.append(make_packet(rng, h, n, str(rng.choice(("random", "splice", "mixed")))))
        h = advance(h, packets[-1])
    for kind in ("splice", "copy", "run"):
        packets.append(make_packet(rng, h, int(rng.integers(30, 120)), kind))
        h = advance(h, packets[-1])
    return packets


@functools.lru_cache(maxsize=None)
def burst_scenario(seed=52, long_run=600, out_of_range=True):
    """Bursts: runs of 1, 2, 13 and `long_run` packets and random ones, ids interleaved; zero-length packets first, in the middle
    and last in a run; runs whose earlier packets total exactly 2046, 2047 and 2048 bytes behind a slot history of 2047 and of
    0 bytes; a slot that is no state and (`out_of_range`) ids that name no channel; two rounds on the same slots."""
    rng = np.random.default_rng(seed)
    nch, bad = 200, (77,)
    slots = start_slots(rng, nch, bad)
    for c in (4, 5, 6):
        slots[c] = make_history(rng, WINDOW, "random")        # kept only in part once the run's packets stand behind it
    for c in (7, 8, 9):
        slots[c] = b""
    hists = list(slots)
    rounds = []
    for r in range(2):
        per = {0: long_run, 1: 13, 2: 2, 3: 1, bad[0]: 13, 10: 13, 11: 13, 12: 13}
        for c in rng.integers(13, nch, 700):
            per[int(c)] = per.get(int(c), 0) + 1
        queue = {}
        for c, count in per.items():
            h, mine = hists[c], []
            for k in range(count):
                if h is None:
                    mine.append(rng.integers(0, 256, int(rng.integers(0, 100)), dtype=np.uint8).tobytes())
                    continue
                empty = (c == 10 and k == 0) or (c == 11 and k == 6) or (c == 12 and k == count - 1) or (c == 0 and k % 50 == 7)
                if c == 0:                                      # the long run: short packets, a slot's worth and more in all
                    p = b"" if empty else make_packet(rng, h, int(rng.integers(1, 24)), str(rng.choice(PACKET_KINDS[:-1])))
                else:
                    p = b"" if empty else next_packet(rng, h)
                mine.append(p)
                h = advance(h, p)
            queue[c], hists[c] = mine, h
        for c, total in zip((4, 5, 6, 7, 8, 9), (2046, 2047, 2048) * 2):
            queue[c] = _exact_run(rng, hists[c], total)
            for p in queue[c]:
                hists[c] = advance(hists[c], p)
        ids = np.concatenate([np.full(len(q), c) for c, q in queue.items()])
        if out_of_range:
            ids = np.concatenate([ids, np.full(6, nch), np.full(6, 0x7FFFFFFF), np.full(6, nch + 1000)])
        ids = rng.permutation(ids)
        taken = {c: 0 for c in queue}
        packets = []
        for c in ids:
            c = int(c)
            if c in queue:
                packets.append(queue[c][taken[c]])
                taken[c] += 1
            else:
                packets.append(rng.integers(0, 256, int(rng.integers(0, 100)), dtype=np.uint8).tobytes())
        rounds.append((packets, ids))
    return Scenario(f"burst{long_run}", rounds, slots, (roomy(rounds), CUT_CAP))


@functools.lru_cache(maxsize=None)
def one_byte_scenario(seed=53):
    """2100 packets of one byte on one channel, among the packets of 40 other channels: the history of the later ones is gathered
    from up to 2047 packets.  Then, on that channel, packets that copy what the one-byte packets left."""
    rng = np.random.default_rng(seed)
    nch = 41
    slots = start_slots(rng, nch)
    slots[0] = make_history(rng, 700, "random")
    h = slots[0]
    mine = []
    for k in range(2100):
        # a third of them repeat a piece of what stands 2047, 128 or 1 bytes back, so that the later ones have matches to find
        back = (WINDOW, 128, 1)[k % 3]
        mine.append(bytes([h[-back]]) if k % 3 != 1 and len(h) >= back else bytes([int(rng.integers(256))]))
        h = advance(h, mine[-1])
    for kind in ("splice", "copy", "run", "splice"):
        mine.append(make_packet(rng, h, 150, kind))
        h = advance(h, mine[-1])
    others = rng.integers(1, nch, 300)
    ids = np.concatenate([np.zeros(len(mine), dtype=np.int64), others])
    ids = rng.permutation(ids)
    hists = list(slots)
    packets, k = [], 0
    for c in ids:
        c = int(c)
        if c == 0:
            packets.append(mine[k])
            k += 1
        else:
            packets.append(next_packet(rng, hists[c])[:300])
            hists[c] = advance(hists[c], packets[-1])
    return Scenario("one byte", [(packets, ids)], slots, (roomy([(packets, ids)]), 1))


@functools.lru_cache(maxsize=None)
def uniform_scenario(length=100, n=257):
    """single_scenario(n) with every packet cut or filled up to `length` bytes: the call without a length array."""
    sc = single_scenario(n)
    rng = np.random.default_rng(54)
    hists, rounds = list(sc.slots), []
    for packets, ids in sc.rounds:
        same = []
        for p, c in zip(packets, ids):
            h = hists[c]
            same.append((p + (make_packet(rng, advance(h, p), length, "splice") if h is not None else bytes(length)))[:length])
            if h is not None:
                hists[c] = advance(h, same[-1])
        rounds.append((same, ids))
    return Scenario(f"uniform{length}", rounds, sc.slots, (A.compressed_max(length), CUT_CAP))


def gpu_scenarios():
    return [single_scenario(n) for n in SINGLE_BATCHES] + [burst_scenario(), burst_scenario(long_run=40, out_of_range=False),
                                                            one_byte_scenario(), uniform_scenario()]


def chosen_capacities(packets, hists):
    """[(packet index, capacity, place)] from the model: for a handful of the packets total - 1, total and total + 1, and one
    capacity inside the head of a match; and the capacities 0 and 1."""
    chosen = [(0, 0, "nothing"), (0, 1, "one byte")]
    picked = 0
    for b, (p, h) in enumerate(zip(packets, hists)):
        if h is None or len(p) < 20 or picked == 5:
            continue
        _, total, _, _, tokens = O.compress_channel(h, p, trace=True)
        heads = [t for t in tokens if t[1] and t[3] >= 16]
        if not heads:
            continue
        picked += 1
        chosen += [(b, total - 1, "total - 1"), (b, total, "total"), (b, total + 1, "total + 1")]
        chosen.append((b, int(heads[len(heads) // 2][3]) // 8 + 1, "inside a match head"))      # the head's bits go on past it
    return chosen


def digest(outs):
    """One SHA-256 over a round's lengths and streams."""
    d = hashlib.sha256()
    for out in outs:
        d.update(len(out).to_bytes(4, "little") + out)
    return d.hexdigest()


# ------------------------------------------------------------------ the model itself
@functools.lru_cache(maxsize=None)
def _modelled(name):
    sc = {s.name: s for s in gpu_scenarios()}[name]
    return sc.modelled(None)


def _all_rounds():
    for sc in gpu_scenarios():
        for r, ((packets, ids), m) in enumerate(zip(sc.rounds, _modelled(sc.name))):
            yield sc, r, packets, ids, m


def test_the_model_knows_the_rules():
    """Packets whose answers follow from the rule by hand."""
    C = O.compress_channel
    marker = bytes([0xC0, 0x00])
    assert C(b"", b"") == (marker, 2, DONE, b"") and C(b"abc", b"") == (marker, 2, DONE, b"abc")
    assert C(b"", b"", cap=1) == (marker[:1], 2, CUT, b"") and C(b"", b"", cap=2)[2] == DONE
    # "abc" after "xabc": one match at offset 3, length 3, then the marker: 1 1 0000011 01 | 1 1 0000000
    out, total, st, hist, tokens = C(b"xabc", b"abc", trace=True)
    assert tokens.tolist() == [[0, 3, 3, 0]] and out == int("11000001101" + "110000000" + "0000", 2).to_bytes(3, "big")
    assert (total, st, hist) == (3, DONE, b"xabcabc")
    # the nearest offset wins: "ab" stands 2 and 4 bytes back
    assert C(b"abab", b"ab", trace=True)[4].tolist() == [[0, 2, 2, 0]]
    # a run that continues the history's last byte: offset 1, 8 + 15 + 2, and the source crosses the border
    counters = np.zeros(len(oracle.CHANNEL_ENCODE_COUNTERS), dtype=np.uint64)
    out, total, st, hist, tokens = C(b"q", b"q" * 25, counters=counters, trace=True)
    assert tokens.tolist() == [[0, 1, 25, 0]] and hist == b"q" * 26
    got = dict(zip(oracle.CHANNEL_ENCODE_COUNTERS, counters.tolist()))
    assert got == dict(got, src_straddles=1, reaches_view_0=1, nibble_15=1, ext_ends_at_packet_end=1, first_token_offset_1=1,
                       src_in_history=0, cut=0, last_byte_literal=0)
    # offset 2047 to view byte 0, and one byte more of history puts it out of reach
    h = b"abcdefg" + bytes(2040)
    assert C(h, b"abcdefg", trace=True)[4].tolist() == [[0, 2047, 7, 0]]
    assert C(h[1:] + b"\0", b"abcdefg", trace=True)[4][:, 1].tolist() == [0] * 7       # "bcdefg" now stands 2048 back
    # a match is capped by the end of the packet, a single last byte is a literal
    assert C(b"abcdef", b"abcde", trace=True)[4].tolist() == [[0, 6, 5, 0]]
    assert C(b"abcdef", b"a", trace=True)[4].tolist() == [[0, 0, 1, 0]]


def test_chained_equals_brute_on_every_packet():
    for sc in gpu_scenarios():
        for r, (m, b) in enumerate(zip(_modelled(sc.name), sc.modelled(None, brute=True))):
            bad = [i for i in range(len(m.outs)) if m.outs[i] != b.outs[i]]
            assert not bad and (m.totals == b.totals).all() and m.hists == b.hists, (sc.name, r, bad[:5])


def test_empty_history_equals_the_stateless_oracle():
    seen = 0
    for sc, r, packets, ids, m in _all_rounds():
        for b in range(0, len(packets), 3):
            if m.before[b] is not None:
                out, total, st, hist = O.compress_channel(b"", packets[b])
                assert out == O.compress(packets[b]) and total == len(out) and st == DONE and hist == packets[b][-WINDOW:], (sc.name, r, b)
                seen += 1
    assert seen > 1000


def test_the_decoder_model_gives_the_packet_back():
    for sc, r, packets, ids, m in _all_rounds():
        for b, p in enumerate(packets):
            if m.before[b] is None:
                continue
            out, st, hist = O.decompress_channel(m.before[b], m.outs[b], len(p))
            assert out == p and st == 0x04, (sc.name, r, b, len(m.before[b]))
            assert hist == advance(m.before[b], p) == O.compress_channel(m.before[b], p)[3], (sc.name, r, b)
        for c, h in enumerate(m.hists):
            assert h is None or len(h) <= WINDOW


def test_cut_law():
    """At any capacity the bytes are a prefix of the uncut stream, the length is min(total, cap), the status says DONE exactly where
    total <= cap, and the history is that of the uncut packet."""
    rng = np.random.default_rng(55)
    seen = {DONE: 0, CUT: 0}
    for sc, r, packets, ids, m in _all_rounds():
        for b in range(r, len(packets), 7):
            h = m.before[b]
            if h is None:
                continue
            full, total = m.outs[b], int(m.totals[b])
            assert len(full) == total
            for cap in (0, 1, total - 1, total, total + 1, int(rng.integers(0, total + 1))):
                out, t, st, hist = O.compress_channel(h, packets[b], cap)
                assert out == full[:cap] and t == total and len(out) == min(total, cap), (sc.name, r, b, cap)
                assert st == (DONE if total <= cap else CUT) and hist == advance(h, packets[b]), (sc.name, r, b, cap)
                seen[st] += 1
    assert min(seen.values()) > 1000, seen


def test_golden_packets_of_one_channel():
    """The reference's lzs_compress_incremental() wrote inc_packets.lzs for the three packets on one parameter block."""
    hist, streams = b"", []
    for i in range(3):
        out, total, st, hist = O.compress_channel(hist, golden_bytes(f"inc_packet_{i}.bin"), brute=bool(i % 2))
        assert st == DONE and total == len(out)
        streams.append(out)
    assert b"".join(streams) == golden_bytes("inc_packets.lzs")


class RefCompressor:
    """The compiled reference's own parameter block (oracle/_ref/liblzs_ref.so), one a channel."""
    REF = None

    def __init__(self):
        if RefCompressor.REF is None:
            R = ctypes.CDLL(REF_SO)
            R.lzs_compress_init_full.restype, R.lzs_compress_init_full.argtypes = None, [ctypes.c_void_p]
            R.lzs_compress_incremental.restype = ctypes.c_size_t
            R.lzs_compress_incremental.argtypes = [ctypes.c_void_p, ctypes.c_bool]
            RefCompressor.REF = R
        self.p = A.CompressParameters()
        RefCompressor.REF.lzs_compress_init_full(ctypes.addressof(self.p))

    def step(self, data):
        out, pending = bytearray(), data
        while True:
            src = ctypes.create_string_buffer(pending, max(len(pending), 1))
            room = A.compressed_max(len(data)) + 16
            dst = ctypes.create_string_buffer(room)
            self.p.inPtr, self.p.inLength, self.p.outPtr, self.p.outLength = ctypes.addressof(src), len(pending), ctypes.addressof(dst), room
            n = RefCompressor.REF.lzs_compress_incremental(ctypes.addressof(self.p), True)
            out += dst.raw[:n]
            pending = pending[len(pending) - self.p.inLength:]
            if self.p.status & A.STATUS_END_MARKER:
                return bytes(out)


class HostCompressor:
    """The library's small-call codec (LZS_ROUTE=host), one parameter block a channel."""

    def __init__(self):
        self.c = A.IncrementalCompressor()

    def step(self, data):
        got, used, status = self.c.step(data, A.compressed_max(len(data)) + 16, add_end_marker=True)
        assert used == len(data) and status & A.STATUS_END_MARKER
        return got


def through_parameter_blocks(sc, make):
    """The scenario through one incremental compressor a channel: [[stream per packet] per round], None where the model says
    ERROR.  A parameter block starts empty, so a channel's starting history is fed to it first, as a packet of its own."""
    blocks = {}
    rounds = []
    for (packets, ids), m in zip(sc.rounds, _modelled(sc.name)):
        streams = []
        for b, (p, c) in enumerate(zip(packets, ids)):
            if m.before[b] is None:
                streams.append(None)
                continue
            if c not in blocks:
                blocks[c] = make()
                if sc.slots[c]:
                    blocks[c].step(sc.slots[c])
            streams.append(blocks[c].step(p))
        rounds.append(streams)
    return rounds


def _compare_with_blocks(make, who):
    n = 0
    for sc in gpu_scenarios():
        for r, (streams, m) in enumerate(zip(through_parameter_blocks(sc, make), _modelled(sc.name))):
            for b, s in enumerate(streams):
                if s is not None and s != m.outs[b]:
                    tokens = O.compress_channel(m.before[b], sc.rounds[r][0][b], trace=True)[4]
                    k = next((i for i in range(min(len(s), len(m.outs[b]))) if s[i] != m.outs[b][i]), min(len(s), len(m.outs[b])))
                    at = [t.tolist() for t in tokens if t[3] <= 8 * k + 7][-1:]
                    raise AssertionError(f"{who}: {sc.name}, round {r}, packet {b}, channel {sc.rounds[r][1][b]}, hlen {len(m.before[b])}, "
                                         f"{len(sc.rounds[r][0][b])} bytes: {len(s)} bytes (model {len(m.outs[b])}), first differing byte {k}; "
                                         f"model token there [pos, offset, length, bit] {at}")
                n += s is not None
    return n


def test_the_compiled_references_incremental_compressor_live():
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref/liblzs_ref.so was not built")
    assert _compare_with_blocks(RefCompressor, "the reference") > 5000


def test_the_librarys_host_codec(monkeypatch):
    """lzs_hostcodec.c is product code that runs without a device: A.IncrementalCompressor under LZS_ROUTE=host, one a channel."""
    monkeypatch.setenv("LZS_ROUTE", "host")
    assert _compare_with_blocks(HostCompressor, "LZS_ROUTE=host") > 5000


def test_reference_digests():
    """tests/golden/channel_encode_digests.json (make_channel_encode_digests.py: the compiled reference's incremental compressor
    on the same scenarios) keeps the model pinned where the reference did not travel."""
    want = golden_json("channel_encode_digests.json")
    got = {sc.name: [digest(m.outs) for m in _modelled(sc.name)] for sc in gpu_scenarios()}
    assert got == want, [name for name in got if got[name] != want.get(name)]


def test_the_gpu_sets_reach_every_edge():
    """A condition on the inputs of tests/test_gpu_channel_encode_model.py: over its scenarios and capacities every counter of the
    model is reached at least 20 times, each of the two statuses at least 100 times and ERROR at least 20 times."""
    counters = np.zeros(len(oracle.CHANNEL_ENCODE_COUNTERS), dtype=np.uint64)
    status = {DONE: 0, CUT: 0, ERROR: 0}
    npackets = 0
    for sc in gpu_scenarios():
        for cap in sc.caps:
            for m in sc.modelled(cap, counters):
                npackets += len(m.outs)
                for st in m.status:
                    status[int(st)] += 1
    print(dict(zip(oracle.CHANNEL_ENCODE_COUNTERS, counters.tolist())), status, npackets)
    assert (counters >= 20).all(), dict(zip(oracle.CHANNEL_ENCODE_COUNTERS, counters.tolist()))
    assert min(status[DONE], status[CUT]) >= 100 and status[ERROR] >= 20, status
    sc = single_scenario(64)
    places = {place for _, _, place in chosen_capacities(sc.rounds[0][0], _modelled(sc.name)[0].before)}
    assert len(places) == 6, places
    # the scenarios keep to the sizes the GPU tests can afford
    for sc in gpu_scenarios():
        for packets, ids in sc.rounds:
            assert len(packets) <= 2500 and max(len(p) for p in packets) <= MAX_PACKET, sc.name
    # the burst scenario holds what its name promises
    sc = burst_scenario()
    for packets, ids in sc.rounds:
        runs = {int(c): [len(p) for p, i in zip(packets, ids) if i == c] for c in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)}
        assert [len(runs[c]) for c in (0, 1, 2, 3)] == [600, 13, 2, 1]
        assert [sum(runs[c][:3]) for c in (4, 5, 6, 7, 8, 9)] == [2046, 2047, 2048] * 2
        assert runs[10][0] == 0 and runs[11][6] == 0 and runs[12][-1] == 0 and min(runs[0]) == 0
        assert (ids >= sc.nch).sum() == 18


def test_the_standalone_sanitizer_program(tmp_path):
    """oracle/channel_encode_san.c: the model under AddressSanitizer and UndefinedBehaviorSanitizer in a program of its own (no
    runtime is preloaded into anything): chained == brute and the round trip through lzs_oracle_decompress_channel."""
    exe = tmp_path / "channel_encode_san"
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "san-program", f"SAN_PROGRAM={exe}"], check=True,
                   stdout=subprocess.DEVNULL)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 failure(s)" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
