"""What the tests of history resets inside a burst share (include/lzs/lzs_channels.h, LZS_PACKET_RESET): the rule
as a plain loop over a queue, generated queues of flagged packets, and a report of what each queue reaches.  No device code: the
queues and every expected value come from the CPU models (oracle.oracle().compress_channel / decompress_channel);
tests/test_burst_flags_cases.py holds the rule to its rank-by-rank definition and the queues to the edges they are meant to reach,
tests/test_gpu_burst_flags.py and tests/test_gpu_burst_flags_queues.py run them on the device."""
import functools

import numpy as np

import lzs_compression_amd as lzs
from lzs_compression_amd import api as A

import test_channel_model as M
from test_channel_model import O

SLOT, HIST_AT = A.CHANNEL_STATE_BYTES, 64
PATTERNS = ("distinct", "uniform4", "zipf", "one300", "tiny", "pairs", "two", "three")
DENSITIES = ("sparse", "quarter", "all", "first_only", "last_only", "not_first")
JUNK = b"\x01\x02\x03"                   # a decoder packet where the compressor model gave none (ERROR): never decoded


# ------------------------------------------------------------------ the rule
def _apply_rule(step, ids, flags, hists, skip=()):
    """The rule of the header over a queue: packet b on channel ids[b]; a flag on a block of a channel in range empties the
    history first.  step(b, hist) -> (bytes, status, new history).  Returns (outs, status, final histories, touched channels)."""
    hists = list(hists)
    outs, status, touched = [], [], set()
    for b, c in enumerate(ids):
        if not 0 <= c < len(hists) or b in skip:
            outs.append(b"")
            status.append(A.STATUS_ERROR)
            continue
        if flags[b] & 1:
            hists[c] = b""
        if hists[c] is None:
            outs.append(b"")
            status.append(A.STATUS_ERROR)
            continue
        out, st, hists[c] = step(b, hists[c])
        touched.add(c)
        outs.append(out)
        status.append(st)
    return outs, np.array(status, dtype=np.uint8), hists, touched


def _want_slots(before, hists, touched):
    """A committed channel has its hist_len and all of hist[] rewritten, the reserved bytes as they were; the others are untouched."""
    want = before.copy()
    for c in touched:
        h = hists[c]
        want[c, :4] = np.frombuffer(len(h).to_bytes(4, "little"), dtype=np.uint8)
        want[c, HIST_AT:] = 0
        want[c, HIST_AT:HIST_AT + len(h)] = np.frombuffer(h, dtype=np.uint8)
    return want


def _check_slots(tag, states, want):
    s = states.cpu().numpy()
    rows = np.nonzero((s != want).any(axis=1))[0]
    if rows.size:
        c = int(rows[0])
        i = int(np.nonzero(s[c] != want[c])[0][0])
        raise AssertionError(f"{tag}: {rows.size} slots differ, first channel {c} at slot byte {i}: hist_len {int(s[c, :4].view('<u4')[0])} "
                             f"(model {int(want[c, :4].view('<u4')[0])}), bytes {s[c, i:i + 8].tobytes().hex()} (model {want[c, i:i + 8].tobytes().hex()})")


def _reach_back(rng, size):
    """A whole packet of exactly `size` >= 24 bytes that BEGINS with a copy reaching in front of its own output: what it gives
    depends on the history it starts from."""
    head = int(rng.integers(8, 24))
    bits = M.copy_bits(int(rng.integers(head + 1, 41)), head)      # (every history here that is one has 40 bytes and more)
    return _join(bits, M.synth_exact(rng, size - head))


def _join(bits, tail_packet):
    """`bits`, then the tokens of a whole packet made by the synthesiser (its bits are its bytes: it ends with the marker and padding)."""
    tail = "".join(f"{v:08b}" for v in tail_packet)
    return M.to_bytes(bits + tail)


def _reach_back_text(rng, data):
    """The same for a packet of real bytes: a copy of 8 - 23 bytes from in front of the packet, then `data` behind its first bytes as
    the compressor model codes it from an empty history (the bytes that follow are no zeros, so the next reset has something to discard)."""
    head = int(rng.integers(8, 24))
    return _join(M.copy_bits(int(rng.integers(head + 1, 41)), head), O.compress_channel(b"", data[head:])[0])


def decode_step(packets, rooms):
    return lambda b, hist: O.decompress_channel(hist, packets[b], rooms[b])


def compress_step(packets, rooms):
    def step(b, hist):
        out, _, st, new = O.compress_channel(hist, packets[b], rooms[b])
        return out, st, new
    return step


def slot_rows(hists):
    """The slots' bytes for these starting histories; None: no state (hist_len 4000 over a 0x77 fill)."""
    rows = np.zeros((len(hists), SLOT), dtype=np.uint8)
    for c, h in enumerate(hists):
        if h is None:
            rows[c] = 0x77
            rows[c, :4] = (0xA0, 0x0F, 0, 0)
        else:
            rows[c, :4] = np.frombuffer(len(h).to_bytes(4, "little"), dtype=np.uint8)
            rows[c, HIST_AT:HIST_AT + len(h)] = np.frombuffer(h, dtype=np.uint8)
    return rows


# ------------------------------------------------------------------ the runs of a queue
class Run:
    """Packets (entries of the queue, ascending) that one decoder stream takes: `key` the channel (nch for ids out of range),
    `fresh` where a reset started it."""

    def __init__(self, key, fresh):
        self.key, self.fresh, self.packets = key, fresh, []


def runs(ids, flags, nch, skip=()):
    """The runs of DESIGN.md 3.18, in sorted order (their index is the run's 0-based id): the entries grouped by channel with a
    stable sort, ids out of range behind every channel; a run starts at a channel's first entry and at every flagged block of a
    channel in range."""
    ids = np.asarray(ids)
    key = np.where((ids >= 0) & (ids < nch), ids, nch)
    out = []
    for b in np.argsort(key, kind="stable"):
        b = int(b)
        reset = bool(flags[b] & 1) and key[b] < nch and b not in skip
        if not out or out[-1].key != key[b] or reset:
            out.append(Run(int(key[b]), reset))
        out[-1].packets.append(b)
    return out


def run_weights(rs, packets, nch, skip=()):
    """[compressed bytes] of the runs of channels in range: what the decoder's threshold (LZS_BURST_SPLIT_MIN) is held against."""
    return [sum(len(packets[b]) for b in r.packets if b not in skip) for r in rs if r.key < nch]


def mixed_threshold(weights):
    """A threshold with runs on both sides of it, from the weights alone: their median, or -- where nothing is lighter than the
    median -- the lightest weight above the minimum.  None: all runs weigh the same."""
    w = sorted(weights)
    if not w or w[0] == w[-1]:
        return None
    t = w[len(w) // 2]
    if t == w[0]:
        t = next(v for v in w if v > w[0])
    assert any(v < t for v in w) and any(v >= t for v in w)
    return t


# ------------------------------------------------------------------ the queues
class Form:
    """A queue as one call sees it: `index` the queue's entries taken, `skip` the positions (in this form) that are not blocks."""

    def __init__(self, q, packed):
        self.packed = packed
        self.index = [b for b in range(len(q.ids)) if packed or q.block[b]]
        self.ids = [int(q.ids[b]) for b in self.index]
        self.flags = [int(q.flags[b]) for b in self.index]
        self.skip = {k for k, b in enumerate(self.index) if not q.block[b]}
        self.plain = [q.plain[b] for b in self.index]
        self.coded = [q.coded[b] for b in self.index]
        self.n = len(self.index)

    def runs(self, nch):
        return runs(self.ids, self.flags, nch, self.skip)


class Queue:
    """ids, flags (bit 0 the reset, the upper bits random), nch, start histories (None: no state); block[b] False: an entry of the
    packed calls only, not a block; plain[b]: the compressor's packet; coded[b]: the decoder's."""

    def __init__(self, name, ids, flags, nch, block, hists, plain):
        self.name, self.ids, self.flags, self.nch, self.block, self.hists, self.plain = name, ids, flags, nch, block, hists, plain
        self.coded, self.kinds = [], []
        self.strided, self.packed = None, None

    def forms(self):
        return (self.strided, self.packed)


def _pattern_ids(pattern, rng):
    """(ids of the blocks, nchannels, ids out of range among them): the patterns of tests/test_gpu_channels_burst.py scaled to about
    600 packets, and three of this file."""
    if pattern == "distinct":
        return rng.permutation(500), 500, 10
    if pattern == "uniform4":
        return rng.permutation(np.repeat(np.arange(150), 4)), 150, 12
    if pattern == "zipf":
        return (rng.zipf(1.1, 600) - 1) % 150, 150, 12
    if pattern == "one300":
        return rng.permutation(np.concatenate([np.zeros(300, dtype=np.int64), np.arange(1, 301)])), 301, 12
    if pattern == "tiny":
        return rng.integers(0, 4, 600), 4, 8
    if pattern == "pairs":                                       # 330 channels of 2 - 3 packets, every fourth id a single one (110)
        nch = 440
        counts = np.where(np.arange(nch) % 4 == 1, 1, rng.integers(2, 4, nch))
        if counts.sum() % 2:                                     # (an even number in range: with the one out of range n is odd)
            counts[np.nonzero(counts == 2)[0][0]] = 3
        return rng.permutation(np.repeat(np.arange(nch), counts)), nch, 1
    if pattern == "two":
        return np.array([0, 0]), 1, 0
    if pattern == "three":
        return np.array([1, 0, 1]), 2, 0                         # (the last run of the call is a second run: the last staging slot)
    raise ValueError(pattern)


def _density_bits(density, ids, rng):
    """Bit 0 of the blocks' flags."""
    n = len(ids)
    first, last = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for c in np.unique(ids):
        at = np.nonzero(ids == c)[0]
        first[at[0]], last[at[-1]] = True, True
    if density == "sparse":
        return rng.random(n) < 1 / 16
    if density == "quarter":
        return rng.random(n) < 1 / 4
    if density == "all":
        return np.ones(n, dtype=bool)
    if density == "first_only":
        return first
    if density == "last_only":
        return last
    if density == "not_first":
        return ~first
    raise ValueError(density)


def _lengths(pattern, n, rng):
    if pattern == "tiny":
        return rng.integers(1, 41, n)
    if pattern in ("two", "three"):
        return rng.integers(200, 401, n)
    u = rng.random(n)
    return np.where(u < 0.1, 0, np.where(u < 0.55, rng.integers(1, 41, n), rng.integers(41, 1501, n)))


PERIODS = (300, 777, 1024, 1900)         # a channel's text repeats after this many bytes: inside the window, across many packets


@functools.lru_cache(maxsize=None)
def _text():
    return lzs.workload.fill("text", 64, 2048)


def channel_string(c, start, n):
    """Bytes [start, start + n) of channel c's text."""
    return _text()[c % 64, (start + np.arange(n)) % PERIODS[c % 4]]


@functools.lru_cache(maxsize=None)
def queue(pattern, density, seed=1):
    rng = np.random.default_rng([seed, PATTERNS.index(pattern), DENSITIES.index(density)])
    ids, nch, outside = _pattern_ids(pattern, rng)
    ids = np.asarray(ids, dtype=np.int64).copy()
    if outside:                                                  # some ids >= nchannels (pairs: one, an entry of its own)
        if pattern == "pairs":
            ids = np.insert(ids, int(rng.integers(0, ids.size)), nch + 2)
        else:
            at = rng.choice(ids.size, outside, replace=False)
            ids[at] = nch + rng.integers(0, 4, outside)
    bits = _density_bits(density, ids, rng)
    if pattern == "two":
        bits[1] = True
    # the packed form's entries that are not blocks: an even number of them, on channels in range, half of them flagged
    n = ids.size
    extra = 0 if n < 4 else max(2, n // 40 // 2 * 2)
    block = np.ones(n + extra, dtype=bool)
    block[rng.choice(n + extra, extra, replace=False)] = False
    full = np.zeros(n + extra, dtype=np.int64)
    full[block] = ids
    full[~block] = rng.choice(ids[ids < nch], extra) if extra else []
    fbits = np.zeros(n + extra, dtype=bool)
    fbits[block] = bits
    fbits[~block] = rng.random(extra) < 0.5
    flags = (fbits.astype(np.uint8) | (rng.integers(0, 128, n + extra) << 1).astype(np.uint8))
    for k, b in enumerate(np.nonzero(~fbits)[0][:2]):            # the upper bits alone never reset ...
        flags[b] = (0xFE, 0x80)[k]
    for k, b in enumerate(np.nonzero(fbits)[0][:2]):             # ... and never keep bit 0 from it
        flags[b] = (0xFF, 0x01)[k]
    # start slots: history lengths in turn, one slot in eight no state; the history is the channel's text in front of its packets
    hl = [M.HIST_LENS[(c + 6) % len(M.HIST_LENS)] for c in range(nch)]
    hists = [None if nch >= 6 and c % 8 == 5 else channel_string(c, 4096 - hl[c], hl[c]).tobytes() for c in range(nch)]
    pos = {}
    lens = _lengths(pattern, n + extra, rng)
    plain = []
    for b, c in enumerate(full):
        if not block[b]:
            plain.append(b"junk!")
            continue
        c, k = int(c), int(lens[b])
        p = channel_string(c, pos.setdefault(c, 4096), k).copy()
        pos[c] += k
        if k >= 16 and rng.random() < 0.5:
            p[rng.integers(0, k, 2)] = rng.integers(0, 256, 2, dtype=np.uint8)
        plain.append(p.tobytes())
    q = Queue(f"{pattern}/{density}", full, flags, nch, block, hists, plain)
    # the decoder's packets: the compressor's, encoded by the model under the rule; about a third of the flagged ones replaced by
    # packets whose first copy reaches in front of their own output, about one in eight of the others by packets of random tokens
    # (copies at every offset: what they give depends on the whole window, and on where it was emptied)
    skip = set(int(b) for b in np.nonzero(~block)[0])
    outs, status, _, _ = _apply_rule(compress_step(plain, [A.compressed_max(len(p)) for p in plain]), full, flags, hists, skip)
    carried = list(hists)                                        # the decoder's histories on the way, by the model
    for b in range(n + extra):
        kind, p, c = "", outs[b], int(full[b])
        if status[b] == A.STATUS_ERROR:
            q.coded.append(JUNK)
            q.kinds.append("error")
            continue
        if fbits[b] and rng.random() < 1 / 3:
            kind, p = "reach back", _reach_back_text(rng, plain[b])
            for _ in range(8):                                   # (one whose first copy finds more than zeros in the history the reset discards)
                if not carried[c] or O.decompress_channel(carried[c], p, 1 << 20)[0] != O.decompress_channel(b"", p, 1 << 20)[0]:
                    break
                p = _reach_back_text(rng, plain[b])
        elif not fbits[b] and len(plain[b]) >= 2 and rng.random() < 1 / 8:
            kind, p = "deep", M.synth_exact(rng, len(plain[b]))
        carried[c] = O.decompress_channel(b"" if fbits[b] else carried[c], p, 1 << 20)[2]
        q.coded.append(p)
        q.kinds.append(kind)
    q.strided, q.packed = Form(q, False), Form(q, True)
    return q


def all_queues():
    return [queue(p, d) for p in PATTERNS for d in DENSITIES]


# ------------------------------------------------------------------ what a queue reaches
def told_apart(step, form, hists):
    """(flagged blocks of channels in range that are not their channel's first block, how many of them the model codes differently
    with that one flag cleared -- other bytes, or another status)."""
    hists = list(hists)
    later, told, seen = 0, 0, set()
    for b, c in enumerate(form.ids):
        if not 0 <= c < len(hists) or b in form.skip:
            continue
        if form.flags[b] & 1:
            if c in seen:
                later += 1
                kept = (b"", A.STATUS_ERROR) if hists[c] is None else step(b, hists[c])[:2]
                told += kept != step(b, b"")[:2]
            hists[c] = b""
        seen.add(c)
        if hists[c] is not None:
            hists[c] = step(b, hists[c])[2]
    return later, told


def reach(q, form):
    """Counts of what the queue reaches in this form, from the run borders and the models alone."""
    rs = form.runs(q.nch)
    per = {}
    for k, r in enumerate(rs):
        if r.key < q.nch:
            per.setdefault(r.key, []).append(k)
    staged = [v[-1] for v in per.values() if len(v) >= 2]
    flagged = [b for b in range(form.n) if form.flags[b] & 1]
    roomy = [1 << 20] * form.n
    later, told_c = told_apart(compress_step(form.plain, [A.compressed_max(len(p)) for p in form.plain]), form, q.hists)
    _, told_d = told_apart(decode_step(form.coded, roomy), form, q.hists)
    later_flagged = _later_flagged(form, q.nch)
    return {"n": form.n, "runs1": sum(len(v) == 1 for v in per.values()), "runs2": sum(len(v) == 2 for v in per.values()),
            "runs3+": sum(len(v) >= 3 for v in per.values()), "staged": len(staged),
            "top_slot": max(((k - 1) // 2 for k in staged), default=-1), "commit_nowhere": sum(len(v) - 1 for v in per.values()),
            "flagged_not_blocks": sum(b in form.skip for b in flagged), "flagged_outside": sum(form.ids[b] >= q.nch for b in flagged),
            "flagged_later": later, "told_compress": told_c, "told_decode": told_d,
            "reach_back_later": sum(1 for k, b in enumerate(form.index) if q.kinds[b] == "reach back" and k in later_flagged)}


def _later_flagged(form, nch):
    seen, out = set(), set()
    for b, c in enumerate(form.ids):
        if not 0 <= c < nch or b in form.skip:
            continue
        if form.flags[b] & 1 and c in seen:
            out.add(b)
        seen.add(c)
    return out
