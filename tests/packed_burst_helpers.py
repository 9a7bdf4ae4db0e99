"""What tests/test_gpu_packed_burst_compress.py and test_gpu_packed_burst_decode.py share: which entries of a scenario's rounds are
made "not a block", where the packets are placed, and how the rooms are laid out when some pairs of output offsets decrease."""
import numpy as np

GUARD, FILL = 64, 0xA5
BLOCK_MAX = 3 << 30


def valid(c, hists):
    return 0 <= c < len(hists) and hists[c] is not None


def special_channels(sc):
    """(A, B) from the scenario's first round: the channel in range and with a state that has the most packets there -- its
    first, middle and last packet of every round become entries that are not blocks --, and the one with the next most, all of
    whose packets do in every round (its slot gets junk behind hist_len and must stay as it is)."""
    ids = np.asarray(sc.rounds[0][1])
    cs, counts = np.unique(ids[[valid(int(c), sc.slots) for c in ids]], return_counts=True)
    order = np.argsort(-counts, kind="stable")
    assert order.size >= 2 and counts[order[0]] >= 3 and counts[order[1]] >= 2, "the scenario has no two runs to choose"
    return int(cs[order[0]]), int(cs[order[1]])


def not_blocks(sc, r, with_len, use_a=True, use_b=True):
    """{entry: kind} for round r: "length" -- a length above LZS_BLOCK_MAX, where there are lengths -- or "pair" -- a decreasing
    pair of output offsets.  Channel A's first packet, one a third into its run and its last (first in a run, in mid-run, last in
    a run), and all of B's."""
    if not (use_a or use_b):
        return {}
    a, b = special_channels(sc)
    ids = np.asarray(sc.rounds[r][1])
    mine = np.nonzero(ids == a)[0]
    chosen = []
    if use_a:
        chosen += [int(mine[0]), int(mine[len(mine) // 3]), int(mine[-1])] if len(mine) >= 3 else [int(x) for x in mine[:1]]
    if use_b:
        chosen += [int(x) for x in np.nonzero(ids == b)[0]]
    return {e: ("length" if with_len and k % 2 == 0 else "pair") for k, e in enumerate(chosen)}


def junk_slot(before, c, hist):
    """Junk in slot c behind hist_len: the reserved bytes of the header and the history area past the history."""
    before[c, 4:64] = 0x3C
    before[c, 64 + len(hist):] = 0x5A
    return before[c].copy()


def place(torch, packets, with_len, too_long=()):
    """The packets back to back, the first byte one byte behind an aligned address; with lengths they lie in reverse order, and the
    entries in `too_long` claim more than LZS_BLOCK_MAX bytes.  Returns (data, in_off int64 [n + 1], in_len or None)."""
    n = len(packets)
    order = list(reversed(range(n))) if with_len else list(range(n))
    start, at = [0] * n, 0
    for b in order:
        start[b] = at
        at += len(packets[b])
    host = np.random.default_rng(at).integers(0, 256, at + 1 + 64, dtype=np.uint8)
    for b, p in enumerate(packets):
        host[1 + start[b]:1 + start[b] + len(p)] = np.frombuffer(p, dtype=np.uint8)
    flat = torch.from_numpy(host).cuda()
    assert flat.data_ptr() % 16 == 0
    in_off = torch.tensor(start + [at], dtype=torch.int64, device="cuda")
    in_len = None
    if with_len:
        lens = np.array([len(p) for p in packets], dtype=np.uint32)
        for b in too_long:
            lens[b] = BLOCK_MAX + 1
        in_len = torch.from_numpy(lens.view(np.int32).copy()).cuda()
    return flat[1:1 + at], in_off, in_len


def lay_out(rooms, decreasing=(), align=1):
    """out_off [n + 1] for these rooms, and the size of d_out.  The entries in `decreasing` have a pair of offsets that decreases:
    the entries up to and including one form a chain of rooms back to back (its own room is none), and the chain behind it lies
    lower in d_out, three bytes and more below everything before -- so no two rooms overlap.  `align`: every room starts at a
    multiple of it (rooms rounded up)."""
    n = len(rooms)
    chains, cur = [], []
    for b in range(n):
        cur.append(b)
        if b in decreasing:
            chains.append(cur)
            cur = []
    chains.append(cur)                                             # (the last chain may be empty: off[n] alone)
    off = np.zeros(n + 1, dtype=np.int64)
    at = 0
    for k in range(len(chains) - 1, -1, -1):                       # the last chain lowest
        first = chains[k][0] if chains[k] else n
        off[first] = at
        for b in chains[k]:
            size = 0 if b in decreasing else -(-int(rooms[b]) // align) * align
            at += size
            if b not in decreasing:
                off[b + 1] = at
        at = -(-(at + 3) // align) * align
    for b in decreasing:
        assert off[b + 1] < off[b], (b, off[b], off[b + 1])
    return off, int(at)


def expected_buffer(off, outs, total, lead=GUARD + 1):
    """d_out lies `lead` bytes into a buffer of 0xA5 with GUARD more behind it."""
    want = np.full(lead + total + GUARD, FILL, dtype=np.uint8)
    for b, w in enumerate(outs):
        want[lead + off[b]:lead + off[b] + len(w)] = np.frombuffer(w, dtype=np.uint8)
    return want


def compare(tag, got_buf, got_len, got_st, want_buf, outs, status, off, lead=GUARD + 1):
    want_len = np.array([len(w) for w in outs])
    bad = np.nonzero((got_len != want_len) | (got_st != status))[0]
    assert not bad.size, (tag, "packets", bad[:5].tolist(), "lengths", got_len[bad[:5]].tolist(), "model", want_len[bad[:5]].tolist(),
                          "status", got_st[bad[:5]].tolist(), "model", status[bad[:5]].tolist())
    diff = np.nonzero(got_buf != want_buf)[0]
    if diff.size:
        i = int(diff[0]) - lead
        near = int(np.argmin([abs(int(off[k]) - i) if int(off[k]) <= i else 1 << 60 for k in range(len(outs))]))
        raise AssertionError(f"{tag}: {diff.size} bytes differ, the first at d_out[{i}] (behind the start of packet {near} at {int(off[near])}, "
                             f"length {int(want_len[near])}): {got_buf[diff[0]:diff[0] + 8].tobytes().hex()}, the model "
                             f"{want_buf[diff[0]:diff[0] + 8].tobytes().hex()}")
