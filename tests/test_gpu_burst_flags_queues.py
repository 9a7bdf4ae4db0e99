"""History resets inside a burst on generated queues (tests/burst_flags_cases.py): the four flags entries against the
plain CPU models under the rule, at the sizes where the run tables, the staging slots and the two decode routes can go wrong --
hundreds of channels with a second run, n = 2 and n = 3, runs of one call on both sides of the threshold, windows of tiny packets
that would reach across a reset, malformed packets and cut rooms inside runs that a reset started, and graph capture.

Every call here gets a work area filled with 0xA5 with a guard behind it and outputs filled with 0xA5 with guards, and is compared
with none left out: every packet's bytes, length and status, every slot in full, the fill past each length, and the guards.  No
expected value comes from the library."""
import numpy as np
import pytest

import lzs_compression_amd as lzs
from lzs_compression_amd import api as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import burst_flags_cases as C  # noqa: E402
import packed_burst_helpers as H  # noqa: E402
import test_channel_model as M  # noqa: E402
from burst_flags_cases import _apply_rule, _check_slots, _reach_back, _want_slots  # noqa: E402
from packed_burst_helpers import FILL, GUARD  # noqa: E402
from test_channel_model import O  # noqa: E402
from test_gpu_burst_flags import _check_strided, _dev, _rows, _work  # noqa: E402

QUEUES = [(p, d) for p in C.PATTERNS for d in C.DENSITIES]
LEAD = GUARD + 1


def _split_env(monkeypatch, split_min):
    if split_min is None:
        monkeypatch.delenv("LZS_BURST_SPLIT_MIN", raising=False)
    else:
        monkeypatch.setenv("LZS_BURST_SPLIT_MIN", str(int(split_min)))


def _staging_untouched(tag, work, n):
    """A flagged decode keeps its tables and its n // 2 staging slots where the compressor has its n work slots (lzs_burst_plan.h,
    restated: every part rounded up to 256 bytes).  What lies between the last staging slot and the end of that region belongs to
    nothing: a staging index one too high writes there."""
    def up(x):
        return (x + 255) // 256 * 256
    stage_end = up(4) + 2 * up(4 * n) + 3 * up(8 * n) + up(n // 2 * A.CHANNEL_STATE_BYTES)
    region_end = up(n * A.CHANNEL_STATE_BYTES)
    assert stage_end < region_end
    assert bool((work[stage_end:region_end] == FILL).all()), f"{tag}: bytes behind the last staging slot were written"


class Strided:
    """A queue's packets as rows on the device, once for all calls on them."""

    def __init__(self, packets, ids, flags):
        self.n = len(packets)
        self.x, self.xl = _rows(packets)
        self.ch, self.fl = _dev(ids, torch.int32), _dev(flags, torch.uint8)

    def call(self, tag, decompress, before, cap, work_bytes, want):
        """One call on a copy of the slots `before`; want: what _apply_rule gave.  Returns (the call's tensors, its work area)."""
        nch = before.shape[0]
        states = torch.from_numpy(before).cuda()
        out = torch.full((self.n, (cap + 15) // 16 * 16 + GUARD), FILL, dtype=torch.uint8, device="cuda")
        work, behind = _work(work_bytes)
        fn = lzs.decompress_channels_burst if decompress else lzs.compress_channels_burst
        got = fn(self.x, self.xl, self.ch, states, cap, out=out, work=work, flags=self.fl)
        torch.cuda.synchronize()
        outs, status, final, touched = want
        _check_strided(tag, got, outs, status)
        _check_slots(tag, states, _want_slots(before, final, touched))
        assert bool((behind == FILL).all()), f"{tag}: bytes behind the work area were written"
        assert nch == len(final)
        if decompress:
            _staging_untouched(tag, work, self.n)
        return got, work


class Packed:
    """The same packets back to back, in reverse order with lengths, and their rooms laid out with the entries in `not_blocks`
    {entry: "pair" | "length"} made no blocks: a decreasing pair of output offsets, or a length above LZS_BLOCK_MAX."""

    def __init__(self, packets, ids, flags, rooms, not_blocks):
        self.n = len(packets)
        pairs = {b for b, kind in not_blocks.items() if kind == "pair"}
        rooms = [0 if b in not_blocks else int(r) for b, r in enumerate(rooms)]
        self.off, self.total = H.lay_out(rooms, pairs)
        assert all(b in pairs or int(self.off[b + 1] - self.off[b]) == rooms[b] for b in range(self.n))
        self.rooms = rooms
        self.data, self.in_off, self.in_len = H.place(torch, packets, True, {b for b, kind in not_blocks.items() if kind == "length"})
        self.ch, self.fl = _dev(ids, torch.int32), _dev(flags, torch.uint8)
        self.doff = torch.from_numpy(self.off).cuda()

    def call(self, tag, decompress, before, split, want):
        nch = before.shape[0]
        states = torch.from_numpy(before).cuda()
        buf = torch.full((LEAD + self.total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        size = lzs.channels_burst_packed_split_work_bytes(self.n, nch, self.total) if split else lzs.channels_burst_work_bytes(self.n, nch)
        work, behind = _work(size)
        fn = lzs.decompress_channels_burst_packed if decompress else lzs.compress_channels_burst_packed
        _, out_len, st = fn(self.data, self.in_off, self.ch, states, buf[LEAD:LEAD + self.total], self.doff, in_len=self.in_len, work=work,
                            flags=self.fl)
        torch.cuda.synchronize()
        outs, status, final, touched = want
        H.compare(tag, buf.cpu().numpy(), out_len.cpu().numpy(), st.cpu().numpy(), H.expected_buffer(self.off, outs, self.total, LEAD), outs,
                  status, self.off, LEAD)
        _check_slots(tag, states, _want_slots(before, final, touched))
        assert bool((behind == FILL).all()), f"{tag}: bytes behind the work area were written"
        if decompress:
            _staging_untouched(tag, work, self.n)
        return (buf, out_len, st), work


def _kinds(skip):
    return {b: ("length" if k % 2 == 0 else "pair") for k, b in enumerate(sorted(skip))}


def _mixed(form, nch):
    """The threshold that puts runs of this queue on both routes, from the queue's own run weights (None: they are all equal)."""
    return C.mixed_threshold(C.run_weights(form.runs(nch), form.coded, nch, form.skip))


# ------------------------------------------------------------------ a. the decoder, every queue, every route
@pytest.mark.parametrize("pattern,density", QUEUES)
def test_decoder_equals_the_model_on_every_queue_and_route(monkeypatch, pattern, density):
    q = C.queue(pattern, density)
    before = C.slot_rows(q.hists)
    for form in q.forms():
        sizes = M.true_sizes(form.coded)
        mixed = _mixed(form, q.nch)
        name = f"{q.name} {'packed' if form.packed else 'strided'} decode"
        if form.packed:
            dev = Packed(form.coded, form.ids, form.flags, sizes, _kinds(form.skip))          # every room exactly the packet's size
            want = _apply_rule(C.decode_step(form.coded, dev.rooms), form.ids, form.flags, q.hists, form.skip)
        else:
            cap = max(sizes) + 1
            dev = Strided(form.coded, form.ids, form.flags)
            want = _apply_rule(C.decode_step(form.coded, [cap] * form.n), form.ids, form.flags, q.hists)
        routes = [("run", False, None), ("split 0", True, 0), ("split default", True, None)]
        if mixed is not None:                                                  # (all runs weigh the same: no threshold divides them)
            routes.insert(2, ("split mixed", True, mixed))
        for route, split, split_min in routes:
            tag = f"{name}, {route} ({split_min})"
            _split_env(monkeypatch, split_min)
            if form.packed:
                dev.call(tag, True, before, split, want)
            else:
                size = lzs.channels_burst_split_work_bytes(form.n, q.nch, cap) if split else lzs.channels_burst_work_bytes(form.n, q.nch)
                dev.call(tag, True, before, cap, size, want)


# ------------------------------------------------------------------ b. the compressor, every queue
def _cut_rooms(form, nch, outs, status):
    """{entry: a room three bytes short of what it needs}: two flagged and two unflagged blocks of channels in range."""
    cut = {}
    for flagged in (1, 0):
        mine = [b for b in range(form.n) if (form.flags[b] & 1) == flagged and status[b] == 0x07 and len(outs[b]) > 8 and b not in form.skip]
        for b in (mine[len(mine) // 3], mine[-1]) if len(mine) >= 2 else ():
            cut[b] = len(outs[b]) - 3
    return cut


@pytest.mark.parametrize("pattern,density", QUEUES)
def test_compressor_equals_the_model_on_every_queue(pattern, density):
    q = C.queue(pattern, density)
    before = C.slot_rows(q.hists)
    for form in q.forms():
        name = f"{q.name} {'packed' if form.packed else 'strided'} compress"
        rooms = [A.compressed_max(len(p)) for p in form.plain]
        want = _apply_rule(C.compress_step(form.plain, rooms), form.ids, form.flags, q.hists, form.skip)
        cut = _cut_rooms(form, q.nch, want[0], want[1]) if pattern == "tiny" else {}
        assert pattern != "tiny" or len(cut) == 4 or density not in ("sparse", "quarter", "not_first", "last_only")
        size = lzs.channels_burst_work_bytes(form.n, q.nch)
        if form.packed:
            for b, room in cut.items():
                rooms[b] = room
            dev = Packed(form.plain, form.ids, form.flags, rooms, _kinds(form.skip))
            want = _apply_rule(C.compress_step(form.plain, dev.rooms), form.ids, form.flags, q.hists, form.skip)
            assert all(want[1][b] == 0x0B for b in cut)
            dev.call(name, False, before, False, want)
        else:
            dev = Strided(form.plain, form.ids, form.flags)
            cap = max(rooms)
            dev.call(name, False, before, cap, size, want)
            if cut:                                                            # one capacity for all: it cuts these and every longer packet
                cap = min(cut.values())
                want = _apply_rule(C.compress_step(form.plain, [cap] * form.n), form.ids, form.flags, q.hists)
                assert all(want[1][b] == 0x0B for b in cut)
                dev.call(name + f", capacity {cap}", False, before, cap, size, want)


# ------------------------------------------------------------------ c. both routes on one channel
def _both_routes_queue():
    """Channels 0 - 4 with runs of one and of three text packets of 1500 bytes, flags F where a reset starts a run:
    0: p F p p       light from the slot, heavy fresh and last          3: p F p p F    light, heavy fresh that commits nowhere, light fresh last
    1: p p p F       heavy from the slot, light fresh and last          4: p F p p      a slot that is no state (ERROR), a heavy fresh run
    2: p p p F p p   heavy, heavy fresh
    among 40 channels of one packet each, four of them flagged.  The flagged packets begin with a copy from in front of themselves."""
    rng = np.random.default_rng(318)
    shapes = ("pFpp", "pppF", "pppFpp", "pFppF", "pFpp")
    nch = len(shapes) + 40
    order = rng.permutation(np.concatenate([np.repeat(np.arange(len(shapes)), [len(s) for s in shapes]), np.arange(len(shapes), nch)]))
    seen = {}
    ids, flags = [], []
    for c in order:
        c = int(c)
        k = seen.get(c, 0)
        seen[c] = k + 1
        ids.append(c)
        flags.append(int(shapes[c][k] == "F") if c < len(shapes) else int(c % 10 == 7))
    text = lzs.workload.fill("text", nch, 1 << 14)
    hists = [text[c, :M.HIST_LENS[(c + 1) % 7] if c >= 4 else 2047].tobytes() for c in range(nch)]
    hists[4] = None
    pos = {}
    plain = []
    for c in ids:
        at = pos.setdefault(c, 2047)
        plain.append(text[c, at:at + 1500].tobytes())
        pos[c] = at + 1500
    outs, status, _, _ = _apply_rule(C.compress_step(plain, [A.compressed_max(1500)] * len(ids)), ids, flags, hists)
    coded = [C.JUNK if status[b] == A.STATUS_ERROR else (_reach_back(rng, 1500) if flags[b] else outs[b]) for b in range(len(ids))]
    return ids, flags, nch, hists, coded


def _origins_by_route(tag, work, small, ids, nch, rs, heavy, rooms, lens):
    """Which route took a run is seen in the work area behind the burst size: PARSE writes a 16-bit origin for every byte a packet
    of a heavy run gives, at the packet's sorted position -- its rooms' scan --, and nothing writes there for a light run."""
    org = work[small:].cpu().numpy()
    org = org[:org.size // 2 * 2].view(np.uint16)
    at = 0
    seen = {True: 0, False: 0}
    for r, run in enumerate(rs):
        for b in run.packets:
            mine = org[at:at + rooms[b]]
            if run.key < nch and heavy[r]:
                assert (mine[:lens[b]] != FILL * 0x0101).all(), f"{tag}: packet {b} of a heavy run has origins that were not written"
                assert (mine[lens[b]:] == FILL * 0x0101).all(), f"{tag}: packet {b}: origins behind its length were written"
                seen[True] += lens[b] > 0
            elif run.key < nch:
                assert (mine == FILL * 0x0101).all(), f"{tag}: packet {b} of a light run has origins: it was parsed"
                seen[False] += 1
            at += rooms[b]
    assert seen[True] and seen[False], f"{tag}: {seen}"


@pytest.mark.parametrize("packed", [False, True], ids=["strided", "packed"])
def test_runs_of_one_channel_on_both_routes(monkeypatch, packed):
    ids, flags, nch, hists, coded = _both_routes_queue()
    n, cap = len(ids), 1500
    rs = C.runs(ids, flags, nch)
    weights = [sum(len(coded[b]) for b in r.packets) for r in rs]
    light = max(w for r, w in zip(rs, weights) if len(r.packets) == 1)
    heavy_min = min(w for r, w in zip(rs, weights) if len(r.packets) == 3)
    assert light < heavy_min and {len(r.packets) for r in rs} == {1, 3}
    threshold = light + 1
    heavy = [w >= threshold for w in weights]
    by_channel = {c: [(heavy[k], r.fresh) for k, r in enumerate(rs) if r.key == c] for c in range(5)}
    assert by_channel == {0: [(False, False), (True, True)], 1: [(True, False), (False, True)], 2: [(True, False), (True, True)],
                          3: [(False, False), (True, True), (False, True)], 4: [(False, False), (True, True)]}
    _split_env(monkeypatch, threshold)
    before = C.slot_rows(hists)
    rooms = [cap] * n
    want = _apply_rule(C.decode_step(coded, rooms), ids, flags, hists)
    assert want[1][ids.index(4)] == A.STATUS_ERROR and (want[1] == M.END).sum() == n - 1
    lens = [len(o) for o in want[0]]
    small = lzs.channels_burst_work_bytes(n, nch)
    if packed:
        dev = Packed(coded, ids, flags, rooms, {})
        _, work = dev.call("both routes, packed", True, before, True, want)
    else:
        dev = Strided(coded, ids, flags)
        _, work = dev.call("both routes, strided", True, before, cap, lzs.channels_burst_split_work_bytes(n, nch, cap), want)
    _origins_by_route("both routes", work, small, ids, nch, rs, heavy, rooms, lens)


# ------------------------------------------------------------------ d. a copy that reaches back to a reset, and over it
@pytest.mark.parametrize("behind", [1, 2046, 2047, 2048])
def test_a_copy_reaches_back_over_one_byte_packets_to_a_reset(monkeypatch, behind):
    """3000 packets of one byte on one channel, the one that gives the byte `behind` bytes in front of the first copying packet
    flagged; then three packets that copy the 2047 bytes before them.  What lies in front of the reset reads as zero."""
    rng = np.random.default_rng(behind)
    base = rng.integers(1, 256, 3000)
    packets = [M.to_bytes(M.lit_bits(int(v)) + M.MARKER) for v in base] + [M.to_bytes(M.copy_bits(2047, 2047) + M.MARKER)] * 3
    n = len(packets)
    ids, flags = [0] * n, [0] * n
    flags[3000 - behind] = 0x81
    hists = [M.random_hist(rng, 2047)]
    cap = 2047
    want = _apply_rule(C.decode_step(packets, [cap] * n), ids, flags, hists)
    first = np.frombuffer(want[0][3000], dtype=np.uint8)
    zeros = max(0, 2047 - behind)
    assert first.size == 2047 and not first[:zeros].any() and first[zeros:].all() and (want[1] == M.END).all()
    before = C.slot_rows(hists)
    dev = Strided(packets, ids, flags)
    _split_env(monkeypatch, 0)
    dev.call(f"reset {behind} behind, split 0", True, before, cap, lzs.channels_burst_split_work_bytes(n, 1, cap), want)
    dev.call(f"reset {behind} behind, run", True, before, cap, lzs.channels_burst_work_bytes(n, 1), want)


# ------------------------------------------------------------------ e. malformed packets and cut rooms inside fresh runs
def _fresh_runs_queue():
    """Four channels, each: two packets from the slot, then three runs that a reset starts, of four packets each.  Run t of the
    twelve has one packet spoilt -- its first, a middle one or its last (t // 4) -- in one of four ways ((t + t // 4) % 4): random
    bytes, a good packet with random bytes behind it, a good packet cut short, a room that cuts its first copy."""
    rng = np.random.default_rng(11)
    nch = 4
    text = lzs.workload.fill("text", nch, 1 << 14)
    per = [["p", "p"] for _ in range(nch)]
    for t in range(12):
        run = ["F", "p", "p", "p"]
        run[(0, 2, 3)[t // 4]] += ("random", "tail", "short", "room")[(t + t // 4) % 4]
        per[t % 4] += run
    order = rng.permutation(np.repeat(np.arange(nch), [len(p) for p in per]))
    ids, flags, what, seen = [], [], [], [0] * nch
    for c in order:
        c = int(c)
        w = per[c][seen[c]]
        seen[c] += 1
        ids.append(c)
        flags.append(int(w[0] == "F"))
        what.append(w[1:])
    hists = [text[c, :2047].tobytes() for c in range(nch)]
    pos = [2047] * nch
    plain = []
    for c in ids:
        k = int(rng.integers(200, 400))
        plain.append(text[c, pos[c] % 4096:pos[c] % 4096 + k].tobytes())              # (a channel comes back to its text within the window)
        pos[c] += 1024
    outs, _, _, _ = _apply_rule(C.compress_step(plain, [A.compressed_max(len(p)) for p in plain]), ids, flags, hists)
    coded, rooms = [], []
    for b, good in enumerate(outs):
        room = len(plain[b])
        if flags[b]:
            good = _reach_back(rng, room)
        if what[b] == "random":
            good = rng.integers(0, 256, int(rng.integers(1, 400)), dtype=np.uint8).tobytes()
            room = 600
        elif what[b] == "tail":
            good = good + rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8).tobytes()
        elif what[b] == "short":
            good = good[:int(rng.integers(1, len(good)))]
        elif what[b] == "room":                                                       # inside the packet's first copy
            tokens = O.decompress_channel(b"", good, 1 << 20, trace=True)[3]
            copy = next(t for t in tokens if t[1] and t[2] >= 3)
            room = int(copy[0]) + 1
        coded.append(good)
        rooms.append(room)
    return ids, flags, nch, hists, coded, rooms, what


@pytest.mark.parametrize("route", ["run", "split 0", "split default"])
def test_malformed_packets_and_cut_rooms_inside_fresh_runs(monkeypatch, route):
    ids, flags, nch, hists, coded, rooms, what = _fresh_runs_queue()
    n = len(ids)
    before = C.slot_rows(hists)
    _split_env(monkeypatch, 0 if route == "split 0" else None)
    # packed: every packet its own room; and in the middle of channel 0's second fresh run a flagged entry that is not a block (ERROR)
    mine = [b for b in range(n) if ids[b] == 0]
    extra = mine[2 + 4 + 2]
    p_ids, p_flags, p_coded, p_rooms = list(ids), list(flags), list(coded), list(rooms)
    for lst, v in ((p_ids, 0), (p_flags, 0x01), (p_coded, b"junk!"), (p_rooms, 0)):
        lst.insert(extra, v)
    dev = Packed(p_coded, p_ids, p_flags, p_rooms, {extra: "pair"})
    want = _apply_rule(C.decode_step(p_coded, dev.rooms), p_ids, p_flags, hists, {extra})
    status = np.delete(want[1], extra)
    cut = [b for b in range(n) if what[b] == "room"]
    assert len(cut) == 3 and (status[cut] == M.FULL).all() and want[1][extra] == A.STATUS_ERROR
    assert {int(s) for s in status} == {M.END, M.FULL, M.STARVED}, status.tolist()
    dev.call(f"fresh runs, packed, {route}", True, before, route != "run", want)
    # strided: one capacity -- above every room, and one that cuts most packets
    dev = Strided(coded, ids, flags)
    for cap in (600, 100):
        want = _apply_rule(C.decode_step(coded, [cap] * n), ids, flags, hists)
        size = lzs.channels_burst_work_bytes(n, nch) if route == "run" else lzs.channels_burst_split_work_bytes(n, nch, cap)
        dev.call(f"fresh runs, strided, capacity {cap}, {route}", True, before, cap, size, want)


# ------------------------------------------------------------------ f. graph capture
def _capture(call):
    """One call outside the graph first (the library's start-up), then the same captured: one stream, no branches."""
    call(True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(False)
    return g


@pytest.mark.parametrize("packed", [False, True], ids=["strided", "packed"])
@pytest.mark.parametrize("decompress", [False, True], ids=["compress", "decompress"])
def test_graph_capture_with_flags_equals_direct_calls_and_the_model(monkeypatch, decompress, packed):
    """The `pairs` queue at its mixed threshold: a flagged call captured (the marks kernel, the scan and the staged commit with it),
    replayed twice on restored slots; each replay equals the direct call and the model."""
    q = C.queue("pairs", "quarter")
    form = q.packed if packed else q.strided
    threshold = _mixed(form, q.nch)
    assert threshold is not None
    _split_env(monkeypatch, threshold)
    before = C.slot_rows(q.hists)
    packets = form.coded if decompress else form.plain
    sizes = M.true_sizes(form.coded) if decompress else [A.compressed_max(len(p)) for p in form.plain]
    step = C.decode_step if decompress else C.compress_step
    n, nch = form.n, q.nch
    start = torch.from_numpy(before).cuda()
    states, scratch = start.clone(), start.clone()
    out_len = torch.empty(n, dtype=torch.int32, device="cuda")
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    if packed:
        dev = Packed(packets, form.ids, form.flags, sizes, _kinds(form.skip))
        want = _apply_rule(step(packets, dev.rooms), form.ids, form.flags, q.hists, form.skip)
        direct, _ = dev.call("direct", decompress, before, decompress, want)
        buf = torch.full((LEAD + dev.total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        size = lzs.channels_burst_packed_split_work_bytes(n, nch, dev.total) if decompress else lzs.channels_burst_work_bytes(n, nch)
        work, behind = _work(size)
        fn = lzs.decompress_channels_burst_packed if decompress else lzs.compress_channels_burst_packed
        g = _capture(lambda warm: fn(dev.data, dev.in_off, dev.ch, scratch if warm else states, buf[LEAD:LEAD + dev.total], dev.doff,
                                     in_len=dev.in_len, out_len=out_len, status=status, work=work, flags=dev.fl))
    else:
        cap = max(sizes) + 1
        dev = Strided(packets, form.ids, form.flags)
        want = _apply_rule(step(packets, [cap] * n), form.ids, form.flags, q.hists)
        size = lzs.channels_burst_split_work_bytes(n, nch, cap) if decompress else lzs.channels_burst_work_bytes(n, nch)
        direct, _ = dev.call("direct", decompress, before, cap, size, want)
        buf = torch.full((n, (cap + 15) // 16 * 16 + GUARD), FILL, dtype=torch.uint8, device="cuda")
        work, behind = _work(size)
        fn = lzs.decompress_channels_burst if decompress else lzs.compress_channels_burst
        g = _capture(lambda warm: fn(dev.x, dev.xl, dev.ch, scratch if warm else states, cap, out=buf, out_len=out_len, status=status,
                                     work=work, flags=dev.fl))
    outs, st, final, touched = want
    for r in range(2):
        states.copy_(start)
        buf.fill_(FILL)
        work.fill_(FILL)
        out_len.fill_(-1)
        status.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        tag = f"replay {r}"
        assert all(torch.equal(a, b) for a, b in zip((buf, out_len, status), direct)), f"{tag}: differs from the direct call"
        if packed:
            H.compare(tag, buf.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy(), H.expected_buffer(dev.off, outs, dev.total, LEAD),
                      outs, st, dev.off, LEAD)
        else:
            _check_strided(tag, (buf, out_len, status), outs, st)
        _check_slots(tag, states, _want_slots(before, final, touched))
        assert bool((behind == FILL).all()), f"{tag}: bytes behind the work area were written"
