"""lzs_decompress_channels_burst_packed_device against the plain CPU model of the channel decoder (oracle/lzs_oracle.c:
lzs_oracle_decompress_channel), applied packet by packet in row order per channel with each packet's own room -- the header's
rank-by-rank definition.  The packets of tests/test_channel_model.py's scenarios, synthesised token by token (lengths 0, 1, 2046,
2047 and 2048, long offset 0, young channels copying zeros, preset slots, malformed packets, a copy of 70 000 bytes in mid-run, 2100
one-byte packets), decoded from packed packets to packed rooms three ways -- the run decoder alone (a work area of the burst size),
the split route for every run (LZS_BURST_SPLIT_MIN=0) and at the default threshold -- each byte-equal to the model: the whole output
buffer with its guards, every length, every status, every slot.  The rooms come from the model's true sizes: exact, one byte short,
none, and a cut inside the packet's first copy -- back to back; at align 16 each rounded up to the next room's start."""
import numpy as np
import pytest

import lzs_compression_amd as lzs
from lzs_compression_amd import api as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import packed_burst_helpers as H  # noqa: E402
import test_channel_model as M  # noqa: E402
from packed_burst_helpers import FILL, GUARD  # noqa: E402
from test_channel_model import O  # noqa: E402
from test_gpu_channel_model import _slot_rows  # noqa: E402

ROUTES = ("run", "split 0", "split default")
SCENARIOS = {"burst": M.burst_scenario, "big copy": M.big_copy_scenario, "one byte": M.one_byte_scenario,
             "single65": lambda: M.single_scenario(65)}
_ROOMS = {}


def _rooms(name):
    """Per round and packet the room, chosen from the model (a packet's size does not depend on its history): its true size T, T - 1,
    0, one byte into its first copy (a cut inside a copy), T again -- the marker behind a closing nibble 0 is reached where such a
    packet gets T.  Computed once per scenario."""
    if name not in _ROOMS:
        rounds = []
        for r, (packets, _) in enumerate(SCENARIOS[name]().rounds):
            rooms = []
            for b, p in enumerate(packets):
                out, _, _, tokens, _ = O.decompress_channel(b"", p, 1 << 30, trace=True)
                size = len(out)
                copies = [t for t in tokens if t[1]]
                kind = (b + r) % 5
                rooms.append(size if kind in (0, 4) else max(size - 1, 0) if kind == 1 else 0 if kind == 2 else
                             min(int(copies[0][0]) + 1, size) if copies else size)
            rounds.append(rooms)
        _ROOMS[name] = rounds
    return _ROOMS[name]


def _model(packets, ids, hists, rooms, skip):
    hists = list(hists)
    outs, status = [], []
    for b, (data, c) in enumerate(zip(packets, ids)):
        c = int(c)
        if b in skip or not H.valid(c, hists):
            outs.append(b"")
            status.append(A.STATUS_ERROR)
            continue
        out, st, hists[c] = O.decompress_channel(hists[c], data, rooms[b])
        outs.append(out)
        status.append(st)
    return outs, np.array(status, dtype=np.uint8), hists


def _work(route, monkeypatch, n, nch, out_bytes):
    """The route's work area, filled with 0xA5, and a guard behind it."""
    if route == "split 0":
        monkeypatch.setenv("LZS_BURST_SPLIT_MIN", "0")
    else:
        monkeypatch.delenv("LZS_BURST_SPLIT_MIN", raising=False)
    small = lzs.channels_burst_work_bytes(n, nch)
    need = small if route == "run" else lzs.channels_burst_packed_split_work_bytes(n, nch, out_bytes)
    whole = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 256 == 0
    return whole[:need], whole[need:], whole[small:need]


def _run(name, route, monkeypatch, align, special):
    sc = SCENARIOS[name]()
    hists = list(sc.slots)
    before = _slot_rows(hists)
    chan_b = junk = None
    if special:
        _, chan_b = H.special_channels(sc)
        junk = H.junk_slot(before, chan_b, hists[chan_b])
    states = torch.from_numpy(before).cuda()
    lead = GUARD if align == 16 else GUARD + 1                     # (rooms at multiples of 16, or back to back from an odd address)
    for r, (packets, ids) in enumerate(sc.rounds):
        n = len(packets)
        with_len = bool(r % 2) or len(sc.rounds) == 1
        skip = H.not_blocks(sc, r, with_len, use_a=special, use_b=special)
        rooms = [3 if b in skip else room for b, room in enumerate(_rooms(name)[r])]
        pairs = {b for b, kind in skip.items() if kind == "pair"}
        off, total = H.lay_out(rooms, pairs, align)
        rooms = [0 if b in pairs else int(off[b + 1] - off[b]) for b in range(n)]      # (at align 16 a room ends where the next begins)
        outs, status, hists = _model(packets, ids, hists, rooms, skip)
        data, in_off, in_len = H.place(torch, packets, with_len, [b for b, kind in skip.items() if kind == "length"])
        buf = torch.full((lead + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        ch = torch.tensor(np.asarray(ids, dtype=np.int64).astype(np.int32), dtype=torch.int32, device="cuda")
        work, behind, _ = _work(route, monkeypatch, n, sc.nch, total)
        _, out_len, st = lzs.decompress_channels_burst_packed(data, in_off, ch, states, buf[lead:lead + total], torch.from_numpy(off).cuda(),
                                                              in_len=in_len, work=work)
        torch.cuda.synchronize()
        tag = f"{sc.name}, {route}, align {align}, round {r}, {'lengths given' if with_len else 'no lengths'}, {len(skip)} entries not blocks"
        H.compare(tag, buf.cpu().numpy(), out_len.cpu().numpy(), st.cpu().numpy(), H.expected_buffer(off, outs, total, lead), outs, status,
                  off, lead)
        assert bool((behind == FILL).all()), f"{tag}: bytes behind the work area were written"
        before = _slot_rows(hists, before)
        if special:
            before[chan_b] = junk
        s = states.cpu().numpy()
        rows = np.nonzero((s != before).any(axis=1))[0]
        assert not rows.size, (tag, "slots differ", rows[:5].tolist(), [int(s[c, :4].view("<u4")[0]) for c in rows[:5]],
                               [len(hists[c] or b"") for c in rows[:5]])


@pytest.mark.parametrize("align", (1, 16))
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_three_routes_equal_the_model(monkeypatch, name, route, align):
    _run(name, route, monkeypatch, align, special=False)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ("burst", "one byte"))
def test_entries_that_are_not_blocks_and_a_channel_of_nothing_else(monkeypatch, name, route):
    """Entries that are not blocks -- a length above LZS_BLOCK_MAX, a decreasing pair of output offsets -- first, in mid-run and
    last in the longest run: ERROR, length 0, nothing written, the run goes on with the history it had.  All packets of a second
    channel are such entries and its slot holds junk behind hist_len: untouched byte for byte on every route."""
    _run(name, route, monkeypatch, 1, special=True)


def _burst_case():
    """The burst scenario's first round with rooms of the packets' sizes, placed and modelled."""
    sc = M.burst_scenario()
    packets, ids = sc.rounds[0]
    rooms = [len(O.decompress_channel(b"", p, 1 << 30)[0]) for p in packets]
    outs, status, hists = _model(packets, ids, sc.slots, rooms, {})
    off, total = H.lay_out(rooms)
    data, in_off, in_len = H.place(torch, packets, True)
    ch = torch.tensor(np.asarray(ids, dtype=np.int64).astype(np.int32), dtype=torch.int32, device="cuda")
    return sc, data, in_off, in_len, ch, off, total, outs, status, hists


def test_which_route_ran_is_seen_in_the_work_area(monkeypatch):
    """Equal bytes cannot tell the routes apart; the work area can: filled with 0xA5, the part beyond the burst size is written by
    the split route (the origins) and by nothing else.  A split-size area computed for too small an out_bytes -- one byte of room
    short -- takes the run decoder for every run: the same results, nothing beyond the burst size written, the guard intact."""
    sc, data, in_off, in_len, ch, off, total, outs, status, hists = _burst_case()
    n = len(outs)
    want = H.expected_buffer(off, outs, total)
    want_slots = _slot_rows(hists, _slot_rows(sc.slots))
    small = lzs.channels_burst_work_bytes(n, sc.nch)
    rooms_sum = int(off[n] - off[0])

    def beyond_written(out_bytes):
        need = small if out_bytes is None else lzs.channels_burst_packed_split_work_bytes(n, sc.nch, out_bytes)
        whole = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        states = torch.from_numpy(_slot_rows(sc.slots)).cuda()
        buf = torch.full((GUARD + 1 + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        _, out_len, st = lzs.decompress_channels_burst_packed(data, in_off, ch, states, buf[GUARD + 1:GUARD + 1 + total],
                                                              torch.from_numpy(off).cuda(), in_len=in_len, work=whole[:need])
        torch.cuda.synchronize()
        H.compare(f"out_bytes {out_bytes}", buf.cpu().numpy(), out_len.cpu().numpy(), st.cpu().numpy(), want, outs, status, off)
        assert np.array_equal(states.cpu().numpy(), want_slots), out_bytes
        assert bool((whole[need:] == FILL).all()), f"out_bytes {out_bytes}: bytes behind the work area were written"
        return bool((whole[small:need] != FILL).any().item())

    monkeypatch.setenv("LZS_BURST_SPLIT_MIN", "0")
    assert beyond_written(rooms_sum), "every run split: the origins were not written"
    assert not beyond_written(rooms_sum - 1), "origins for one byte less than the rooms: no run may be split"
    assert not beyond_written(rooms_sum // 2)
    assert not beyond_written(None)
    monkeypatch.setenv("LZS_BURST_SPLIT_MIN", str(1 << 30))
    assert not beyond_written(rooms_sum), "a threshold above every run: nothing beyond the burst size may be written"
    monkeypatch.delenv("LZS_BURST_SPLIT_MIN")
    assert beyond_written(rooms_sum), "the default threshold splits the run of 600 packets"


@pytest.mark.parametrize("route", ("run", "split 0"))
def test_packets_of_one_trip_more_than_4_gib_apart(monkeypatch, route):
    """Two packets of one channel and two of another, first and second of their runs, lie more than 4 GiB apart in one input buffer,
    crosswise: each trip of the run decoder has packets whose extent exceeds 32 bits, so its groups take turns within the trip.
    The large tensor is never filled."""
    far = 5 << 30
    try:
        space = torch.empty(far + 8192, dtype=torch.uint8, device="cuda")
    except RuntimeError:
        pytest.skip("the device cannot allocate 5 GiB")
    rng = np.random.default_rng(77)
    hists = [M.random_hist(rng, 300), M.random_hist(rng, 2047), b""]
    packets = [M.synth(rng, 400), M.synth(rng, 300), M.synth_exact(rng, 2049), M.synth(rng, 200), M.synth(rng, 100)]
    ids = np.array([0, 1, 1, 0, 2])
    at = [67, far + 33, 1029, far + 2050, 4000]                   # trip 0: packets 0 and 1, trip 1: packets 3 and 2 -- both far apart
    for a, p in zip(at, packets):
        space[a:a + len(p)] = torch.from_numpy(np.frombuffer(p, dtype=np.uint8).copy()).cuda()
    rooms = [len(O.decompress_channel(b"", p, 1 << 30)[0]) for p in packets]
    rooms[3] = max(rooms[3] - 1, 0)
    outs, status, after = _model(packets, ids, hists, rooms, {})
    off, total = H.lay_out(rooms)
    before = _slot_rows(hists)
    states = torch.from_numpy(before).cuda()
    buf = torch.full((GUARD + 1 + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    work, behind, _ = _work(route, monkeypatch, 5, 3, total)
    _, out_len, st = lzs.decompress_channels_burst_packed(space, torch.tensor(at, dtype=torch.int64, device="cuda"),
                                                          torch.tensor(ids, dtype=torch.int32, device="cuda"), states,
                                                          buf[GUARD + 1:GUARD + 1 + total], torch.from_numpy(off).cuda(),
                                                          in_len=torch.tensor([len(p) for p in packets], dtype=torch.int32, device="cuda"),
                                                          work=work)
    torch.cuda.synchronize()
    H.compare(f"far apart, {route}", buf.cpu().numpy(), out_len.cpu().numpy(), st.cpu().numpy(), H.expected_buffer(off, outs, total), outs,
              status, off)
    assert bool((behind == FILL).all())
    assert np.array_equal(states.cpu().numpy(), _slot_rows(after, before))


def test_graph_capture_equals_the_direct_call(monkeypatch):
    """The call captured into a graph (split-size work area, some runs on either side of the threshold) and replayed on new packets
    gives what the direct call gives, slots included."""
    monkeypatch.setenv("LZS_BURST_SPLIT_MIN", "3000")
    sc = M.burst_scenario()
    n = min(len(packets) for packets, _ in sc.rounds)
    size = max(sum(len(p) for p in packets) for packets, _ in sc.rounds) + 16
    rounds = []
    for packets, ids in sc.rounds:
        data, in_off, in_len = H.place(torch, list(packets[:n]), True)
        rounds.append((torch.cat([data, torch.zeros(size - data.numel(), dtype=torch.uint8, device="cuda")]), in_off, in_len,
                       torch.tensor(np.asarray(ids[:n], dtype=np.int64).astype(np.int32), dtype=torch.int32, device="cuda")))
    room_off = lzs.offsets_from_sizes(torch.full((n,), 4096, dtype=torch.int32, device="cuda"), 1)
    total = 4096 * n
    before = _slot_rows(sc.slots)
    direct_states = torch.from_numpy(before).cuda()
    direct = []
    for data, in_off, in_len, ch in rounds:
        out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        _, ol, st = lzs.decompress_channels_burst_packed(data, in_off, ch, direct_states, out, room_off, in_len=in_len)
        direct.append((out, ol.clone(), st.clone()))
    data, in_off, in_len, ch = (t.clone() for t in rounds[0])
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    out_len = torch.empty(n, dtype=torch.int32, device="cuda")
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    work = torch.empty(lzs.channels_burst_packed_split_work_bytes(n, sc.nch, total), dtype=torch.uint8, device="cuda")
    scratch = torch.from_numpy(before).cuda()                      # a call outside the graph first: the library's start-up
    lzs.decompress_channels_burst_packed(data, in_off, ch, scratch, out, room_off, in_len=in_len, out_len=out_len, status=status, work=work)
    torch.cuda.synchronize()
    graph_states = torch.from_numpy(before).cuda()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lzs.decompress_channels_burst_packed(data, in_off, ch, graph_states, out, room_off, in_len=in_len, out_len=out_len, status=status,
                                             work=work)
    for r, src in enumerate(rounds):
        for mine, theirs in zip((data, in_off, in_len, ch), src):
            mine.copy_(theirs)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_len, direct[r][1]) and torch.equal(status, direct[r][2]), r
        keep = torch.arange(4096, device="cuda")[None, :] < out_len[:, None]
        assert torch.equal(out.view(n, 4096) * keep, direct[r][0].view(n, 4096) * keep), r
    assert torch.equal(graph_states, direct_states)


def test_decompress_channels_dense_allocates_exactly_the_total():
    """Whole packets of the burst compressor through decompress_channels_dense on peer states: the packets back to back in a tensor
    of exactly their total, the offsets their scan, the peer's slots the compressor's; a packet without its end marker is named."""
    import test_channel_encode_model as E
    sc = E.burst_scenario(long_run=40, out_of_range=False)
    enc = torch.from_numpy(_slot_rows(sc.slots)).cuda()
    dec = torch.from_numpy(_slot_rows(sc.slots)).cuda()
    for r, ((packets, ids), m) in enumerate(zip(sc.rounds, sc.modelled(None))):
        data, in_off, in_len = H.place(torch, packets, bool(r % 2))
        ch = torch.tensor(np.asarray(ids, dtype=np.int64).astype(np.int32), dtype=torch.int32, device="cuda")
        streams, offsets, _ = lzs.compress_channels_dense(data, in_off, ch, enc, in_len=in_len)
        good = m.status != E.ERROR
        # (the packets of the slot that is no state arrive as empty streams, which end in no marker: left out of the queue)
        keep = np.nonzero(good)[0]
        sel_off = offsets[torch.from_numpy(keep).cuda()].contiguous()
        sel_len = (offsets[1:] - offsets[:-1])[torch.from_numpy(keep).cuda()].to(torch.int32).contiguous()
        dense, out_off, status = lzs.decompress_channels_dense(streams, sel_off, ch[torch.from_numpy(keep).cuda()].contiguous(), dec,
                                                               in_len=sel_len)
        torch.cuda.synchronize()
        sent = [packets[b] for b in keep]
        assert dense.numel() == sum(len(p) for p in sent) and dense.cpu().numpy().tobytes() == b"".join(sent), r
        assert out_off.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(p) for p in sent])]).tolist(), r
        assert bool((status == A.STATUS_END_MARKER).all()), r
        assert torch.equal(dec, enc), r
    short = sel_len[:2].clone()
    short[1] -= 1                                                  # (a stream's last byte holds a bit of its marker)
    with pytest.raises(ValueError, match="packet 1 does not end in an end marker"):
        lzs.decompress_channels_dense(streams, sel_off[:2].contiguous(), ch[torch.from_numpy(keep[:2]).cuda()].contiguous(), dec.clone(),
                                      in_len=short)
