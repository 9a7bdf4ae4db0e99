"""lzs_compress_channels_burst_packed_device against the plain CPU model of channel compression (oracle/lzs_oracle.c:
lzs_oracle_compress_channel), applied packet by packet in row order per channel with each packet's own room -- the header's
rank-by-rank definition.  The rounds of tests/test_channel_encode_model.py's burst scenarios (runs of 1, 2, 13 and 600, interleaved
ids, zero-length packets first, in the middle and last in a run, earlier packets of 2046, 2047 and 2048 bytes behind a 2047-byte
slot history, 2100 one-byte packets on one channel, a slot that is no state, ids out of range) on the same states, the packets
placed back to back one byte behind an aligned address, with and without d_in_len (in reverse order where there are lengths).
Every room is the model's uncut total T (0x07) or T - 1 (0x0B), so every byte of d_out is determined: the whole buffer with its
guards, every length, every status and every slot are compared.  Every round has entries that are not blocks, of both kinds, first,
in the middle and last in a run, and one channel all of whose packets are none and whose slot holds junk behind hist_len."""
import numpy as np
import pytest

import lzs_compression_amd as lzs
from lzs_compression_amd import api as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import packed_burst_helpers as H  # noqa: E402
import test_channel_encode_model as M  # noqa: E402
from packed_burst_helpers import FILL, GUARD  # noqa: E402
from test_channel_encode_model import O  # noqa: E402
from test_gpu_channel_model import _slot_rows  # noqa: E402

SCENARIOS = {"burst": M.burst_scenario, "one byte": M.one_byte_scenario}


def _model(packets, ids, hists, room_of, skip, r):
    """The model over round `r`: packet b's room is room_of(b + r, T) from its uncut total T.  The entries in `skip` are not
    blocks, a history of None is no state and an id outside the slots names no channel: ERROR, nothing written, nothing changed."""
    hists = list(hists)
    outs, status, rooms = [], [], []
    for b, (data, c) in enumerate(zip(packets, ids)):
        c = int(c)
        if b in skip or not H.valid(c, hists):
            outs.append(b"")
            status.append(A.STATUS_ERROR)
            rooms.append(3 if b in skip else 5)                    # (a room that must stay 0xA5)
            continue
        total = O.compress_channel(hists[c], data)[1]
        room = room_of(b + r, total)
        out, total2, st, hists[c] = O.compress_channel(hists[c], data, room)
        assert total2 == total and st == (M.DONE if total <= room else M.CUT) and len(out) == min(total, room)
        outs.append(out)
        status.append(st)
        rooms.append(room)
    return outs, np.array(status, dtype=np.uint8), rooms, hists


def _work(n, nch):
    """A work area of exactly channels_burst_work_bytes() bytes and a guard behind it."""
    need = lzs.channels_burst_work_bytes(n, nch)
    whole = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 256 == 0
    return whole[:need], whole[need:]


def _run(sc, room_of, first_with_len, decode):
    hists = list(sc.slots)
    _, chan_b = H.special_channels(sc)
    before = _slot_rows(hists)
    junk = H.junk_slot(before, chan_b, hists[chan_b])
    states = torch.from_numpy(before).cuda()
    peers = torch.from_numpy(before).cuda()
    seen = set()
    for r, (packets, ids) in enumerate(sc.rounds):
        n = len(packets)
        with_len = bool((r + first_with_len) % 2)
        skip = H.not_blocks(sc, r, with_len)
        assert skip and {"pair"} <= set(skip.values()) and (not with_len or "length" in skip.values())
        outs, status, rooms, hists = _model(packets, ids, hists, room_of, skip, r)
        pairs = {b for b, kind in skip.items() if kind == "pair"}
        off, total = H.lay_out(rooms, pairs)
        data, in_off, in_len = H.place(torch, packets, with_len, [b for b, kind in skip.items() if kind == "length"])
        buf = torch.full((GUARD + 1 + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        out = buf[GUARD + 1:GUARD + 1 + total]
        out_off = torch.from_numpy(off).cuda()
        ch = torch.tensor(np.asarray(ids, dtype=np.int64).astype(np.int32), dtype=torch.int32, device="cuda")
        work, behind = _work(n, sc.nch)
        _, out_len, st = lzs.compress_channels_burst_packed(data, in_off, ch, states, out, out_off, in_len=in_len, work=work)
        torch.cuda.synchronize()
        tag = f"{sc.name}, round {r}, {'lengths given, reverse order' if with_len else 'no lengths'}, {len(skip)} entries not blocks"
        H.compare(tag, buf.cpu().numpy(), out_len.cpu().numpy(), st.cpu().numpy(), H.expected_buffer(off, outs, total), outs, status, off)
        assert bool((behind == FILL).all()), f"{tag}: bytes behind the work area were written"
        before = _slot_rows(hists, before)
        before[chan_b] = junk
        s = states.cpu().numpy()
        rows = np.nonzero((s != before).any(axis=1))[0]
        assert not rows.size, (tag, "slots differ", rows[:5].tolist(), [int(s[c, :4].view("<u4")[0]) for c in rows[:5]],
                               [len(hists[c] or b"") for c in rows[:5]])
        assert np.array_equal(s[chan_b], junk), f"{tag}: the slot of the channel whose packets are all not blocks was touched"
        seen |= set(status.tolist())
        if decode:
            # the peer: the rooms as packed packets (their lengths say how much of each room is stream), decoded to rooms of the
            # packets' sizes; the entries that were not blocks are none here either (decreasing pairs), so that the peer's slots
            # see what the compressor's saw
            good = status != A.STATUS_ERROR
            plain = [len(p) if good[b] else 0 for b, p in enumerate(packets)]
            dec_off, dec_total = H.lay_out(plain, set(skip))
            back = torch.full((GUARD + 1 + dec_total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            dwork = torch.empty(lzs.channels_burst_packed_split_work_bytes(n, sc.nch, dec_total), dtype=torch.uint8, device="cuda")
            _, back_len, back_st = lzs.decompress_channels_burst_packed(out, out_off, ch, peers, back[GUARD + 1:GUARD + 1 + dec_total],
                                                                        torch.from_numpy(dec_off).cuda(), in_len=out_len, work=dwork)
            torch.cuda.synchronize()
            sent = [p if good[b] else b"" for b, p in enumerate(packets)]
            want_st = np.where(good, A.STATUS_END_MARKER, A.STATUS_ERROR).astype(np.uint8)
            H.compare(tag + ", the peer", back.cpu().numpy(), back_len.cpu().numpy(), back_st.cpu().numpy(),
                      H.expected_buffer(dec_off, sent, dec_total), sent, want_st, dec_off)
            assert np.array_equal(peers.cpu().numpy(), s), (tag, "the peer's slots differ from the compressor's")
    return seen


@pytest.mark.parametrize("first_with_len", (0, 1))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_rooms_of_the_total_and_one_less(name, first_with_len):
    """Two rooms in three are the model's uncut total (0x07), the third one byte less (0x0B: the history advances all the same)."""
    seen = _run(SCENARIOS[name](), lambda k, total: total - (k % 3 == 2), first_with_len, decode=False)
    assert {M.DONE, M.CUT, M.ERROR} <= seen


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_the_peer_recovers_the_packets(name):
    """Every room the model's total: all 0x07, and decompress_channels_burst_packed on peer states gives every packet back, round
    after round, with slots equal to the compressor's."""
    _run(SCENARIOS[name](), lambda k, total: total, 1, decode=True)


def test_compress_channels_dense_gives_the_models_streams():
    """The whole sequence -- bounds, offsets, rooms, burst, compaction -- on the burst scenario: the dense string is the model's
    streams back to back, the offsets their scan, the slots the model's."""
    sc = M.burst_scenario()
    before = _slot_rows(sc.slots)
    states = torch.from_numpy(before).cuda()
    for r, ((packets, ids), m) in enumerate(zip(sc.rounds, sc.modelled(None))):
        data, in_off, in_len = H.place(torch, packets, bool(r % 2))
        ch = torch.tensor(np.asarray(ids, dtype=np.int64).astype(np.int32), dtype=torch.int32, device="cuda")
        dense, offsets, status = lzs.compress_channels_dense(data, in_off, ch, states, in_len=in_len)
        torch.cuda.synchronize()
        assert offsets.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(w) for w in m.outs])]).tolist(), r
        assert dense.cpu().numpy().tobytes() == b"".join(m.outs), r
        assert np.array_equal(status.cpu().numpy(), m.status), r
        before = _slot_rows(m.hists, before)
        assert np.array_equal(states.cpu().numpy(), before), r


def test_graph_capture_equals_the_direct_call():
    """The call captured into a graph and replayed on new packets gives what the direct call gives, slots included."""
    sc = M.burst_scenario()
    before = _slot_rows(sc.slots)
    rounds = []
    sizes = [sum(len(p) for p in packets) for packets, _ in sc.rounds]
    n = min(len(packets) for packets, _ in sc.rounds)
    for packets, ids in sc.rounds:                                 # the same number of packets and bytes in both rounds
        packets = list(packets[:n])
        data, in_off, in_len = H.place(torch, packets, True)
        pad = torch.zeros(max(sizes) + 16 - data.numel(), dtype=torch.uint8, device="cuda")
        rounds.append((torch.cat([data, pad]), in_off, in_len, torch.tensor(np.asarray(ids[:n], dtype=np.int64).astype(np.int32),
                                                                            dtype=torch.int32, device="cuda")))
    bound = lzs.compressed_bounds_packed(rounds[0][1], rounds[0][2])
    room_off = lzs.offsets_from_sizes(torch.full_like(bound, int(A.compressed_max(M.MAX_PACKET))), 16)
    total = int(room_off[-1].cpu())
    direct_states = torch.from_numpy(before).cuda()
    direct = []
    for data, in_off, in_len, ch in rounds:
        out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        _, ol, st = lzs.compress_channels_burst_packed(data, in_off, ch, direct_states, out, room_off, in_len=in_len)
        direct.append((out, ol.clone(), st.clone()))
    data, in_off, in_len, ch = (t.clone() for t in rounds[0])
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    out_len = torch.empty(n, dtype=torch.int32, device="cuda")
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    work = torch.empty(lzs.channels_burst_work_bytes(n, sc.nch), dtype=torch.uint8, device="cuda")
    scratch = torch.from_numpy(before).cuda()                      # a call outside the graph first: the library's start-up
    lzs.compress_channels_burst_packed(data, in_off, ch, scratch, out, room_off, in_len=in_len, out_len=out_len, status=status, work=work)
    torch.cuda.synchronize()
    graph_states = torch.from_numpy(before).cuda()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lzs.compress_channels_burst_packed(data, in_off, ch, graph_states, out, room_off, in_len=in_len, out_len=out_len, status=status,
                                           work=work)
    for r, src in enumerate(rounds):
        for mine, theirs in zip((data, in_off, in_len, ch), src):
            mine.copy_(theirs)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_len, direct[r][1]) and torch.equal(status, direct[r][2]) and torch.equal(out, direct[r][0]), r
    assert torch.equal(graph_states, direct_states)
