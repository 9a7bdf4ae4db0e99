"""lzs_decompress_channels_packed_device against the plain CPU model of the channel decoder (oracle/lzs_oracle.c:
lzs_oracle_decompress_channel): the packets and starting histories of tests/test_gpu_channel_model.py's scenarios, synthesised
token by token (tests/test_channel_model.py), decoded from packed packets to packed outputs over three successive calls on the
same states.  Every packet's bytes, length and status, every slot after every call, and the 0xA5 around every output are
compared with the model -- never with another decoder of the library."""
import numpy as np
import pytest

import lzs_compression_amd as lzs
from lzs_compression_amd import api as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_channel_model as M  # noqa: E402
from test_channel_model import O  # noqa: E402
from test_gpu_channel_model import _slot_rows  # noqa: E402

GUARD, FILL = 64, 0xA5


def _rooms(n, cap, spread):
    """Packet b's room: `cap`, and with `spread` up to 16 bytes more, so that the outputs start at every residue mod 16."""
    return [cap + (b * 7 % 17 if spread else 0) for b in range(n)]


def _model(packets, ids, hists, rooms):
    """test_channel_model.run_model with a room of its own for every packet."""
    hists = list(hists)
    outs, status, before = [], [], []
    for data, c, room in zip(packets, ids, rooms):
        h = hists[c]
        before.append(h)
        if h is None:
            outs.append(b"")
            status.append(A.STATUS_ERROR)
            continue
        out, st, hists[c] = O.decompress_channel(h, data, room)
        outs.append(out)
        status.append(st)
    return outs, np.array(status, dtype=np.uint8), before, hists


def _place(packets, with_len):
    """The packets back to back, the first byte one byte behind an aligned address; with lengths they lie in reverse order."""
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
    in_len = torch.tensor([len(p) for p in packets], dtype=torch.int32, device="cuda") if with_len else None
    return flat[1:1 + at], in_off, in_len


def _crosses_the_border(hist, packet, room):
    """Does a copy of this packet start in the history and end in the packet's own output?"""
    _, _, _, tokens, _ = O.decompress_channel(hist, packet, room, trace=True)
    return any(off > pos and off < pos + length for pos, off, length, _ in (t.tolist() for t in tokens) if length)


def _run(sc, cap, spread, channels_given):
    hists = sc.slots
    before = _slot_rows(hists)
    states = torch.from_numpy(before).cuda()
    crossing = set()
    for r, (packets, ids) in enumerate(sc.rounds):
        n = len(packets)
        if not channels_given:                                     # d_channel NULL: packet b is channel b's
            ids = np.arange(n)
        rooms = _rooms(n, cap, spread)
        outs, status, started, hists = _model(packets, ids, hists, rooms)
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum(rooms)
        total = int(off[-1])
        data, in_off, in_len = _place(packets, with_len=bool(r % 2))
        buf = torch.full((GUARD + 1 + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        ch = torch.tensor(np.asarray(ids), dtype=torch.int32, device="cuda") if channels_given else None
        _, out_len, st = lzs.decompress_channels_packed(data, in_off, ch, states, buf[GUARD + 1:GUARD + 1 + total],
                                                        torch.from_numpy(off).cuda(), in_len=in_len)
        torch.cuda.synchronize()
        tag = f"{sc.name}, capacity {cap}{' and up to 16 more' if spread else ''}, round {r}, channels {'given' if channels_given else 'NULL'}"
        want = np.full(buf.shape[0], FILL, dtype=np.uint8)
        for b, w in enumerate(outs):
            want[GUARD + 1 + off[b]:GUARD + 1 + off[b] + len(w)] = np.frombuffer(w, dtype=np.uint8)
        got_len, got_st, got = out_len.cpu().numpy(), st.cpu().numpy(), buf.cpu().numpy()
        want_len = np.array([len(w) for w in outs])
        bad = np.nonzero((got_len != want_len) | (got_st != status))[0]
        assert not bad.size, (tag, bad[:5].tolist(), got_len[bad[:5]].tolist(), want_len[bad[:5]].tolist(), got_st[bad[:5]].tolist(),
                              status[bad[:5]].tolist(), [started[b] is None for b in bad[:5]])
        diff = np.nonzero(got != want)[0]
        if diff.size:
            i = int(diff[0]) - GUARD - 1
            b = int(np.searchsorted(off, i, side="right")) - 1
            raise AssertionError(f"{tag}: {diff.size} bytes differ, the first at d_out[{i}] (packet {b} at {int(off[max(b, 0)])}, length "
                                 f"{int(want_len[max(b, 0)])}, hist_len {len(started[max(b, 0)] or b'')}): "
                                 f"{got[diff[0]:diff[0] + 8].tobytes().hex()}, the model {want[diff[0]:diff[0] + 8].tobytes().hex()}")
        before = _slot_rows(hists, before)
        s = states.cpu().numpy()
        rows = np.nonzero((s != before).any(axis=1))[0]
        assert not rows.size, (tag, "slots differ", rows[:5].tolist(), [int(s[c, :4].view("<u4")[0]) for c in rows[:5]],
                               [len(hists[c] or b"") for c in rows[:5]])
        if spread:
            crossing |= {int(off[b]) % 16 for b in range(n) if started[b] is not None and _crosses_the_border(started[b], packets[b], rooms[b])}
    return crossing


@pytest.mark.parametrize("n", (1, 65, 257))
def test_three_calls_on_the_same_states(n):
    """1, 65 and 257 packets (the grouping of eight streams per wavefront), compressed lengths 0, 2, 40 and 3000 side by side,
    a slot with hist_len 4000 (ERROR, the slot untouched), at the scenario's capacities -- roomy, 100, 1, 0 -- as every
    packet's room, d_channel given."""
    sc = M.single_scenario(n)
    assert n == 1 or any(h is None for h in sc.slots)
    for cap in sc.caps:
        _run(sc, cap, False, True)


def test_without_channel_ids():
    """d_channel NULL: packet b on channel b."""
    sc = M.single_scenario(65)
    for cap in (sc.caps[0], 100):
        _run(sc, cap, False, False)


def test_copies_across_the_border_at_every_output_alignment():
    """Rooms of the capacity and up to 16 bytes more: the outputs start at every residue mod 16, and at every one of them some
    packet has a copy that begins in its channel's history and ends in its own output."""
    sc = M.single_scenario(257)
    crossing = _run(sc, sc.caps[0], True, True)
    assert crossing == set(range(16)), sorted(crossing)
    _run(sc, 100, True, True)


def test_a_slot_with_hist_len_2048():
    """The smallest hist_len that is no state: ERROR, length 0, nothing written, the slot as it was; its neighbours in the same
    wavefront decode as the model says."""
    rng = np.random.default_rng(48)
    packets = M.synth_batch(rng, 9)
    hists = M.start_slots(rng, 9)
    before = _slot_rows(hists)
    before[4] = 0x77
    before[4, :4] = (0x00, 0x08, 0, 0)                              # hist_len 2048
    states = torch.from_numpy(before).cuda()
    hists[4] = None
    rooms = _rooms(9, max(M.true_sizes(packets)) + 1, True)
    outs, status, _, after = _model(packets, np.arange(9), hists, rooms)
    assert status[4] == A.STATUS_ERROR and outs[4] == b""
    off = np.zeros(10, dtype=np.int64)
    off[1:] = np.cumsum(rooms)
    data, in_off, _ = _place(packets, with_len=False)
    buf = torch.full((GUARD + 1 + int(off[-1]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    _, out_len, st = lzs.decompress_channels_packed(data, in_off, None, states, buf[GUARD + 1:GUARD + 1 + int(off[-1])], torch.from_numpy(off).cuda())
    torch.cuda.synchronize()
    want = np.full(buf.shape[0], FILL, dtype=np.uint8)
    for b, w in enumerate(outs):
        want[GUARD + 1 + off[b]:GUARD + 1 + off[b] + len(w)] = np.frombuffer(w, dtype=np.uint8)
    assert out_len.cpu().numpy().tolist() == [len(w) for w in outs] and st.cpu().numpy().tolist() == status.tolist()
    assert np.array_equal(buf.cpu().numpy(), want)
    want_slots = _slot_rows(after, before)
    want_slots[4] = before[4]
    assert np.array_equal(states.cpu().numpy(), want_slots)
