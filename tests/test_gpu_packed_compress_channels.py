"""lzs_compress_channels_packed_device against the plain CPU model of channel compression (oracle/lzs_oracle.c:
lzs_oracle_compress_channel): the packets and starting histories of tests/test_channel_encode_model.py's one-packet scenarios,
compressed from packed packets to packed rooms over three successive calls on the same states.  Every packet's room is chosen
from the model -- its uncut total T (status 0x07) or T - 1 (0x0B) --, so every byte of d_out is determined: the whole buffer with
its guards, every length, every status and every slot after every call are compared with the model.  One slot has hist_len 2048
and one entry of every call is not a block: ERROR, length 0, the slot identical.  Then every call's packed output goes through
lzs_decompress_channels_packed_device on peer states, which gives the packets back."""
import numpy as np
import pytest

import lzs_compression_amd as lzs
from lzs_compression_amd import api as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_channel_encode_model as M  # noqa: E402
from test_channel_encode_model import O  # noqa: E402
from test_gpu_channel_model import _slot_rows  # noqa: E402

GUARD, FILL = 64, 0xA5
BLOCK_MAX = 3 << 30


def _slots(hists, before=None):
    """_slot_rows, with hist_len 2048 -- the first length that is no state -- in the slots that are none."""
    s = _slot_rows(hists, before)
    for c, h in enumerate(hists):
        if h is None:
            s[c, :4] = np.frombuffer((2048).to_bytes(4, "little"), dtype=np.uint8)
    return s


def _model(packets, ids, hists, room_of, skip, r):
    """The model over call `r` with a room of its own for every packet: room_of(b + r, T) from the packet's uncut total.  Packet
    `skip` is not a block and a history of None is no state: ERROR, nothing written, nothing changed."""
    hists = list(hists)
    outs, status, rooms = [], [], []
    for b, (data, c) in enumerate(zip(packets, ids)):
        h = hists[c]
        if h is None or b == skip:
            outs.append(b"")
            status.append(A.STATUS_ERROR)
            rooms.append(3 if b == skip else 5)                    # (a room that must stay 0xA5)
            continue
        total = O.compress_channel(h, data)[1]
        room = room_of(b + r, total)
        out, total2, st, hists[c] = O.compress_channel(h, data, room)
        assert total2 == total and st == (M.DONE if total <= room else M.CUT) and len(out) == min(total, room)
        outs.append(out)
        status.append(st)
        rooms.append(room)
    return outs, np.array(status, dtype=np.uint8), rooms, hists


def _place(packets, with_len, skip):
    """The packets back to back, the first byte one byte behind an aligned address; with lengths they lie in reverse order, and
    packet `skip` claims more than LZS_BLOCK_MAX bytes."""
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
        if skip is not None:
            lens[skip] = BLOCK_MAX + 1
        in_len = torch.from_numpy(lens.view(np.int32).copy()).cuda()
    return flat[1:1 + at], in_off, in_len


def _lay_out(rooms, decreasing):
    """out_off for these rooms.  `decreasing`: that entry's pair of offsets decreases -- the entries before it lie in an upper part
    of d_out, its pair leads from there back to 0, the entries after it lie in the lower part, and no two rooms overlap."""
    if decreasing is None:
        off = np.concatenate([[0], np.cumsum(rooms)]).astype(np.int64)
        return off, int(off[-1])
    low = np.concatenate([[0], np.cumsum(rooms[decreasing + 1:])]).astype(np.int64)
    high = int(low[-1]) + 3 + np.concatenate([[0], np.cumsum(rooms[:decreasing])]).astype(np.int64)
    return np.concatenate([high, low]), int(high[-1])


def _run(sc, room_of, decode):
    hists = sc.slots
    before = _slots(hists)
    states = torch.from_numpy(before).cuda()
    peers = torch.from_numpy(before).cuda()
    seen = set()
    for r, (packets, ids) in enumerate(sc.rounds):
        n = len(packets)
        with_len = bool(r % 2)
        skip = min(2, n - 1) if n > 1 or r == 1 else None          # (the batch of one packet: its only entry, in one of the calls)
        outs, status, rooms, hists = _model(packets, ids, hists, room_of, skip, r)
        # the entry that is not a block: a length above LZS_BLOCK_MAX where there are lengths, a decreasing pair in out_off otherwise
        off, total = _lay_out(rooms, None if with_len else skip)
        if skip is not None and not with_len:
            rooms[skip] = 0
        data, in_off, in_len = _place(packets, with_len, skip)
        buf = torch.full((GUARD + 1 + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        out = buf[GUARD + 1:GUARD + 1 + total]
        out_off = torch.from_numpy(off).cuda()
        ch = torch.tensor(np.asarray(ids), dtype=torch.int32, device="cuda")
        _, out_len, st = lzs.compress_channels_packed(data, in_off, ch, states, out, out_off, in_len=in_len)
        torch.cuda.synchronize()
        tag = f"{sc.name}, round {r}, {'lengths given' if with_len else 'no lengths'}, entry {skip} not a block"
        want = np.full(buf.shape[0], FILL, dtype=np.uint8)
        for b, w in enumerate(outs):
            want[GUARD + 1 + off[b]:GUARD + 1 + off[b] + len(w)] = np.frombuffer(w, dtype=np.uint8)
        got_len, got_st, got = out_len.cpu().numpy(), st.cpu().numpy(), buf.cpu().numpy()
        want_len = np.array([len(w) for w in outs])
        bad = np.nonzero((got_len != want_len) | (got_st != status))[0]
        assert not bad.size, (tag, bad[:5].tolist(), got_len[bad[:5]].tolist(), want_len[bad[:5]].tolist(), got_st[bad[:5]].tolist(),
                              status[bad[:5]].tolist())
        diff = np.nonzero(got != want)[0]
        if diff.size:
            i = int(diff[0]) - GUARD - 1
            b = int(np.argmax([int(off[k]) <= i < int(off[k]) + max(rooms[k], 1) for k in range(n)]))
            raise AssertionError(f"{tag}: {diff.size} bytes differ, the first at d_out[{i}] (near packet {b} at {int(off[b])}, length "
                                 f"{int(want_len[b])}, room {rooms[b]}): {got[diff[0]:diff[0] + 8].tobytes().hex()}, the model "
                                 f"{want[diff[0]:diff[0] + 8].tobytes().hex()}")
        before = _slots(hists, before)
        s = states.cpu().numpy()
        rows = np.nonzero((s != before).any(axis=1))[0]
        assert not rows.size, (tag, "slots differ", rows[:5].tolist(), [int(s[c, :4].view("<u4")[0]) for c in rows[:5]],
                               [len(hists[c] or b"") for c in rows[:5]])
        seen |= set(status.tolist())
        if decode:
            # the peer: the rooms as packed packets (their lengths say how much of each room is stream), decoded to rooms of
            # the packets' sizes; an ERROR entry arrives as an empty packet, which decodes to nothing and changes nothing
            plain = [len(p) if status[b] != A.STATUS_ERROR else 0 for b, p in enumerate(packets)]
            dec_off = np.concatenate([[0], np.cumsum(plain)]).astype(np.int64)
            back = torch.full((int(dec_off[-1]) + 1,), FILL, dtype=torch.uint8, device="cuda")
            _, back_len, back_st = lzs.decompress_channels_packed(out, out_off, ch, peers, back[:int(dec_off[-1])], torch.from_numpy(dec_off).cuda(),
                                                                  in_len=out_len)
            torch.cuda.synchronize()
            assert back_len.cpu().numpy().tolist() == plain, tag
            sent = b"".join(p for b, p in enumerate(packets) if status[b] != A.STATUS_ERROR)
            assert back.cpu().numpy().tobytes() == sent + bytes([FILL]), tag
            good = back_st.cpu().numpy()[status != A.STATUS_ERROR]
            assert (good == A.STATUS_END_MARKER).all(), (tag, good[:10].tolist())
            assert np.array_equal(peers.cpu().numpy(), s), (tag, "the peer's slots differ from the compressor's")
    return seen


@pytest.mark.parametrize("n", M.SINGLE_BATCHES)
def test_three_calls_with_rooms_of_the_total_and_one_less(n):
    """1, 64, 257 and 1500 packets on carried slots; two rooms in three are the model's uncut total (0x07), the third one byte less
    (0x0B: the history advances all the same); a slot with hist_len 2048, an entry that is not a block in every call."""
    sc = M.single_scenario(n)
    assert n == 1 or any(h is None for h in sc.slots)
    seen = _run(sc, lambda k, total: total - (k % 3 == 2), decode=False)
    assert {M.DONE, M.CUT} <= seen and (n == 1 or M.ERROR in seen)


def test_packets_of_one_length():
    sc = M.uniform_scenario()
    _run(sc, lambda k, total: total - (k % 3 == 2), decode=False)


@pytest.mark.parametrize("n", (1, 257))
def test_the_peer_recovers_the_packets(n):
    """Every room the model's total: all 0x07, and decompress_channels_packed on peer states gives every packet back, call after
    call, with slots equal to the compressor's."""
    _run(M.single_scenario(n), lambda k, total: total, decode=True)
