"""History resets inside a burst (include/lzs/lzs_channels.h, LZS_PACKET_RESET): the four flags entries against the
plain CPU models of the channel decoder and compressor (oracle.oracle().decompress_channel / compress_channel), applied packet by
packet in row order per channel with ``hist = b""`` where the rule resets -- the header's rank-by-rank definition.  No expected value
comes from the library: every packet's bytes, length and status, every final slot in full, the 0xA5 fill behind every length and a
guard behind the work area are compared, none left out."""
import ctypes

import numpy as np
import pytest

import lzs_compression_amd as lzs
from lzs_compression_amd import api as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import packed_burst_helpers as H  # noqa: E402
import test_channel_model as M  # noqa: E402
from burst_flags_cases import _apply_rule, _check_slots, _reach_back, _want_slots  # noqa: E402
from packed_burst_helpers import FILL, GUARD  # noqa: E402
from test_channel_model import O  # noqa: E402

SLOT, HIST_AT = A.CHANNEL_STATE_BYTES, 64
NCH, OUTSIDE = 3, 7                     # three channels, and an id out of range
ROUTES = ("run", "split 0", "split default")
R = lzs.PACKET_RESET

# The queue, in interleaved order: (channel, flagged, what it is).  Channels 0 and 1 start with a full history of 2047 bytes,
# channel 2's slot is no state (hist_len 4000 over a 0x77 fill).  "not a block" is an entry of the packed calls only.
QUEUE = ((0, R, "first packet of a primed slot"), (1, 0, ""), (2, 0, "no state: ERROR"), (0, 0, ""), (OUTSIDE, R, "id out of range"),
         (1, R, "mid-run"), (2, R, "revives the slot"), (1, R, "two in a row"), (0, 0, ""), (1, R, "not a block"), (2, 0, ""), (1, 0, ""),
         (0, R, "produces nothing"), (2, 0, ""), (1, 0, ""))
NOT_A_BLOCK = next(b for b, q in enumerate(QUEUE) if q[2] == "not a block")
STRIDED = [b for b in range(len(QUEUE)) if b != NOT_A_BLOCK]


def _start_slots(rng):
    """[history or None] and the slots' bytes."""
    hists = [M.random_hist(rng, 2047), M.random_hist(rng, 2047), None]
    rows = np.zeros((NCH, SLOT), dtype=np.uint8)
    for c, h in enumerate(hists):
        if h is None:
            rows[c] = 0x77
            rows[c, :4] = (0xA0, 0x0F, 0, 0)
        else:
            rows[c, :4] = np.frombuffer(len(h).to_bytes(4, "little"), dtype=np.uint8)
            rows[c, HIST_AT:HIST_AT + len(h)] = np.frombuffer(h, dtype=np.uint8)
    return hists, rows


def _rows(packets):
    """The packets as rows of a device tensor with an odd stride."""
    n = len(packets)
    stride = (max(len(p) for p in packets) + 4) // 4 * 4 + 1
    host = np.random.default_rng(n).integers(0, 256, (n, stride), dtype=np.uint8)
    for b, p in enumerate(packets):
        host[b, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    return torch.from_numpy(host).cuda(), torch.tensor([len(p) for p in packets], dtype=torch.int32, device="cuda")


def _dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _route_env(route, monkeypatch):
    if route == "split 0":
        monkeypatch.setenv("LZS_BURST_SPLIT_MIN", "0")
    else:
        monkeypatch.delenv("LZS_BURST_SPLIT_MIN", raising=False)


def _work(need):
    whole = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 256 == 0
    return whole[:need], whole[need:]


def _check_strided(tag, got, outs, status):
    o, n, st = got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()
    want = np.full(o.shape, FILL, dtype=np.uint8)
    for b, w in enumerate(outs):
        want[b, :len(w)] = np.frombuffer(w, dtype=np.uint8)
    want_n = np.array([len(w) for w in outs])
    print(tag, "lengths", n.tolist(), "model", want_n.tolist(), "status", st.tolist(), "model", status.tolist())
    bad = np.nonzero((n != want_n) | (st != status) | (o != want).any(axis=1))[0]
    if bad.size:
        b = int(bad[0])
        diff = np.nonzero(o[b] != want[b])[0]
        raise AssertionError(f"{tag}: packets {bad.tolist()} differ; packet {b}: length {n[b]} (model {want_n[b]}), status {st[b]:#x} (model "
                             f"{status[b]:#x}), first differing byte {diff[:1].tolist()}: {o[b, diff[:1].sum():][:8].tobytes().hex()} "
                             f"(model {want[b, diff[:1].sum():][:8].tobytes().hex()})")


# ------------------------------------------------------------------ 1. the decoder against the model
def _decoder_queue():
    rng = np.random.default_rng(1974)
    packets = []
    for b, (c, flag, what) in enumerate(QUEUE):
        if what == "produces nothing":
            packets.append(M.to_bytes(M.MARKER))
        elif flag:
            packets.append(_reach_back(rng, int(rng.integers(40, 301))))
        else:
            packets.append(M.synth_exact(rng, int(rng.integers(0, 301))))
    return packets


def _decode_step(packets, rooms):
    return lambda b, hist: O.decompress_channel(hist, packets[b], rooms[b])


def test_the_decoder_queue_tells_a_reset_from_none():
    """On the model, before any device call: every flagged block of a channel in range decodes to other bytes from the empty
    history than from the history it would otherwise have (or to bytes where the channel would otherwise be no state)."""
    packets = _decoder_queue()
    hists, _ = _start_slots(np.random.default_rng(7))
    ids, flags = [q[0] for q in QUEUE], [q[1] for q in QUEUE]
    carried = list(hists)
    told = 0
    for b, c in enumerate(ids):
        if not 0 <= c < NCH or b == NOT_A_BLOCK:
            continue
        fresh = O.decompress_channel(b"", packets[b], 1 << 20)
        if flags[b] and QUEUE[b][2] != "produces nothing":
            other = None if carried[c] is None else O.decompress_channel(carried[c], packets[b], 1 << 20)[0]
            assert other != fresh[0] and len(fresh[0]) >= 24, (b, QUEUE[b])
            told += 1
        if flags[b]:
            carried[c] = b""
        if carried[c] is not None:
            carried[c] = O.decompress_channel(carried[c], packets[b], 1 << 20)[2]
    assert told == 4


@pytest.mark.parametrize("route", ROUTES)
def test_strided_decoder_equals_the_model(monkeypatch, route):
    allp = _decoder_queue()
    packets = [allp[b] for b in STRIDED]
    ids, flags = [QUEUE[b][0] for b in STRIDED], [QUEUE[b][1] for b in STRIDED]
    hists, before = _start_slots(np.random.default_rng(7))
    cap = max(M.true_sizes(packets)) + 1
    outs, status, final, touched = _apply_rule(_decode_step(packets, [cap] * len(packets)), ids, flags, hists)
    assert status[ids.index(2)] == A.STATUS_ERROR and (status[[b for b, c in enumerate(ids) if c == 2][1:]] == M.END).all()
    assert final[0] == b"" and len(final[1]) and len(final[2])
    n = len(packets)
    x, xl = _rows(packets)
    states = torch.from_numpy(before).cuda()
    out = torch.full((n, (cap + 15) // 16 * 16 + GUARD), FILL, dtype=torch.uint8, device="cuda")
    _route_env(route, monkeypatch)
    work, behind = _work(lzs.channels_burst_work_bytes(n, NCH) if route == "run" else lzs.channels_burst_split_work_bytes(n, NCH, cap))
    got = lzs.decompress_channels_burst(x, xl, _dev(ids, torch.int32), states, cap, out=out, work=work, flags=_dev(flags, torch.uint8))
    torch.cuda.synchronize()
    _check_strided(f"strided decode, {route}", got, outs, status)
    _check_slots(f"strided decode, {route}", states, _want_slots(before, final, touched))
    assert bool((behind == FILL).all()), "bytes behind the work area were written"


@pytest.mark.parametrize("route", ROUTES)
def test_packed_decoder_equals_the_model(monkeypatch, route):
    """The same queue with a flagged entry that is not a block (a decreasing pair of output offsets) in the middle of channel 1's
    run: the entry does nothing, its flag is ignored, and the packet behind it copies from the history the run had.  One flagged
    packet has a room that cuts its first copy: NO_OUTPUT_BUFFER_SPACE, and the history goes on with the five bytes it gave."""
    packets = _decoder_queue()
    ids, flags = [q[0] for q in QUEUE], [q[1] for q in QUEUE]
    hists, before = _start_slots(np.random.default_rng(7))
    rooms = M.true_sizes(packets)
    cut = next(b for b, q in enumerate(QUEUE) if q[2] == "two in a row")
    rooms[cut] = 5                                                  # (inside the flagged packet's first copy, of 8 bytes or more)
    off, total = H.lay_out(rooms, {NOT_A_BLOCK})
    rooms = [0 if b == NOT_A_BLOCK else int(off[b + 1] - off[b]) for b in range(len(packets))]
    outs, status, final, touched = _apply_rule(_decode_step(packets, rooms), ids, flags, hists, skip={NOT_A_BLOCK})
    assert status[cut] == M.FULL and outs[cut] == bytes(5)          # (cut as without a flag; the copy read the empty history's zeros)
    ignored = _apply_rule(_decode_step(packets, rooms), ids, [f if b != NOT_A_BLOCK else 0 for b, f in enumerate(flags)], hists, skip={NOT_A_BLOCK})
    assert outs == ignored[0]                                       # (the model of "ignored", stated twice)
    data, in_off, in_len = H.place(torch, packets, True)
    lead = GUARD + 1
    buf = torch.full((lead + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    states = torch.from_numpy(before).cuda()
    n = len(packets)
    _route_env(route, monkeypatch)
    work, behind = _work(lzs.channels_burst_work_bytes(n, NCH) if route == "run" else lzs.channels_burst_packed_split_work_bytes(n, NCH, total))
    _, out_len, st = lzs.decompress_channels_burst_packed(data, in_off, _dev(ids, torch.int32), states, buf[lead:lead + total],
                                                          torch.from_numpy(off).cuda(), in_len=in_len, work=work, flags=_dev(flags, torch.uint8))
    torch.cuda.synchronize()
    print("packed decode", route, "lengths", out_len.tolist(), "status", st.tolist(), "model", status.tolist())
    H.compare(f"packed decode, {route}", buf.cpu().numpy(), out_len.cpu().numpy(), st.cpu().numpy(), H.expected_buffer(off, outs, total, lead),
              outs, status, off, lead)
    _check_slots(f"packed decode, {route}", states, _want_slots(before, final, touched))
    assert bool((behind == FILL).all()), "bytes behind the work area were written"


# ------------------------------------------------------------------ 2. the compressor against the model
def _compress_queue():
    """Packets of real bytes: each repeats most of its channel's previous packet (the first: of the tail of the primed history), so
    that an unflagged packet is mostly matches into the history."""
    rng = np.random.default_rng(2395)
    text = lzs.workload.fill("text", NCH + 1, 4096)
    hists, before = _start_slots(rng)
    hists = [None if h is None else text[c, :2047].tobytes() for c, h in enumerate(hists)]
    for c, h in enumerate(hists):
        if h is not None:
            before[c, HIST_AT:HIST_AT + 2047] = np.frombuffer(h, dtype=np.uint8)
    last = {c: text[c if c < NCH else NCH, 1700:2047].copy() for c in (0, 1, 2, OUTSIDE)}
    packets = []
    for c, flag, what in QUEUE:
        if what == "produces nothing":
            packets.append(b"")
            continue
        p = last[c].copy()
        p[rng.integers(0, p.size, 6)] = rng.integers(0, 256, 6, dtype=np.uint8)     # a few bytes changed ...
        p = np.concatenate([p[int(rng.integers(0, 40)):], text[NCH, :int(rng.integers(0, 60))]])   # ... the front cut, a tail added
        last[c] = p
        packets.append(p.tobytes())
    return packets, hists, before


def _compress_step(packets, rooms):
    def step(b, hist):
        out, _, st, new = O.compress_channel(hist, packets[b], rooms[b])
        return out, st, new
    return step


def _cut_room(packets, flags, b):
    """A room three bytes short of what flagged packet b needs from an empty history."""
    assert flags[b]
    return O.compress_channel(b"", packets[b])[1] - 3


def test_the_compressor_queue_tells_a_reset_from_none():
    packets, hists, _ = _compress_queue()
    carried = list(hists)
    told = 0
    for b, (c, flag, what) in enumerate(QUEUE):
        if not 0 <= c < NCH or b == NOT_A_BLOCK:
            continue
        if flag and packets[b]:
            fresh = O.compress_channel(b"", packets[b])[0]
            other = None if carried[c] is None else O.compress_channel(carried[c], packets[b])[0]
            assert other != fresh and (other is None or len(other) < len(fresh)), (b, what)
            told += 1
        if flag:
            carried[c] = b""
        if carried[c] is not None:
            carried[c] = O.compress_channel(carried[c], packets[b])[3]
    assert told == 4


def test_strided_compressor_equals_the_model():
    allp, hists, before = _compress_queue()
    packets = [allp[b] for b in STRIDED]
    ids, flags = [QUEUE[b][0] for b in STRIDED], [QUEUE[b][1] for b in STRIDED]
    cut = next(b for b, q in enumerate(QUEUE) if q[2] == "mid-run")
    cap = _cut_room(allp, [q[1] for q in QUEUE], cut)                # one capacity for all: it cuts the flagged packets, not the others
    outs, status, final, touched = _apply_rule(_compress_step(packets, [cap] * len(packets)), ids, flags, hists)
    assert status[STRIDED.index(cut)] == 0x0B and (status == 0x07).sum() >= 6, status.tolist()
    n = len(packets)
    x, xl = _rows(packets)
    states = torch.from_numpy(before).cuda()
    out = torch.full((n, (cap + 15) // 16 * 16 + GUARD), FILL, dtype=torch.uint8, device="cuda")
    work, behind = _work(lzs.channels_burst_work_bytes(n, NCH))
    got = lzs.compress_channels_burst(x, xl, _dev(ids, torch.int32), states, cap, out=out, work=work, flags=_dev(flags, torch.uint8))
    torch.cuda.synchronize()
    _check_strided("strided compress", got, outs, status)
    _check_slots("strided compress", states, _want_slots(before, final, touched))
    assert bool((behind == FILL).all()), "bytes behind the work area were written"


def test_packed_compressor_equals_the_model():
    packets, hists, before = _compress_queue()
    ids, flags = [q[0] for q in QUEUE], [q[1] for q in QUEUE]
    cut = next(b for b, q in enumerate(QUEUE) if q[2] == "two in a row")
    rooms = [_cut_room(packets, flags, b) if b == cut else A.compressed_max(len(p)) for b, p in enumerate(packets)]
    off, total = H.lay_out(rooms, {NOT_A_BLOCK})
    rooms = [0 if b == NOT_A_BLOCK else int(off[b + 1] - off[b]) for b in range(len(packets))]
    outs, status, final, touched = _apply_rule(_compress_step(packets, rooms), ids, flags, hists, skip={NOT_A_BLOCK})
    assert status[cut] == 0x0B
    data, in_off, in_len = H.place(torch, packets, True)
    lead = GUARD + 1
    buf = torch.full((lead + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    states = torch.from_numpy(before).cuda()
    work, behind = _work(lzs.channels_burst_work_bytes(len(packets), NCH))
    _, out_len, st = lzs.compress_channels_burst_packed(data, in_off, _dev(ids, torch.int32), states, buf[lead:lead + total],
                                                        torch.from_numpy(off).cuda(), in_len=in_len, work=work, flags=_dev(flags, torch.uint8))
    torch.cuda.synchronize()
    print("packed compress lengths", out_len.tolist(), "status", st.tolist(), "model", status.tolist())
    H.compare("packed compress", buf.cpu().numpy(), out_len.cpu().numpy(), st.cpu().numpy(), H.expected_buffer(off, outs, total, lead), outs,
              status, off, lead)
    _check_slots("packed compress", states, _want_slots(before, final, touched))
    assert bool((behind == FILL).all()), "bytes behind the work area were written"


# ------------------------------------------------------------------ 3. all flagged is a batch
def _batch():
    rng = np.random.default_rng(64)
    lens = rng.integers(200, 1501, 64)
    text = lzs.workload.fill("text", 64, 1504)
    packets = [text[b, :lens[b]].tobytes() for b in range(64)]
    return packets, torch.from_numpy(text).cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("route", ROUTES[1:])
def test_one_channel_with_every_packet_flagged_is_a_batch_of_blocks(monkeypatch, route):
    packets, x, xl = _batch()
    n = len(packets)
    ids, flags = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.full((n,), R, dtype=torch.uint8, device="cuda")
    enc, dec = lzs.new_channel_states(1), lzs.new_channel_states(1)
    enc[0, HIST_AT:HIST_AT + 100] = 9                                   # (a history the first flag discards)
    enc[0, 0] = 100
    dec.copy_(enc)
    want = [O.compress_channel(b"", p) for p in packets]
    comp, cl, cst = lzs.compress_channels_burst(x, xl, ids, enc, flags=flags)
    blocks, bl = lzs.compress_blocks(x, xl)
    torch.cuda.synchronize()
    assert torch.equal(cl, bl) and bool((cst == 0x07).all())
    c, b, k = comp.cpu().numpy(), blocks.cpu().numpy(), cl.cpu().numpy()
    for p in range(n):
        assert c[p, :k[p]].tobytes() == want[p][0] == b[p, :k[p]].tobytes(), p
    _route_env(route, monkeypatch)
    out, ol, st = lzs.decompress_channels_burst(comp, cl, ids, dec, 1500, flags=flags)
    plain, pl = lzs.decompress_blocks(comp, cl, 1500)
    torch.cuda.synchronize()
    assert torch.equal(ol, xl) and torch.equal(pl, xl) and bool((st == M.END).all())
    o, q = out.cpu().numpy(), plain.cpu().numpy()
    for p in range(n):
        assert o[p, :len(packets[p])].tobytes() == packets[p] == q[p, :len(packets[p])].tobytes(), p
    tail = packets[-1][-2047:]
    slot = np.zeros((1, SLOT), dtype=np.uint8)
    _check_slots("all flagged", enc, _want_slots(slot, [tail], {0}))
    _check_slots("all flagged", dec, _want_slots(slot, [tail], {0}))


# ------------------------------------------------------------------ 4. no flags, or none set: the existing entries
def _raw_strided(name, x, xl, ids, flags, states, cap, work):
    """The flags entry through ctypes, so that d_flags can be NULL."""
    n = x.shape[0]
    out = torch.full((n, (cap + 15) // 16 * 16 + GUARD), FILL, dtype=torch.uint8, device="cuda")
    ol, st = torch.full((n,), -1, dtype=torch.int32, device="cuda"), torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    rc = getattr(A.lib(), name)(out.data_ptr(), out.stride(0), cap, ol.data_ptr(), x.data_ptr(), x.stride(0), xl.data_ptr(), x.shape[1],
                                ids.data_ptr(), None if flags is None else flags.data_ptr(), states.data_ptr(), states.shape[0], st.data_ptr(),
                                work.data_ptr(), work.numel(), n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == A.LZS_OK, A.last_error()
    torch.cuda.synchronize()
    return out, ol, st


def _raw_packed(name, data, in_off, in_len, ids, flags, states, buf, out_off, work):
    n = ids.numel()
    ol, st = torch.full((n,), -1, dtype=torch.int32, device="cuda"), torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    rc = getattr(A.lib(), name)(buf.data_ptr(), out_off.data_ptr(), ol.data_ptr(), data.data_ptr(), in_off.data_ptr(), in_len.data_ptr(),
                                ids.data_ptr(), None if flags is None else flags.data_ptr(), states.data_ptr(), states.shape[0], st.data_ptr(),
                                work.data_ptr(), work.numel(), n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == A.LZS_OK, A.last_error()
    torch.cuda.synchronize()
    return buf, ol, st


def test_null_flags_and_zero_flags_are_the_existing_entries(monkeypatch):
    """A queue with repeats, an id out of range and a slot that is no state, through the existing four entries and through the
    new ones with d_flags NULL and with all flags zero: outputs with their fill, lengths, statuses and slots byte for byte."""
    rng = np.random.default_rng(5)
    n, nch = 300, 9
    ids = rng.integers(0, nch + 1, n)
    text = lzs.workload.fill("text", n, 608)
    lens = rng.integers(0, 601, n)
    x, xl = torch.from_numpy(text).cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")
    ch = _dev(ids, torch.int32)
    start = lzs.new_channel_states(nch)
    start[4, :4] = torch.tensor([0xA0, 0x0F, 0, 0], dtype=torch.uint8)
    zeros = torch.zeros(n, dtype=torch.uint8, device="cuda")
    cap = A.compressed_max(608)
    monkeypatch.setenv("LZS_BURST_SPLIT_MIN", "0")
    size = lzs.channels_burst_split_work_bytes(n, nch, 608)
    results = []
    for flags in ("old", None, zeros):
        enc, dec = start.clone(), start.clone()
        work = torch.full((size,), FILL, dtype=torch.uint8, device="cuda")
        if isinstance(flags, str):
            out = torch.full((n, (cap + 15) // 16 * 16 + GUARD), FILL, dtype=torch.uint8, device="cuda")
            c = lzs.compress_channels_burst(x, xl, ch, enc, cap, out=out, work=work)
            back = torch.full((n, 608 + GUARD), FILL, dtype=torch.uint8, device="cuda")
            d = lzs.decompress_channels_burst(c[0], c[1], ch, dec, 608, out=back, work=work)
            torch.cuda.synchronize()
        else:
            c = _raw_strided("lzs_compress_channels_burst_flags_device", x, xl, ch, flags, enc, cap, work)
            d = _raw_strided("lzs_decompress_channels_burst_flags_device", c[0], c[1], ch, flags, dec, 608, work)
        results.append([t.cpu().numpy() for t in (*c, *d, enc, dec)])
    for other in results[1:]:
        for k, (a, b) in enumerate(zip(results[0], other)):
            assert np.array_equal(a, b), k
    # packed: the compressed packets of above, decoded to rooms of their sizes; the originals, compressed to their bounds
    comp, cl = results[0][0], results[0][1]
    streams = [comp[b, :cl[b]].tobytes() for b in range(n)]
    packets = [text[b, :lens[b]].tobytes() for b in range(n)]
    results = []
    for flags in ("old", None, zeros):
        got = []
        for name, src, rooms in (("compress", packets, [A.compressed_max(len(p)) for p in packets]), ("decompress", streams, [int(v) for v in lens])):
            states = start.clone()
            off, total = H.lay_out(rooms)
            data, in_off, in_len = H.place(torch, src, True)
            buf = torch.full((total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            work = torch.full((lzs.channels_burst_packed_split_work_bytes(n, nch, total),), FILL, dtype=torch.uint8, device="cuda")
            doff = torch.from_numpy(off).cuda()
            if isinstance(flags, str):
                r = getattr(lzs, f"{name}_channels_burst_packed")(data, in_off, ch, states, buf[:total], doff, in_len=in_len, work=work)
                torch.cuda.synchronize()
                r = (buf, r[1], r[2])
            else:
                r = _raw_packed(f"lzs_{name}_channels_burst_packed_flags_device", data, in_off, in_len, ch, flags, states, buf, doff, work)
            got += [t.cpu().numpy() for t in (*r, states)]
        results.append(got)
    for other in results[1:]:
        for k, (a, b) in enumerate(zip(results[0], other)):
            assert np.array_equal(a, b), k


# ------------------------------------------------------------------ 5. the round trip in Python
@pytest.mark.parametrize("route", ROUTES[1:])
def test_dense_round_trip_and_channel_codec_with_resets(monkeypatch, route):
    """120 packets on 5 channels, a quarter of them flagged at random: runs that start from the slot and runs that start from
    nothing side by side, decoded by PARSE and RESOLVE (split 0) and by the run decoder (the default threshold)."""
    _route_env(route, monkeypatch)
    rng = np.random.default_rng(11)
    n, nch = 120, 5
    ids = rng.integers(0, nch, n)
    resets = (rng.random(n) < 0.25).astype(np.uint8)
    text = lzs.workload.fill("text", nch, 1 << 15)
    pos = np.zeros(nch, dtype=np.int64)
    packets = []
    for c in ids:
        k = int(rng.integers(0, 700))
        packets.append(text[c, pos[c] % 4096:pos[c] % 4096 + k].tobytes())      # (a channel comes back to its text: matches into history)
        pos[c] += k
    data, in_off, _ = H.place(torch, packets, False)
    ch, flags = _dev(ids, torch.int32), _dev(resets, torch.uint8)
    enc, dec = lzs.new_channel_states(nch), lzs.new_channel_states(nch)
    dense, offsets, status = lzs.compress_channels_dense(data, in_off, ch, enc, flags=flags)
    assert bool((status == 0x07).all())
    back, boff, bst = lzs.decompress_channels_dense(dense, offsets, ch, dec, flags=flags)
    torch.cuda.synchronize()
    assert bool((bst == M.END).all()) and torch.equal(enc, dec)
    b, bo, d, do = back.cpu().numpy(), boff.cpu().numpy(), dense.cpu().numpy(), offsets.cpu().numpy()
    hists = [b""] * nch
    for p in range(n):
        assert b[bo[p]:bo[p + 1]].tobytes() == packets[p], p
        hists[ids[p]] = b"" if resets[p] else hists[ids[p]]
        want, _, _, hists[ids[p]] = O.compress_channel(hists[ids[p]], packets[p])
        assert d[do[p]:do[p + 1]].tobytes() == want, p
    _check_slots("dense", enc, _want_slots(np.zeros((nch, SLOT), dtype=np.uint8), hists, set(int(c) for c in ids)))
    # the codec, launch by launch with hist_len zeroed in between, agrees with the one call
    codec = lzs.ChannelCodec(nch)
    x, xl = _rows(packets + [b"x" * 700])
    x, xl = x[:n], xl[:n]
    out, ol, st = codec.compress(x, xl, ids, resets=resets)
    one = lzs.compress_channels_burst(x, xl, ch, lzs.new_channel_states(nch), flags=flags)
    torch.cuda.synchronize()
    assert torch.equal(ol, one[1]) and torch.equal(st, one[2]) and torch.equal(codec.enc_states, enc)
    k = ol.cpu().numpy()
    assert all(torch.equal(out[p, :k[p]], one[0][p, :k[p]]) for p in range(n))
    got, gl, gs = codec.decompress(out, ol, ids, 700, resets=resets)
    torch.cuda.synchronize()
    assert torch.equal(gl, xl) and torch.equal(codec.dec_states, dec)
    g = got.cpu().numpy()
    assert all(g[p, :len(packets[p])].tobytes() == packets[p] for p in range(n))
