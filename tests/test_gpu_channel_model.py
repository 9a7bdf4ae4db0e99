"""Every channel decode route of the device against the plain CPU model of include/lzs/lzs_channels.h
(oracle/lzs_oracle.c: lzs_oracle_decompress_channel): lzs_decompress_channels_device, the burst call's run decoder, its split
route (parse + resolve) and the decoded-size query.  The other channel tests compare one instantiation of the decoder template
with another, or decode what our own compressor wrote; here the packets are synthesised token by token
(tests/test_channel_model.py, which also proves on the CPU that they reach every edge) and every packet's bytes, length and
status, every final slot, and the 0xA5 fill past every length are compared with the model, none left out."""
import numpy as np
import pytest

import lzs_compression_amd as lzs
from lzs_compression_amd import api as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_channel_model as M  # noqa: E402
from test_channel_model import O  # noqa: E402

GUARD = 64
FILL = 0xA5
SLOT, HIST_AT = A.CHANNEL_STATE_BYTES, 64
ROUTES = ("channels", "burst run", "burst split 0", "burst split default")
_MODELLED = {}


def _modelled(sc, cap):
    if (sc.name, cap) not in _MODELLED:
        _MODELLED[sc.name, cap] = sc.modelled(cap)
    return _MODELLED[sc.name, cap]


def _place(packets, base=1, fill="random"):
    """The packets as rows of a device tensor whose stride is no multiple of 4 and whose first byte lies `base` bytes behind an
    aligned address; what lies behind each packet in its row is zero or random."""
    n = len(packets)
    stride = (max(len(p) for p in packets) + 4) // 4 * 4 + 1
    size = n * stride
    flat = np.zeros(size + 128, dtype=np.uint8) if fill == "zero" else np.random.default_rng(size).integers(0, 256, size + 128, dtype=np.uint8)
    rows = flat[64 + base:64 + base + size].reshape(n, stride)
    for b, p in enumerate(packets):
        rows[b, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    dev = torch.from_numpy(flat).cuda()
    assert dev.data_ptr() % 64 == 0
    x = dev[64 + base:64 + base + size].view(n, stride)
    return x, torch.tensor([len(p) for p in packets], dtype=torch.int32, device="cuda")


def _slot_rows(hists, before=None):
    """The slots of these histories: hist_len, 60 zero bytes, the history, zeros to 2048.  None: no state (hist_len 4000 over
    0x77), or what `before` held."""
    s = np.zeros((len(hists), SLOT), dtype=np.uint8)
    for c, h in enumerate(hists):
        if h is None:
            s[c] = 0x77 if before is None else before[c]
            s[c, :4] = (0xA0, 0x0F, 0, 0)
        else:
            s[c, :4] = np.frombuffer(len(h).to_bytes(4, "little"), dtype=np.uint8)
            s[c, HIST_AT:HIST_AT + len(h)] = np.frombuffer(h, dtype=np.uint8)
    return s


def _decode(route, monkeypatch, x, xl, ids, states, cap):
    """One call on `route`.  The library splits where the work area has room for the origins, 2 * n * cap bytes more than
    channels_burst_work_bytes: at capacity 0 that is no more, so there "burst run" is "burst split default" (runs of 8192
    compressed bytes or more go through parse + resolve) under another name -- a failure at capacity 0 tagged "burst run" may
    be the split route's."""
    n, nch = len(ids), states.shape[0]
    ch = torch.tensor(np.asarray(ids), dtype=torch.int32, device="cuda")
    out = torch.full((n, (max(cap, 1) + 15) // 16 * 16 + GUARD), FILL, dtype=torch.uint8, device="cuda")
    if route == "channels":
        got = lzs.decompress_channels(x, xl, ch, states, cap, out=out)
    else:
        if route == "burst split 0":
            monkeypatch.setenv("LZS_BURST_SPLIT_MIN", "0")
        else:
            monkeypatch.delenv("LZS_BURST_SPLIT_MIN", raising=False)
        size = lzs.channels_burst_work_bytes(n, nch) if route == "burst run" else lzs.channels_burst_split_work_bytes(n, nch, cap)
        work = torch.full((size,), FILL, dtype=torch.uint8, device="cuda")
        got = lzs.decompress_channels_burst(x, xl, ch, states, cap, out=out, work=work)
    torch.cuda.synchronize()
    return got


def _explain(tag, b, c, packet, hist, cap, got, got_len, got_st):
    """The failing packet for the assertion message: where it differs and the model's token there."""
    want, st, _, tokens, stop = O.decompress_channel(hist, packet, cap, trace=True)
    k = min(len(want), int(got_len), len(got))
    diff = next((i for i in range(k) if want[i] != got[i]), k)
    at = [t.tolist() for t in tokens if t[0] <= diff][-1:] or None
    return (f"{tag}: packet {b}, channel {c}, hist_len {len(hist)}, capacity {cap}: length {int(got_len)} (model {len(want)}), "
            f"status {int(got_st):#x} (model {st:#x}), first differing byte {diff}: {bytes(got[diff:diff + 8]).hex()} (model "
            f"{want[diff:diff + 8].hex()}); model token there [out pos, offset, length, bit] {at}, stopped at bit {stop}; "
            f"packet {packet[:48].hex()}{'...' if len(packet) > 48 else ''} ({len(packet)} bytes)")


def _compare(tag, packets, ids, cap, m, got, states=None, before=None):
    """Everything a call wrote against the model `m`: every packet, the fill past every length, every slot."""
    o, n, st = got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()
    want = np.full(o.shape, FILL, dtype=np.uint8)
    for b, w in enumerate(m.outs):
        want[b, :len(w)] = np.frombuffer(w, dtype=np.uint8)
    want_n = np.array([len(w) for w in m.outs])
    bad = np.nonzero((n != want_n) | (st != m.status) | (o != want).any(axis=1))[0]
    if bad.size:
        b = int(bad[0])
        if m.before[b] is None:
            raise AssertionError(f"{tag}: packet {b} on channel {ids[b]}, whose slot is no state: length {n[b]}, status {st[b]:#x}")
        past = np.nonzero(o[b, want_n[b]:] != FILL)[0]
        note = f"; byte {want_n[b] + past[0]} past the length was written" if n[b] == want_n[b] and past.size else ""
        raise AssertionError(_explain(f"{tag} ({bad.size} packets differ)", b, int(ids[b]), packets[b], m.before[b], cap, o[b], n[b], st[b]) + note)
    if states is not None:
        s, want_s = states.cpu().numpy(), _slot_rows(m.hists, before)
        rows = np.nonzero((s != want_s).any(axis=1))[0]
        if rows.size:
            c = int(rows[0])
            i = int(np.nonzero(s[c] != want_s[c])[0][0])
            last = [b for b in range(len(ids)) if ids[b] == c][-1:]
            raise AssertionError(f"{tag}: {rows.size} slots differ, first channel {c} at slot byte {i}: hist_len {int(s[c, :4].view('<u4')[0])} "
                                 f"(model {len(m.hists[c])}), bytes {s[c, i:i + 8].tobytes().hex()} (model {want_s[c, i:i + 8].tobytes().hex()}); "
                                 f"its last packet {last}, status {m.status[last].tolist()}, capacity {cap}")


def _run(sc, route, monkeypatch, caps=None, base=1, fill="random"):
    """The scenario's rounds at each capacity on slots of their own, carried from round to round."""
    placed = [_place(packets, base, fill) for packets, _ in sc.rounds]
    for cap in caps or sc.caps:
        before = _slot_rows(sc.slots)
        states = torch.from_numpy(before).cuda()
        for r, ((packets, ids), m) in enumerate(zip(sc.rounds, _modelled(sc, cap))):
            got = _decode(route, monkeypatch, *placed[r], ids, states, cap)
            _compare(f"{sc.name}, {route}, round {r}, capacity {cap}, base {base}, {fill} behind", packets, ids, cap, m, got, states, before)


# ------------------------------------------------------------------ the routes
@pytest.mark.parametrize("n", M.SINGLE_BATCHES)
def test_one_packet_call(monkeypatch, n):
    """Batches of 1, 63, 64, 65, 257 and 1500 packets (the grouping of streams per wavefront), compressed lengths 0, 2, 40 and
    3000 side by side, three rounds on the same slots at every capacity: the later rounds copy from what the earlier rounds'
    malformed and cut packets left."""
    _run(M.single_scenario(n), "channels", monkeypatch)


@pytest.mark.parametrize("route", ROUTES[1:])
@pytest.mark.parametrize("n", (65, 1500))
def test_bursts_of_distinct_channels(monkeypatch, route, n):
    _run(M.single_scenario(n), route, monkeypatch)


@pytest.mark.parametrize("route", ROUTES[1:])
def test_bursts_with_runs_of_1_2_13_and_600(monkeypatch, route):
    """Ids interleaved, zero-output packets in the runs, outputs on both sides of 2048 in one run, 600 packets across the resolve
    kernel's meta window, a slot that is no state; two rounds."""
    _run(M.burst_scenario(), route, monkeypatch)


@pytest.mark.parametrize("route", ROUTES[1:])
def test_a_copy_of_70000_bytes_in_mid_run(monkeypatch, route):
    _run(M.big_copy_scenario(), route, monkeypatch)


@pytest.mark.parametrize("route", ROUTES[1:])
def test_copies_over_2100_one_byte_packets(monkeypatch, route):
    _run(M.one_byte_scenario(), route, monkeypatch)


def test_decoded_sizes():
    """The size query on the same packets: length and status are the model's at every capacity, for every packet (it sees no slot: the
    packets of the channel that is no state get what the model gives them on an empty history, not ERROR)."""
    for sc in M.gpu_scenarios():
        for r, (packets, ids) in enumerate(sc.rounds):
            x, xl = _place(packets)
            for cap in sc.caps:
                size, status = lzs.decompressed_sizes(x, xl, limit=cap)
                torch.cuda.synchronize()
                m = _modelled(sc, cap)[r]
                want, want_st = np.array([len(w) for w in m.outs]), m.status.copy()
                for b in (b for b, h in enumerate(m.before) if h is None):     # no state: the query sees none, and a length
                    out, want_st[b], _ = O.decompress_channel(b"", packets[b], cap)   # does not depend on the history
                    want[b] = len(out)
                got_n, got_st = size.cpu().numpy(), status.cpu().numpy()
                bad = np.nonzero((got_n != want) | (got_st != want_st))[0][:5]
                assert not bad.size, (f"size query, {sc.name}, round {r}, capacity {cap}: packets {bad.tolist()}: sizes {got_n[bad].tolist()} "
                                      f"(model {want[bad].tolist()}), status {got_st[bad].tolist()} (model {want_st[bad].tolist()}); first "
                                      f"packet {packets[bad[0]][:48].hex()} ({len(packets[bad[0]])} bytes)")


@pytest.mark.parametrize("route", ROUTES)
def test_capacities_chosen_from_the_model(monkeypatch, route):
    """A capacity inside a first copy, inside a nibble run, exactly at a packet's size (the marker still counts) and exactly at
    the size of a packet that ends on a closing nibble 0 -- read from the model's trace; the whole handful decoded at each."""
    packets = list(M.chosen_packets())
    rng = np.random.default_rng(41)
    slots = M.start_slots(rng, len(packets))
    ids = np.arange(len(packets))
    x, xl = _place(packets)
    chosen = M.chosen_capacities(packets)
    assert len({place for _, _, place in chosen}) == 4
    for cap in sorted({cap for _, cap, _ in chosen}):
        before = _slot_rows(slots)
        states = torch.from_numpy(before).cuda()
        got = _decode(route, monkeypatch, x, xl, ids, states, cap)
        _compare(f"chosen capacity {cap}, {route}", packets, ids, cap, M.run_model(packets, ids, slots, cap), got, states, before)
        size, status = lzs.decompressed_sizes(x, xl, limit=cap)
        assert torch.equal(size, got[1]) and torch.equal(status, got[2]), cap


@pytest.mark.parametrize("route", ROUTES)
def test_input_placement(monkeypatch, route):
    """A stride that is no multiple of 4, the base 0, 1, 2 and 3 bytes behind an aligned address, zeros or random bytes behind
    each packet in its row: the model's results every time."""
    sc = M.single_scenario(257)
    for base in (0, 1, 2, 3):
        for fill in ("zero", "random"):
            _run(sc, route, monkeypatch, caps=(sc.caps[0], 100), base=base, fill=fill)


def test_the_model_decodes_what_the_burst_compressor_writes():
    """The link to the reference-pinned side: compress_channels_burst is held to the incremental interface and the reference
    (test_gpu_channels_burst.py); the model decodes its packets to the originals and ends with the compressor's slots."""
    rng = np.random.default_rng(42)
    for cls in ("text", "lowent"):
        nch = 40
        ids = rng.integers(0, nch, 400)
        blocks = lzs.workload.fill(cls, nch, 1 << 16)
        pos = np.zeros(nch, dtype=np.int64)
        lens = np.where(rng.random(ids.size) < 0.3, rng.choice((0, 1, 2, 2046, 2047, 2048), ids.size), rng.integers(0, 3001, ids.size))
        packets = []
        for c, k in zip(ids, lens):
            packets.append(blocks[c, pos[c]:pos[c] + k].tobytes())
            pos[c] += k
        stride = (int(lens.max()) + 15) // 16 * 16
        x = np.zeros((ids.size, stride), dtype=np.uint8)
        for b, p in enumerate(packets):
            x[b, :len(p)] = np.frombuffer(p, dtype=np.uint8)
        enc = lzs.new_channel_states(nch)
        out, ol, st = lzs.compress_channels_burst(torch.from_numpy(x).cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda"),
                                                  torch.tensor(ids, dtype=torch.int32, device="cuda"), enc)
        torch.cuda.synchronize()
        o, n = out.cpu().numpy(), ol.cpu().numpy()
        streams = [o[b, :n[b]].tobytes() for b in range(ids.size)]
        m = M.run_model(streams, ids, [b""] * nch, int(lens.max()))
        assert m.outs == packets, [b for b in range(ids.size) if m.outs[b] != packets[b]][:5]
        assert (m.status == M.END).all()
        assert np.array_equal(enc.cpu().numpy(), _slot_rows(m.hists)), cls
