"""Every channel compression route of the device against the plain CPU model of include/lzs/lzs_channels.h compression
(oracle/lzs_oracle.c: lzs_oracle_compress_channel): lzs_compress_channels_device, lzs_compress_channels_burst_device and
ChannelCodec.compress.  The other channel tests compress workload data at aligned places; here histories and packets are built on
purpose (tests/test_channel_encode_model.py, which also proves on the CPU that they reach every edge the model counts: matches,
comparisons and refills on the border between history and packet, offset 2047 to view byte 0, nibbles of 15 across the border, the
burst's gathered histories) and every packet's bytes, length and exact status byte, the 0xA5 fill from its length to the end of its
row, and every slot whole are compared with the model, none left out."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lzs_compression_amd as lzs

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_channel_encode_model as M  # noqa: E402
from test_channel_encode_model import O  # noqa: E402
from test_gpu_channel_model import FILL, GUARD, _place, _slot_rows  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_MODELLED = {}


def _modelled(sc, cap):
    if (sc.name, cap) not in _MODELLED:
        _MODELLED[sc.name, cap] = sc.modelled(cap)
    return _MODELLED[sc.name, cap]


def _out_rows(n, cap, base=None):
    """The output rows, filled with 0xA5: the library's own shape (16-byte multiples, aligned), or -- `base` 0..3 -- a view with
    an odd row stride whose first byte lies `base` bytes behind an aligned address.  Returns (rows, the tensor they lie in)."""
    cols = (max(cap, 1) + 15) // 16 * 16 + GUARD
    if base is None:
        out = torch.full((n, cols), FILL, dtype=torch.uint8, device="cuda")
        return out, out
    stride = cols | 1
    flat = torch.full((64 + base + n * stride + 128,), FILL, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 64 == 0
    return flat[64 + base:64 + base + n * stride].view(n, stride), flat


def _compress(route, x, xl, ids, states, cap, out):
    """One call on `route`; a burst call gets a work area of exactly channels_burst_work_bytes(), filled with 0xA5."""
    n, nch = len(ids), states.shape[0]
    ch = torch.tensor(np.asarray(ids, dtype=np.int64).astype(np.int32), dtype=torch.int32, device="cuda")
    if route == "channels":
        assert int(np.max(ids)) < nch and int(np.min(ids)) >= 0            # (the one-packet call does not check its ids)
        got = lzs.compress_channels(x, xl, ch, states, cap, out=out)
    else:
        work = torch.full((lzs.channels_burst_work_bytes(n, nch),), FILL, dtype=torch.uint8, device="cuda")
        got = lzs.compress_channels_burst(x, xl, ch, states, cap, out=out, work=work)
    torch.cuda.synchronize()
    return got


def _explain(tag, b, c, packet, hist, cap, got, got_len, got_st):
    """The failing packet for the assertion message: where it differs and the model's token there."""
    want, total, st, _, tokens = O.compress_channel(hist, packet, cap, trace=True)
    k = min(len(want), int(got_len), len(got))
    diff = next((i for i in range(k) if want[i] != got[i]), k)
    at = [t.tolist() for t in tokens if t[3] <= 8 * diff + 7][-1:] or None
    return (f"{tag}: packet {b}, channel {c}, hlen {len(hist)}, {len(packet)} bytes, capacity {cap}: length {int(got_len)} (model "
            f"{len(want)} of {total}), status {int(got_st):#x} (model {st:#x}), first differing byte {diff}: "
            f"{bytes(got[diff:diff + 8]).hex()} (model {want[diff:diff + 8].hex()}); model token there [pos in packet, offset, length, "
            f"bit] {at}; packet {packet[:32].hex()}{'...' if len(packet) > 32 else ''}, history ends {hist[-8:].hex()}")


def _compare(tag, packets, ids, cap, m, got, states=None, before=None, lengths_only_to=None):
    """Everything a call wrote against the model `m`: every packet, the fill past every length, every slot."""
    o, n, st = got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()
    want = np.full(o.shape, FILL, dtype=np.uint8)
    for b, w in enumerate(m.outs):
        want[b, :len(w)] = np.frombuffer(w, dtype=np.uint8)
    if lengths_only_to is not None:                                            # (a route that hands back rows it did not fill)
        for b, w in enumerate(m.outs):
            o[b, len(w):] = FILL
    want_n = np.array([len(w) for w in m.outs])
    bad = np.nonzero((n != want_n) | (st != m.status) | (o != want).any(axis=1))[0]
    if bad.size:
        b = int(bad[0])
        if m.before[b] is None:
            raise AssertionError(f"{tag}: packet {b} on channel {ids[b]}, which is no state or no channel: length {n[b]}, status "
                                 f"{st[b]:#x}, row written: {bool((o[b] != FILL).any())}")
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
                                 f"(model {len(m.hists[c]) if m.hists[c] is not None else None}), bytes {s[c, i:i + 8].tobytes().hex()} (model "
                                 f"{want_s[c, i:i + 8].tobytes().hex()}); its last packet {last}, {[len(packets[b]) for b in last]} bytes, "
                                 f"hlen before it {[len(m.before[b]) for b in last]}, capacity {cap}")


def _run(sc, route, caps=None, base=1, fill="random", out_base=None, uniform=False):
    """The scenario's rounds at each capacity, the slots carried from round to round (a history does not depend on the
    capacity: every capacity goes through the same slots)."""
    placed = [_place(packets, base, fill) for packets, _ in sc.rounds]
    for cap in caps or sc.caps:
        before = _slot_rows(sc.slots)
        states = torch.from_numpy(before).cuda()
        for r, ((packets, ids), m) in enumerate(zip(sc.rounds, _modelled(sc, cap))):
            x, xl = placed[r]
            if uniform:                                                        # no length array: the rows are the packets
                x, xl = x[:, :len(packets[0])], None
            out, whole = _out_rows(len(packets), cap, out_base)
            got = _compress(route, x, xl, ids, states, cap, out)
            tag = f"{sc.name}, {route}, round {r}, capacity {cap}, input base {base}, {fill} behind, output base {out_base}"
            _compare(tag, packets, ids, cap, m, got, states, before)
            if out_base is not None:                                           # nothing around the rows either
                w = whole.cpu().numpy()
                lead, end = 64 + out_base, 64 + out_base + out.shape[0] * out.stride(0)
                assert (w[:lead] == FILL).all() and (w[end:] == FILL).all(), f"{tag}: bytes outside the output rows were written"


# ------------------------------------------------------------------ the routes
@pytest.mark.parametrize("n", M.SINGLE_BATCHES)
def test_one_packet_call(n):
    """1, 64, 257 and 1500 packets, three rounds on carried slots, roomy and cut: histories of every length of HIST_LENS, packets
    that continue, repeat and straddle them."""
    _run(M.single_scenario(n), "channels")


@pytest.mark.parametrize("n", (65, 1500))
def test_bursts_of_distinct_channels(n):
    _run(M.single_scenario(n), "burst")


def test_bursts_with_runs_of_1_2_13_and_600():
    """Ids interleaved; zero-length packets first, in the middle and last in a run; earlier packets of exactly 2046, 2047 and 2048
    bytes behind a slot history of 2047 bytes (kept only in part) and of none; a slot that is no state, ids that name no channel;
    two rounds."""
    _run(M.burst_scenario(), "burst")


def test_burst_of_2100_one_byte_packets():
    _run(M.one_byte_scenario(), "burst")


def test_without_a_length_array():
    """in_len = None: every row is a packet of the rows' one length, on both calls."""
    _run(M.uniform_scenario(), "channels", uniform=True)
    _run(M.uniform_scenario(), "burst", uniform=True)


def test_channel_codec_splits_repeated_ids():
    """ChannelCodec.compress on bursts (runs of 1, 2, 13 and 40): launch k takes every channel's k-th packet."""
    sc = M.burst_scenario(long_run=40, out_of_range=False)
    for cap in sc.caps:
        codec = lzs.ChannelCodec(sc.nch)
        before = _slot_rows(sc.slots)
        codec.enc_states.copy_(torch.from_numpy(before).cuda())
        for r, ((packets, ids), m) in enumerate(zip(sc.rounds, _modelled(sc, cap))):
            x, xl = _place(packets)
            got = codec.compress(x, xl, ids, out_capacity=cap)
            torch.cuda.synchronize()
            _compare(f"{sc.name}, ChannelCodec, round {r}, capacity {cap}", packets, ids, cap, m, got, codec.enc_states, before,
                     lengths_only_to=cap)                                      # (its rows are not pre-filled: bytes up to the lengths)


@pytest.mark.parametrize("route", ("channels", "burst"))
def test_capacities_chosen_from_the_model(route):
    """out_cap of 0, 1, total - 1, total and total + 1 of chosen packets and one inside a match head, read from the model; all
    packets compressed at each: 0x07 exactly where total <= cap, the history advanced all the same, nothing written from cap on."""
    sc = M.single_scenario(64)
    packets, ids = sc.rounds[0]
    chosen = M.chosen_capacities(packets, _modelled(sc, None)[0].before)
    assert len({place for _, _, place in chosen}) == 6
    x, xl = _place(packets)
    for cap in sorted({cap for _, cap, _ in chosen}):
        m = M.run_model(packets, ids, sc.slots, cap)
        assert ((m.status == M.DONE) == (m.totals <= cap))[m.status != M.ERROR].all()
        before = _slot_rows(sc.slots)
        states = torch.from_numpy(before).cuda()
        got = _compress(route, x, xl, ids, states, cap, _out_rows(len(packets), cap)[0])
        _compare(f"chosen capacity {cap}, {route}", packets, ids, cap, m, got, states, before)


@pytest.mark.parametrize("route", ("channels", "burst"))
def test_placement(route):
    """Input rows with a stride that is no multiple of 4 and their base 0, 1, 2 and 3 bytes behind an aligned address, random bytes
    behind each packet; output rows through out= with an odd stride and their base 0, 1, 2 and 3 behind an aligned address; roomy
    and cut."""
    sc = M.single_scenario(257)
    for base in (0, 1, 2, 3):
        _run(sc, route, base=base, fill="random", out_base=(base + 1) % 4)
    _run(sc, route, base=0, fill="random", out_base=0)


_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_gpu_channel_encode_model as T
T._run(T.M.single_scenario(257), "channels")
T._run(T.M.burst_scenario(), "burst")
print("chain-safe form: the model's streams")
"""


def test_chain_safe_form_gives_the_models_streams():
    """LZS_CHAIN_FALLBACK=1 (decided once per process) compresses through wgv_safe_ch, the order-independent CHAIN form: the
    257-packet scenario and the bursts against the model, in one fresh child process."""
    env = dict(os.environ, PYTHONPATH=ROOT, LZS_CHAIN_FALLBACK="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "the model's streams" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
