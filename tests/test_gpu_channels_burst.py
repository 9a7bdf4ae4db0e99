"""Many packets per channel in one call (lzs_compress_channels_burst_device / lzs_decompress_channels_burst_device,
include/lzs/lzs_channels.h) on the device.  The oracle is ChannelCodec -- the same packets split into ordered calls of the
one-packet-per-channel entries -- byte for byte: every packet's bytes, length and status, and every final slot, on both
sides; through it the incremental interface and, where oracle/_ref/liblzs_ref.so was built, the reference.  Also round
trips, cut capacity inside a run, slots that are not states, ids out of range, malformed packets, the CHAIN-safe form and
graph capture."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import lzs_compression_amd as lzs
from lzs_compression_amd import api as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "liblzs_ref.so")
C_DONE = A.STATUS_END_MARKER | A.STATUS_INPUT_FINISHED | A.STATUS_INPUT_STARVED
SPECIAL = (0, 1, 2, 3, 12, 2046, 2047, 2048, 4095)
BLOCK = 1 << 17                       # a channel's bytes: its own block of the class, read round and round


def _blocks(cls, n):
    if cls == "zeros":
        return np.zeros((n, BLOCK), dtype=np.uint8)
    return lzs.workload.fill(cls, n, BLOCK)


def _ids(pattern, rng):
    """(ids, nchannels) of a pattern of channel ids."""
    if pattern == "distinct":
        return rng.permutation(2048), 2048
    if pattern == "uniform4":
        return rng.permutation(np.repeat(np.arange(1024), 4)), 1024
    if pattern == "zipf":
        return (rng.zipf(1.1, 16384) - 1) % 4096, 4096
    if pattern == "one300":
        return rng.permutation(np.concatenate([np.zeros(300, dtype=np.int64), np.arange(1, 1025)])), 1025
    if pattern == "tiny":                                  # 1-40 bytes: long walks back for the history
        return rng.integers(0, 64, 4096), 64
    raise ValueError(pattern)


def _packets(blocks, ids, lens, pos):
    out = []
    for c, n in zip(ids, lens):
        b = blocks[c % len(blocks)]
        out.append(b[(pos[c] + np.arange(n)) % b.size].tobytes())
        pos[c] += n
    return out


def _pack(packets, stride=None):
    stride = stride or max(16, (max(len(p) for p in packets) + 15) // 16 * 16)
    x = np.zeros((len(packets), stride), dtype=np.uint8)
    for b, p in enumerate(packets):
        x[b, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    return torch.from_numpy(x).cuda(), torch.tensor([len(p) for p in packets], dtype=torch.int32, device="cuda")


def _rows(slots, lens):
    s, n = slots.cpu().numpy(), lens.cpu().numpy()
    return [s[b, :max(int(n[b]), 0)].tobytes() for b in range(len(n))]


def _same(tag, got, want):
    """Both (out, out_len, status) triples: the bytes each packet got, its length and its status."""
    assert torch.equal(got[1], want[1]), f"{tag}: lengths differ at {torch.nonzero(got[1] != want[1])[:5].tolist()}"
    assert torch.equal(got[2], want[2]), f"{tag}: status differs at {torch.nonzero(got[2] != want[2])[:5].tolist()}"
    a, b = _rows(got[0], got[1]), _rows(want[0], want[1])
    bad = [i for i in range(len(a)) if a[i] != b[i]]
    assert not bad, f"{tag}: {len(bad)} packets differ, first {bad[:5]}"


def _burst_c(x, lens, ids, states, cap=None):
    return lzs.compress_channels_burst(x, lens, torch.tensor(ids, dtype=torch.int32, device="cuda"), states, out_capacity=cap)


def _burst_d(x, lens, ids, states, cap):
    return lzs.decompress_channels_burst(x, lens, torch.tensor(ids, dtype=torch.int32, device="cuda"), states, cap)


def _scenario(cls, pattern, rounds=2, seed=1, big=False, cap=None, digests=None):
    """`rounds` batches of the pattern through the burst calls and through ChannelCodec, on their own states each: equal
    packets, lengths, status, streams and slots on both sides; the decoders give the packets back."""
    rng = np.random.default_rng(seed)
    ids, nch = _ids(pattern, rng)
    blocks = _blocks(cls, min(nch, 256))
    codec = lzs.ChannelCodec(nch)
    enc, dec = lzs.new_channel_states(nch), lzs.new_channel_states(nch)
    pos = np.zeros(nch, dtype=np.int64)
    for r in range(rounds):
        if pattern == "tiny":
            lens = rng.integers(1, 41, ids.size)
        else:
            lens = np.where(rng.random(ids.size) < 0.3, rng.choice(SPECIAL, ids.size), rng.integers(0, 3001, ids.size))
        if big and r == 0:
            lens[:3] = (65536, 70000, 66000)
        packets = _packets(blocks, ids, lens, pos)
        x, xl = _pack(packets)
        want = codec.compress(x, xl, ids, out_capacity=cap)
        got = _burst_c(x, xl, ids, enc, cap)
        torch.cuda.synchronize()
        _same(f"{cls}/{pattern} round {r} compress", got, want)
        assert torch.equal(enc, codec.enc_states), f"{cls}/{pattern} round {r}: compressor slots differ"
        if cap is None:
            assert (got[2].cpu().numpy() == C_DONE).all()
        if digests is not None:
            digests += [hashlib.sha256(s).hexdigest() for s in _rows(got[0], got[1])]
        streams = _rows(got[0], got[1])
        y, yl = _pack(streams)
        room = int(lens.max()) + 64
        want_d = codec.decompress(y, yl, ids, room)
        got_d = _burst_d(y, yl, ids, dec, room)
        torch.cuda.synchronize()
        _same(f"{cls}/{pattern} round {r} decompress", got_d, want_d)
        assert torch.equal(dec, codec.dec_states), f"{cls}/{pattern} round {r}: decompressor slots differ"
        if cap is None:
            assert _rows(got_d[0], got_d[1]) == packets, f"{cls}/{pattern} round {r}: round trip"
            assert torch.equal(enc, dec), f"{cls}/{pattern} round {r}: decoder slots differ from the compressor's"
    return ids, enc


@pytest.mark.parametrize("cls", ["text", "lowent", "random", "zeros"])
@pytest.mark.parametrize("pattern", ["distinct", "uniform4", "zipf", "one300", "tiny"])
def test_burst_equals_channel_codec(cls, pattern):
    _scenario(cls, pattern)


def test_burst_with_long_packets_and_many_rounds():
    _scenario("text", "uniform4", rounds=4, seed=3, big=True)


def test_burst_matches_the_incremental_interface_and_the_reference():
    rng = np.random.default_rng(9)
    nch, npk = 16, 600
    ids = rng.integers(0, nch, npk)
    lens = np.where(rng.random(npk) < 0.3, rng.choice(SPECIAL, npk), rng.integers(0, 2500, npk))
    packets = _packets(_blocks("text", nch), ids, lens, np.zeros(nch, dtype=np.int64))
    x, xl = _pack(packets)
    streams = _rows(*_burst_c(x, xl, ids, lzs.new_channel_states(nch))[:2])
    incs = [A.IncrementalCompressor() for _ in range(nch)]
    for b, c in enumerate(ids):
        got, used, st = incs[c].step(packets[b], A.compressed_max(len(packets[b])) + 16, add_end_marker=True)
        assert used == len(packets[b]) and st & A.STATUS_END_MARKER
        assert streams[b] == got, f"packet {b} (channel {c}): differs from the incremental interface"
    if os.path.exists(REF_SO):
        R = ctypes.CDLL(REF_SO)
        R.lzs_compress_init_full.restype, R.lzs_compress_init_full.argtypes = None, [ctypes.c_void_p]
        R.lzs_compress_incremental.restype, R.lzs_compress_incremental.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_bool]
        params = {}
        for b, c in enumerate(ids[:200]):
            if c not in params:
                params[c] = A.CompressParameters()
                R.lzs_compress_init_full(ctypes.addressof(params[c]))
            p, out, pending = params[c], bytearray(), packets[b]
            while True:
                src = ctypes.create_string_buffer(pending, max(len(pending), 1))
                room = A.compressed_max(len(packets[b])) + 16
                dst = ctypes.create_string_buffer(room)
                p.inPtr, p.inLength, p.outPtr, p.outLength = ctypes.addressof(src), len(pending), ctypes.addressof(dst), room
                n = R.lzs_compress_incremental(ctypes.addressof(p), True)
                out += dst.raw[:n]
                pending = pending[len(pending) - p.inLength:]
                if p.status & A.STATUS_END_MARKER:
                    break
            assert streams[b] == bytes(out), f"packet {b} (channel {c}): differs from the reference"


def test_burst_streams_decode_with_the_one_packet_calls():
    rng = np.random.default_rng(4)
    ids, nch = _ids("zipf", rng)
    lens = rng.integers(0, 2000, ids.size)
    packets = _packets(_blocks("text", 256), ids, lens, np.zeros(nch, dtype=np.int64))
    x, xl = _pack(packets)
    enc = lzs.new_channel_states(nch)
    out, ol, _ = _burst_c(x, xl, ids, enc)
    y, yl = _pack(_rows(out, ol))
    codec = lzs.ChannelCodec(nch)
    back, bl, st = codec.decompress(y, yl, ids, 2064)
    torch.cuda.synchronize()
    assert _rows(back, bl) == packets and (st.cpu().numpy() & A.STATUS_END_MARKER).all()
    assert torch.equal(codec.dec_states, enc)


def test_cut_capacity_in_the_middle_of_runs():
    """out_cap below some packets' output: compressor and decoder as ChannelCodec, packet for packet, the later packets of
    each run included."""
    _scenario("text", "one300", rounds=2, seed=5, cap=700)
    rng = np.random.default_rng(6)
    ids, nch = _ids("uniform4", rng)
    lens = np.full(ids.size, 1500)
    packets = _packets(_blocks("text", 256), ids, lens, np.zeros(nch, dtype=np.int64))
    x, xl = _pack(packets)
    streams = _rows(*_burst_c(x, xl, ids, lzs.new_channel_states(nch))[:2])
    y, yl = _pack(streams)
    for room in (1500, 1499, 1460):
        codec = lzs.ChannelCodec(nch)
        want = codec.decompress(y, yl, ids, room)
        dec = lzs.new_channel_states(nch)
        got = _burst_d(y, yl, ids, dec, room)
        torch.cuda.synchronize()
        _same(f"decoder room {room}", got, want)
        assert torch.equal(dec, codec.dec_states)


def test_slots_that_are_not_states_and_ids_out_of_range():
    rng = np.random.default_rng(8)
    nch, npk, bad = 32, 400, (3, 17)
    ids = rng.integers(0, nch + 4, npk)                    # ids nch .. nch + 3 are out of range
    lens = rng.integers(0, 1800, npk)
    packets = _packets(_blocks("text", nch + 4), ids, lens, np.zeros(nch + 4, dtype=np.int64))
    x, xl = _pack(packets)
    good = ids < nch
    gi = torch.from_numpy(np.nonzero(good)[0]).cuda()
    for call in ("compress", "decompress"):
        states = lzs.new_channel_states(nch)
        xs, xls = x, xl
        if call == "decompress":
            enc = lzs.new_channel_states(nch)
            out, ol, _ = _burst_c(x[gi], xl[gi], ids[good], enc)
            streams = _rows(out, ol)
            full = [b""] * npk
            for k, b in enumerate(np.nonzero(good)[0]):
                full[b] = streams[k]
            xs, xls = _pack(full)
        for c in bad:
            states[c] = 0x77
            states[c, :4] = torch.tensor([0xA0, 0x0F, 0, 0], dtype=torch.uint8)        # hist_len 4000
        before = states.clone()
        ref = states.clone()
        codec = lzs.ChannelCodec(nch)
        if call == "compress":
            codec.enc_states = ref
            want = codec.compress(xs[gi], xls[gi], ids[good], out_capacity=4096)
            got = lzs.compress_channels_burst(xs, xls, torch.tensor(ids, dtype=torch.int32, device="cuda"), states,
                                              out_capacity=4096)
        else:
            codec.dec_states = ref
            want = codec.decompress(xs[gi], xls[gi], ids[good], 4096)
            got = lzs.decompress_channels_burst(xs, xls, torch.tensor(ids, dtype=torch.int32, device="cuda"), states, 4096)
        torch.cuda.synchronize()
        st, n = got[2].cpu().numpy(), got[1].cpu().numpy()
        assert (st[~good] == A.STATUS_ERROR).all() and (n[~good] == 0).all(), call
        for c in bad:
            assert (st[ids == c] == A.STATUS_ERROR).all() and (n[ids == c] == 0).all(), (call, c)
            assert torch.equal(states[c], before[c]), (call, c)
        _same(call, (got[0][gi], got[1][gi], got[2][gi]), want)
        assert torch.equal(states, ref), f"{call}: slots differ from ChannelCodec's"


def test_malformed_packets_stay_in_their_slots():
    rng = np.random.default_rng(11)
    ids, nch = _ids("zipf", rng)
    ids, cap, guard = ids[:4096], 4096, 64
    lens = rng.integers(0, 2500, ids.size)
    packets = _packets(_blocks("text", 256), ids, lens, np.zeros(nch, dtype=np.int64))
    x, xl = _pack(packets)
    good = _rows(*_burst_c(x, xl, ids, lzs.new_channel_states(nch))[:2])
    bad = []
    for b in range(ids.size):
        if b % 3 == 0:
            bad.append(rng.integers(0, 256, int(rng.integers(1, 3000)), dtype=np.uint8).tobytes())
        elif b % 3 == 1:
            bad.append(good[b] + rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8).tobytes())
        else:
            bad.append(good[b][:int(rng.integers(0, len(good[b]) + 1))])
    y, yl = _pack(bad)
    codec = lzs.ChannelCodec(nch)
    want = codec.decompress(y, yl, ids, cap)
    dec = lzs.new_channel_states(nch)
    out = torch.full((ids.size, cap + guard), 0xA5, dtype=torch.uint8, device="cuda")
    got = lzs.decompress_channels_burst(y, yl, torch.tensor(ids, dtype=torch.int32, device="cuda"), dec, cap, out=out)
    torch.cuda.synchronize()
    _same("malformed", got, want)
    assert torch.equal(dec, codec.dec_states)
    n, o = got[1].cpu().numpy(), out.cpu().numpy()
    assert (n <= cap).all() and (o[:, cap:] == 0xA5).all(), "a packet wrote past its capacity"
    assert all((o[b, n[b]:cap] == 0xA5).all() for b in range(ids.size)), "a packet wrote past its length"


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_channels_burst as T
d = []
T._scenario("text", "zipf", digests=d)
open(sys.argv[2], "w").write("\n".join(d))
'''


def test_chain_safe_form_gives_the_same_streams(tmp_path):
    """LZS_CHAIN_FALLBACK=1: the burst compressor runs the order-independent CHAIN form of the channel kernel -- the same
    checks against ChannelCodec and the same streams, in a child process."""
    out = tmp_path / "digests.txt"
    env = dict(os.environ, PYTHONPATH=ROOT, LZS_CHAIN_FALLBACK="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    mine = []
    _scenario("text", "zipf", digests=mine)
    assert out.read_text().split("\n") == mine


def test_graph_capture_equals_direct_calls():
    rng = np.random.default_rng(12)
    ids, nch = _ids("uniform4", rng)
    lens = rng.integers(0, 1600, ids.size)
    pos = np.zeros(nch, dtype=np.int64)
    blocks = _blocks("text", 256)
    rounds = [_packets(blocks, ids, lens, pos) for _ in range(2)]
    stride = 1616
    xs = [_pack(p, stride) for p in rounds]
    ch = torch.tensor(ids, dtype=torch.int32, device="cuda")
    cap = A.compressed_max(stride)
    # direct calls
    enc_d = lzs.new_channel_states(nch)
    direct = []
    for x, xl in xs:
        o, ol, st = lzs.compress_channels_burst(x, xl, ch, enc_d, out_capacity=cap)
        direct.append((o.clone(), ol.clone(), st.clone()))
    # the same through one captured call, replayed per round with the round's packets copied in
    x_in, xl_in = xs[0][0].clone(), xs[0][1].clone()
    enc_g = lzs.new_channel_states(nch)
    out = torch.empty((ids.size, (cap + 15) // 16 * 16), dtype=torch.uint8, device="cuda")
    out_len = torch.empty(ids.size, dtype=torch.int32, device="cuda")
    status = torch.empty(ids.size, dtype=torch.uint8, device="cuda")
    work = torch.empty(lzs.channels_burst_work_bytes(ids.size, nch), dtype=torch.uint8, device="cuda")
    scratch = lzs.new_channel_states(nch)                  # a call outside the graph first: the library's start-up
    lzs.compress_channels_burst(x_in, xl_in, ch, scratch, out_capacity=cap, out=out, out_len=out_len, status=status, work=work)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lzs.compress_channels_burst(x_in, xl_in, ch, enc_g, out_capacity=cap, out=out, out_len=out_len, status=status, work=work)
    for r, (x, xl) in enumerate(xs):
        x_in.copy_(x)
        xl_in.copy_(xl)
        g.replay()
        torch.cuda.synchronize()
        _same(f"graph round {r}", (out, out_len, status), direct[r])
    assert torch.equal(enc_g, enc_d)
