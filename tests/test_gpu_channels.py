"""Many channels, one packet each (include/lzs/lzs_channels.h) on the device: packet for packet the bytes of the
incremental interface on that channel's own parameter block (itself pinned to the reference: test_gpu_incremental.py,
tests/golden/inc_packets.lzs), the reference itself where oracle/_ref/liblzs_ref.so was built, round trips with the
decoder's state equal to the compressor's, resets, cut capacity, the order-independent CHAIN form, malformed packets,
the ratio against stateless blocks and repeated channel ids through ChannelCodec.

Not covered here: the packets are workload data at aligned places (_pack: a 16-byte-aligned base, strides of 16, the library's
own output), so matches, comparisons and refills on the border between history and packet, the extreme matches, unaligned rows
and the exact status byte at total == out_cap come up by chance or not at all.  tests/test_gpu_channel_encode_model.py builds
those cases on purpose and compares with the plain model of channel compression (oracle/lzs_oracle.c:
lzs_oracle_compress_channel)."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "liblzs_ref.so")
C_DONE = A.STATUS_END_MARKER | A.STATUS_INPUT_FINISHED | A.STATUS_INPUT_STARVED
SPECIAL = (0, 1, 2, 3, 12, 2046, 2047, 2048, 4095)
BLOCK = 16384                         # a channel's bytes: its own block of the class, read round and round


def _blocks(cls, n):
    if cls == "zeros":
        return np.zeros((n, BLOCK), dtype=np.uint8)
    return lzs.workload.fill(cls, n, BLOCK)


def _take(block, start, n):
    return block[(start + np.arange(n)) % block.size].tobytes()


def _lengths(rng, nch, rounds, big=True):
    """[rounds, nch]: the special lengths and random ones up to 9000; a few packets of 64 KiB and more."""
    L = np.where(rng.random((rounds, nch)) < 0.3, rng.choice(SPECIAL, (rounds, nch)), rng.integers(0, 9001, (rounds, nch)))
    if big:
        L[2, :3] = (65536, 70000, 66000)
    return L


def _pack(packets):
    stride = max(16, (max(len(p) for p in packets) + 15) // 16 * 16)
    x = np.zeros((len(packets), stride), dtype=np.uint8)
    for b, p in enumerate(packets):
        x[b, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    lens = torch.tensor([len(p) for p in packets], dtype=torch.int32, device="cuda")
    return torch.from_numpy(x).cuda(), lens


def _unpack(slots, lens):
    s, n = slots.cpu().numpy(), lens.cpu().numpy()
    return [s[b, :n[b]].tobytes() for b in range(len(n))]


def _compress(packets, states, channels=None, out_capacity=None):
    x, lens = _pack(packets)
    ch = None if channels is None else torch.tensor(channels, dtype=torch.int32, device="cuda")
    cap = A.compressed_max(x.shape[1]) if out_capacity is None else out_capacity
    slots, out_len, status = lzs.compress_channels(x, lens, ch, states, out_capacity=cap)
    torch.cuda.synchronize()
    return _unpack(slots, out_len), status.cpu().numpy()


def _decompress(streams, states, out_capacity, channels=None):
    x, lens = _pack(streams)
    ch = None if channels is None else torch.tensor(channels, dtype=torch.int32, device="cuda")
    out, out_len, status = lzs.decompress_channels(x, lens, ch, states, out_capacity)
    torch.cuda.synchronize()
    return _unpack(out, out_len), status.cpu().numpy()


def _inc_step(enc, data):
    got, used, status = enc.step(data, A.compressed_max(len(data)) + 16, add_end_marker=True)
    assert used == len(data) and status & A.STATUS_END_MARKER
    return got


class _RefCompressor:
    """The reference's own parameter block (oracle/_ref/liblzs_ref.so) through ctypes, as make_incremental_golden.py drives it."""
    REF = None

    def __init__(self):
        if _RefCompressor.REF is None:
            R = ctypes.CDLL(REF_SO)
            R.lzs_compress_init_full.restype, R.lzs_compress_init_full.argtypes = None, [ctypes.c_void_p]
            R.lzs_compress_incremental.restype = ctypes.c_size_t
            R.lzs_compress_incremental.argtypes = [ctypes.c_void_p, ctypes.c_bool]
            _RefCompressor.REF = R
        self.p = A.CompressParameters()
        _RefCompressor.REF.lzs_compress_init_full(ctypes.addressof(self.p))

    def step(self, data):
        out, pending = bytearray(), data
        while True:
            src = ctypes.create_string_buffer(pending, max(len(pending), 1))
            room = A.compressed_max(len(data)) + 16
            dst = ctypes.create_string_buffer(room)
            self.p.inPtr, self.p.inLength, self.p.outPtr, self.p.outLength = ctypes.addressof(src), len(pending), ctypes.addressof(dst), room
            n = _RefCompressor.REF.lzs_compress_incremental(ctypes.addressof(self.p), True)
            out += dst.raw[:n]
            pending = pending[len(pending) - self.p.inLength:]
            if self.p.status & A.STATUS_END_MARKER:
                return bytes(out)


def test_golden_packets_on_one_channel():
    packets = [open(os.path.join(GOLDEN, f"inc_packet_{i}.bin"), "rb").read() for i in range(3)]
    want = open(os.path.join(GOLDEN, "inc_packets.lzs"), "rb").read()
    enc, dec = lzs.new_channel_states(1), lzs.new_channel_states(1)
    streams = []
    for p in packets:
        got, st = _compress([p], enc)
        assert st[0] == C_DONE
        streams += got
    assert b"".join(streams) == want, "the channel's packets differ from the reference's lzs_compress_incremental"
    for p, s in zip(packets, streams):
        full = lzs.new_channel_states(1)
        full.copy_(dec)
        out, st = _decompress([s], dec, len(p) + 64)
        assert out[0] == p and st[0] & A.STATUS_END_MARKER
        out, st = _decompress([s], full, len(p))           # the output exactly full: the end marker still counts
        assert out[0] == p and st[0] == A.STATUS_END_MARKER and torch.equal(full, dec)
    assert torch.equal(enc, dec)


def _scenario(cls, nch=4096, rounds=6, seed=1, ref_sample=256, reset_every=0):
    """Rounds of one packet per channel through both calls, checked packet for packet against an IncrementalCompressor per
    channel (and the reference's block on a sample); the decoder's output and state after every round."""
    rng = np.random.default_rng(seed)
    blocks = _blocks(cls, nch)
    L = _lengths(rng, nch, rounds)
    enc_s, dec_s = lzs.new_channel_states(nch), lzs.new_channel_states(nch)
    incs = [A.IncrementalCompressor() for _ in range(nch)]
    refs = {c: _RefCompressor() for c in range(0, nch, max(1, nch // ref_sample))} if ref_sample and os.path.exists(REF_SO) else {}
    pos = np.zeros(nch, dtype=np.int64)
    digests = []
    for r in range(rounds):
        if reset_every and r == rounds // 2:
            for c in range(0, nch, reset_every):           # hist_len = 0: a fresh channel from here on
                enc_s[c, :4] = 0
                dec_s[c, :4] = 0
                incs[c] = A.IncrementalCompressor()
                refs.pop(c, None)
        packets = [_take(blocks[c], int(pos[c]), int(L[r, c])) for c in range(nch)]
        pos += L[r]
        streams, st = _compress(packets, enc_s)
        assert (st == C_DONE).all(), f"round {r}: status {np.unique(st)}"
        for c in range(nch):
            want = _inc_step(incs[c], packets[c])
            assert streams[c] == want, f"{cls} round {r} channel {c} ({len(packets[c])} bytes): differs from the incremental interface"
            if c in refs:
                assert streams[c] == refs[c].step(packets[c]), f"{cls} round {r} channel {c}: differs from the reference"
        digests += [hashlib.sha256(s).hexdigest() for s in streams]
        out, dst = _decompress(streams, dec_s, int(L[r].max()) + 64)
        assert all(dst & A.STATUS_END_MARKER), f"round {r}: decoder status {np.unique(dst)}"
        bad = [c for c in range(nch) if out[c] != packets[c]]
        assert not bad, f"{cls} round {r}: {len(bad)} packets do not come back, first channel {bad[0]}"
        assert torch.equal(enc_s, dec_s), f"{cls} round {r}: decoder state differs from the compressor's"
        hl = enc_s[:, :4].cpu().numpy().view(np.uint32).reshape(-1)
        assert (hl <= 2047).all()
    return digests


@pytest.mark.parametrize("cls", ["text", "lowent", "random", "zeros"])
def test_channels_match_the_incremental_interface_and_round_trip(cls):
    _scenario(cls)


def test_reset_and_young_channels():
    """hist_len = 0 mid-sequence makes a fresh channel; short packets keep many channels under 2047 bytes of history."""
    _scenario("text", nch=1024, rounds=6, seed=7, ref_sample=64, reset_every=5)
    rng = np.random.default_rng(3)
    blocks = _blocks("text", 256)
    enc_s, dec_s = lzs.new_channel_states(256), lzs.new_channel_states(256)
    incs = [A.IncrementalCompressor() for _ in range(256)]
    pos = np.zeros(256, dtype=np.int64)
    for r in range(12):                                    # 0..300 bytes a packet: histories grow through 2047 slowly
        lens = rng.integers(0, 301, 256)
        packets = [_take(blocks[c], int(pos[c]), int(lens[c])) for c in range(256)]
        pos += lens
        streams, st = _compress(packets, enc_s)
        assert (st == C_DONE).all()
        assert all(streams[c] == _inc_step(incs[c], packets[c]) for c in range(256)), f"round {r}"
        out, _ = _decompress(streams, dec_s, 400)
        assert out == packets and torch.equal(enc_s, dec_s)
    hl = enc_s[:, :4].cpu().numpy().view(np.uint32).reshape(-1)
    assert (hl < 2047).any() and (hl == 2047).any()


def test_cut_capacity_is_a_prefix_and_advances_the_history():
    blocks = _blocks("text", 256)
    first = [_take(blocks[c], 0, 1500) for c in range(256)]
    second = [_take(blocks[c], 1500, 1500) for c in range(256)]
    full, cut = lzs.new_channel_states(256), lzs.new_channel_states(256)
    _compress(first, full)
    _compress(first, cut)
    want, st_full = _compress(second, full)
    got, st_cut = _compress(second, cut, out_capacity=200)
    assert (st_full == C_DONE).all()
    assert all(len(want[c]) > 200 for c in range(256))
    for c in range(256):
        assert got[c] == want[c][:200], f"channel {c}: not a prefix of the uncut output"
    assert all((s & A.STATUS_NO_OUTPUT_BUFFER_SPACE) and not (s & A.STATUS_END_MARKER) for s in st_cut)
    assert torch.equal(full, cut), "the cut run's history differs from the uncut run's"


_CHILD = r'''
import hashlib, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_channels as T
open(sys.argv[2], "w").write("\n".join(T._scenario("text", ref_sample=0)))
'''


def test_chain_safe_form_gives_the_same_streams(tmp_path):
    """LZS_CHAIN_FALLBACK=1 (a device that fails the LDS ordering check) compresses through wgv_safe_ch: the same streams,
    and the same checks against the incremental interface, in a child process."""
    out = tmp_path / "digests.txt"
    env = dict(os.environ, PYTHONPATH=ROOT, LZS_CHAIN_FALLBACK="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert out.read_text().split("\n") == _scenario("text", ref_sample=0)


def test_malformed_packets_stay_in_their_slots():
    nch, cap, guard = 2048, 4096, 64
    rng = np.random.default_rng(11)
    blocks = _blocks("text", nch)
    hist = [_take(blocks[c], 0, int(rng.integers(0, 3000))) for c in range(nch)]
    # channels 2c of a state array of 2 nch slots: the odd slots are guards
    enc_s = lzs.new_channel_states(2 * nch)
    dec_s = torch.full((2 * nch, A.CHANNEL_STATE_BYTES), 0x5A, dtype=torch.uint8, device="cuda")
    dec_s[0::2] = 0
    ids = list(range(0, 2 * nch, 2))
    streams, _ = _compress(hist, enc_s, channels=ids)
    _decompress(streams, dec_s, 4096, channels=ids)
    good, _ = _compress([_take(blocks[c], 5000, 3000) for c in range(nch)], lzs.new_channel_states(nch))
    bad = []
    for c in range(nch):
        if c % 2:
            bad.append(rng.integers(0, 256, int(rng.integers(1, 3000)), dtype=np.uint8).tobytes())
        elif c % 4 == 2:                                   # a whole packet, then bytes the decoder must ignore
            bad.append(good[c] + rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8).tobytes())
        else:
            g = good[c]
            bad.append(g[:int(rng.integers(0, len(g)))])
    before = dec_s.clone()
    x, lens = _pack(bad)
    out = torch.full((nch, cap + guard), 0xA5, dtype=torch.uint8, device="cuda")
    out_len = torch.empty(nch, dtype=torch.int32, device="cuda")
    status = torch.empty(nch, dtype=torch.uint8, device="cuda")
    lzs.decompress_channels(x, lens, torch.tensor(ids, dtype=torch.int32, device="cuda"), dec_s, cap, out=out, out_len=out_len,
                            status=status)
    torch.cuda.synchronize()
    n = out_len.cpu().numpy()
    assert (n <= cap).all()
    assert bool((out[:, cap:] == 0xA5).all()), "a packet wrote past its capacity"
    o = out.cpu().numpy()
    assert all((o[b, n[b]:cap] == 0xA5).all() for b in range(nch)), "a packet wrote past its length"
    assert torch.equal(dec_s[1::2], before[1::2]), "a guard slot between the channels changed"
    # where the library's incremental decoder on the same channel stops at an end marker (within the room), the output is its
    # output; where it runs out of bits first it may hold the packet's last token back for bits to come, which the channel
    # decoder, given whole packets, decodes: its output then begins with the incremental decoder's
    compared = 0
    for c in range(0, nch, 2):                             # (the truncated packets and the whole ones with bytes behind)
        d = A.IncrementalDecompressor()
        d.step(streams[c], 4096)
        try:
            got, used, st = d.step(bad[c], cap)
        except lzs.LzsError:
            continue
        mine = o[c, :n[c]].tobytes()
        if st & A.STATUS_END_MARKER and len(got) < cap:
            assert mine == got, f"channel {c}: differs from the incremental decoder"
            compared += 1
        elif used == len(bad[c]) and len(got) < cap:
            assert mine.startswith(got), f"channel {c}: does not begin with the incremental decoder's output"
    assert compared > 20


def test_history_beats_stateless_blocks_on_text():
    nch, rounds = 4096, 8
    blocks = _blocks("text", nch)
    states, dec_states = lzs.new_channel_states(nch), lzs.new_channel_states(nch)
    total_ch = total_blk = 0
    for r in range(rounds):
        packets = [_take(blocks[c], 1500 * r, 1500) for c in range(nch)]
        got, st = _compress(packets, states)
        assert (st == C_DONE).all()
        back, dst = _decompress(got, dec_states, 1500)      # every output exactly full: the end markers still count
        assert back == packets and (dst == A.STATUS_END_MARKER).all() and torch.equal(states, dec_states)
        total_ch += sum(len(g) for g in got)
        x, _ = _pack(packets)
        _, lens = lzs.compress_blocks(x[:, :1500].contiguous())
        total_blk += int(lens.sum().item())
    raw = nch * rounds * 1500
    print(f"ratio with history {total_ch / raw:.4f}, stateless {total_blk / raw:.4f}")
    assert total_ch < total_blk


def test_channel_codec_splits_repeated_ids():
    nch, npk = 64, 640
    rng = np.random.default_rng(5)
    ids = rng.integers(0, nch, npk)
    blocks = _blocks("text", nch)
    pos = np.zeros(nch, dtype=np.int64)
    packets = []
    for c in ids:
        n = int(rng.integers(0, 2500))
        packets.append(_take(blocks[c], int(pos[c]), n))
        pos[c] += n
    codec = lzs.ChannelCodec(nch)
    x, lens = _pack(packets)
    slots, out_len, status = codec.compress(x, lens, ids)
    torch.cuda.synchronize()
    streams = _unpack(slots, out_len)
    assert (status.cpu().numpy() == C_DONE).all()
    incs = [A.IncrementalCompressor() for _ in range(nch)]
    for b, c in enumerate(ids):
        assert streams[b] == _inc_step(incs[c], packets[b]), f"packet {b} (channel {c})"
    y, ylens = _pack(streams)
    out, n, st = codec.decompress(y, ylens, ids, 2600)
    torch.cuda.synchronize()
    assert _unpack(out, n) == packets and all(st.cpu().numpy() & A.STATUS_END_MARKER)
    assert torch.equal(codec.enc_states, codec.dec_states)


def test_decoder_cut_capacity_reports_no_room():
    """out_cap below a packet's output: the output is a prefix and the status NO_OUTPUT_BUFFER_SPACE without END_MARKER --
    also when the cut falls inside a copy that the end marker follows (its token was consumed whole, its bytes were not)."""
    enc, dec = lzs.new_channel_states(1), lzs.new_channel_states(1)
    (s,), _ = _compress([b"abcabcabc"], enc)               # three literals, a copy of 6 at offset 3, the end marker
    (out,), (st,) = _decompress([s], dec, 5)
    assert out == b"abcab" and st == A.STATUS_NO_OUTPUT_BUFFER_SPACE, (out, st)
    nch = 1024
    blocks = _blocks("text", nch)
    enc = lzs.new_channel_states(nch)
    dec = lzs.new_channel_states(nch)
    first = [_take(blocks[c], 0, 1500) for c in range(nch)]
    second = [_take(blocks[c], 1500, 1500) for c in range(nch)]
    streams, _ = _compress(first, enc)
    _decompress(streams, dec, 1500)
    streams, _ = _compress(second, enc)
    for cut in (0, 1, 3, 40):
        d = lzs.new_channel_states(nch)
        d.copy_(dec)
        out, st = _decompress(streams, d, 1500 - cut)
        assert all(out[c] == second[c][:1500 - cut] for c in range(nch)), f"cap {1500 - cut}: not a prefix"
        want = A.STATUS_END_MARKER if cut == 0 else A.STATUS_NO_OUTPUT_BUFFER_SPACE
        assert (st == want).all(), f"cap {1500 - cut}: status {np.unique(st)}"
        if cut == 0:
            assert torch.equal(d, enc)


def test_slots_that_are_not_states_get_error_and_nothing_changes():
    nch, bad = 8, (3, 5)
    blocks = _blocks("text", nch)
    packets = [_take(blocks[c], 0, 1000) for c in range(nch)]
    x, lens = _pack(packets)
    for call in ("compress", "decompress"):
        states = lzs.new_channel_states(nch)
        if call == "decompress":
            streams, _ = _compress(packets, lzs.new_channel_states(nch))
            x, lens = _pack(streams)
        for c in bad:
            states[c] = 0x77
            states[c, :4] = torch.tensor([0xA0, 0x0F, 0, 0], dtype=torch.uint8)        # hist_len 4000
        before = states.clone()
        out = torch.full((nch, 2048), 0xA5, dtype=torch.uint8, device="cuda")
        out_len = torch.full((nch,), 12345, dtype=torch.int32, device="cuda")
        status = torch.zeros(nch, dtype=torch.uint8, device="cuda")
        if call == "compress":
            lzs.compress_channels(x, lens, None, states, out_capacity=2048, out=out, out_len=out_len, status=status)
        else:
            lzs.decompress_channels(x, lens, None, states, 2048, out=out, out_len=out_len, status=status)
        torch.cuda.synchronize()
        st, n = status.cpu().numpy(), out_len.cpu().numpy()
        for c in range(nch):
            if c in bad:
                assert st[c] == A.STATUS_ERROR and n[c] == 0, (call, c, st[c], n[c])
                assert bool((out[c] == 0xA5).all()) and torch.equal(states[c], before[c]), (call, c)
            else:
                assert st[c] & A.STATUS_END_MARKER and n[c] > 0, (call, c, st[c])
