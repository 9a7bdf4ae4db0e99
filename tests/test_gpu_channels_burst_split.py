"""lzs_decompress_channels_burst_device with the larger work area (lzs_channels_burst_split_work_bytes): the
packets of long runs are parsed all at once with per-byte origins and resolved per run afterwards.  The results must be those
of the other route byte for byte.  The oracle is ChannelCodec, and beside it the same entry with a work area of the burst
size, on clones of the same states: every packet's bytes, length and status, every final slot, and a 0xA5 fill past each
length untouched.  LZS_BURST_SPLIT_MIN puts runs on either side: 0 splits every run, a value between the weights of one
call's runs splits some, the default splits the long ones.  Which route ran is read from the work area itself."""
import numpy as np
import pytest

import lzs_compression_amd as lzs
from lzs_compression_amd import api as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_channels_burst import _blocks, _ids, _pack, _packets, _rows, _same  # noqa: E402

GUARD = 64
FILL = 0xA5


def _ch(ids):
    return torch.tensor(np.asarray(ids), dtype=torch.int32, device="cuda")


def _compress(packets, ids, nch, states=None):
    x, xl = _pack(packets)
    enc = lzs.new_channel_states(nch) if states is None else states
    out, ol, _ = lzs.compress_channels_burst(x, xl, _ch(ids), enc)
    return _rows(out, ol)


def _decode(y, yl, ids, states, cap, size):
    """One burst decode into a 0xA5-filled output with a 0xA5-filled work area of `size` bytes."""
    work = torch.full((size,), FILL, dtype=torch.uint8, device="cuda")
    out = torch.full((len(ids), (max(cap, 1) + 15) // 16 * 16 + GUARD), FILL, dtype=torch.uint8, device="cuda")
    got = lzs.decompress_channels_burst(y, yl, _ch(ids), states, cap, out=out, work=work)
    torch.cuda.synchronize()
    return got, work


def _fill_untouched(tag, got):
    o, n = got[0].cpu().numpy(), got[1].cpu().numpy()
    col = np.arange(o.shape[1])[None, :]
    assert ((o == FILL) | (col < n[:, None])).all(), f"{tag}: bytes past a packet's length were written"


def _check(tag, streams, ids, nch, cap, states, codec_ok=None):
    """Decode `streams` on clones of `states` by ChannelCodec, by the burst entry with the burst-sized work area and with the
    split-sized one: all the same.  `codec_ok`: the packets ChannelCodec can take (ids in range).  Returns the final slots."""
    ids = np.asarray(ids)
    y, yl = _pack(streams)
    n = len(ids)
    small, large = lzs.channels_burst_work_bytes(n, nch), lzs.channels_burst_split_work_bytes(n, nch, cap)
    assert large > small
    s_old, s_new = states.clone(), states.clone()
    old, _ = _decode(y, yl, ids, s_old, cap, small)
    new, _ = _decode(y, yl, ids, s_new, cap, large)
    _same(f"{tag}: split against the other route", new, old)
    assert torch.equal(s_new, s_old), f"{tag}: slots differ between the routes"
    _fill_untouched(tag, new)
    _fill_untouched(tag + " (other route)", old)
    codec = lzs.ChannelCodec(nch)
    codec.dec_states = states.clone()
    if codec_ok is None:
        want = codec.decompress(y, yl, ids, cap)
        _same(f"{tag}: split against ChannelCodec", new, want)
    else:
        gi = torch.from_numpy(np.nonzero(codec_ok)[0]).cuda()
        want = codec.decompress(y[gi], yl[gi], ids[codec_ok], cap)
        _same(f"{tag}: split against ChannelCodec", (new[0][gi], new[1][gi], new[2][gi]), want)
    torch.cuda.synchronize()
    assert torch.equal(s_new, codec.dec_states), f"{tag}: slots differ from ChannelCodec's"
    return s_new, new


SPECIAL = (0, 1, 2, 3, 12, 2046, 2047, 2048, 4095)


def _two_rounds(cls, pattern, seed=1):
    rng = np.random.default_rng(seed)
    ids, nch = _ids(pattern, rng)
    blocks = _blocks(cls, min(nch, 256))
    enc, dec = lzs.new_channel_states(nch), lzs.new_channel_states(nch)
    pos = np.zeros(nch, dtype=np.int64)
    for r in range(2):
        if pattern == "tiny":
            lens = rng.integers(1, 41, ids.size)
        else:
            lens = np.where(rng.random(ids.size) < 0.3, rng.choice(SPECIAL, ids.size), rng.integers(0, 3001, ids.size))
        packets = _packets(blocks, ids, lens, pos)
        streams = _compress(packets, ids, nch, enc)
        dec, got = _check(f"{cls}/{pattern} round {r}", streams, ids, nch, int(lens.max()) + 64, dec)
        assert _rows(got[0], got[1]) == packets, f"{cls}/{pattern} round {r}: round trip"
        assert torch.equal(enc, dec)


# the compressed bytes of a run are its weight: 0 splits every run, 6000 some runs of every pattern but `tiny` and `distinct`
# (whose runs are lighter; `tiny` has 64 runs of about 1.4 KB: 1400 divides them), the default the long ones only
@pytest.mark.parametrize("split_min", ["0", "mixed", None])
@pytest.mark.parametrize("cls", ["text", "lowent", "random", "zeros"])
@pytest.mark.parametrize("pattern", ["distinct", "uniform4", "zipf", "one300", "tiny"])
def test_split_equals_channel_codec_and_the_other_route(monkeypatch, cls, pattern, split_min):
    if split_min == "mixed":
        split_min = {"tiny": "1400", "distinct": "1500"}.get(pattern, "6000")
    if split_min is None:
        monkeypatch.delenv("LZS_BURST_SPLIT_MIN", raising=False)
    else:
        monkeypatch.setenv("LZS_BURST_SPLIT_MIN", split_min)
    _two_rounds(cls, pattern)


def test_a_threshold_puts_runs_of_one_call_on_both_sides(monkeypatch):
    """13 runs of 3 text packets of 1500 bytes among 200 single ones: with a threshold between the two weights the heavy runs
    are 13 (not a multiple of eight), and the work area beyond the burst size is written; every run decodes as before."""
    rng = np.random.default_rng(21)
    nch = 213
    ids = rng.permutation(np.concatenate([np.repeat(np.arange(13), 3), np.arange(13, nch)]))
    packets = _packets(_blocks("text", 213), ids, np.full(ids.size, 1500), np.zeros(nch, dtype=np.int64))
    streams = _compress(packets, ids, nch)
    sizes = np.array([len(s) for s in streams])
    heavy = min(sizes[ids == c].sum() for c in range(13))
    light = sizes[ids >= 13].max()
    assert light < heavy
    monkeypatch.setenv("LZS_BURST_SPLIT_MIN", str(int(light) + 1))
    dec, got = _check("both sides", streams, ids, nch, 1500, lzs.new_channel_states(nch))
    assert _rows(got[0], got[1]) == packets


def test_lengths_0_1_2046_2047_2048_and_long_packets_in_one_run(monkeypatch):
    monkeypatch.setenv("LZS_BURST_SPLIT_MIN", "0")
    lens = [1500, 0, 1, 2046, 0, 2047, 2048, 70000, 3, 66000, 0, 2049, 5, 4096, 1]
    for cls in ("text", "zeros", "lowent"):
        ids = np.concatenate([np.zeros(len(lens), dtype=np.int64), np.ones(len(lens), dtype=np.int64)])
        ll = np.array(lens + lens[::-1])
        packets = _packets(_blocks(cls, 2), ids, ll, np.zeros(2, dtype=np.int64))
        streams = _compress(packets, ids, 2)
        for cap in (70000, 70001):
            dec, got = _check(f"lengths/{cls}/{cap}", streams, ids, 2, cap, lzs.new_channel_states(2))
            assert _rows(got[0], got[1]) == packets


def test_a_copy_reaches_back_over_thousands_of_one_byte_packets(monkeypatch):
    """3000 packets of one byte on one channel, then packets that copy the 2047 bytes before them: every byte of those comes
    from a packet of its own.  On a second channel the same with a byte pattern of period 7 (copies all the way)."""
    monkeypatch.setenv("LZS_BURST_SPLIT_MIN", "0")
    rng = np.random.default_rng(22)
    base = rng.integers(0, 256, 3000, dtype=np.uint8)
    packets, ids = [], []
    for k in range(3000):
        packets += [bytes(base[k:k + 1]), bytes([k % 7])]
        ids += [0, 1]
    for _ in range(3):                                     # what the last 2047 one-byte packets gave, once more (a copy)
        packets += [bytes(base[-2047:]), bytes([k % 7 for k in range(3000, 5047)])]
        ids += [0, 1]
    ids = np.array(ids)
    streams = _compress(packets, ids, 2)
    assert len(streams[-2]) < 400, "the long packet should be one copy"
    dec, got = _check("one-byte packets", streams, ids, 2, 2047, lzs.new_channel_states(2))
    assert _rows(got[0], got[1]) == packets


def test_young_channels_copy_zeros_and_preset_slots(monkeypatch):
    """Packets compressed on a channel with history, decoded on slots with less: what lies before the start reads as zero.
    Slots preset with hist_len 1 and 2047 (and 0, 5, 100)."""
    monkeypatch.setenv("LZS_BURST_SPLIT_MIN", "0")
    rng = np.random.default_rng(23)
    nch = 5
    ids = rng.integers(0, nch, 60)
    blocks = _blocks("text", nch)
    pos = np.zeros(nch, dtype=np.int64)
    enc = lzs.new_channel_states(nch)
    _compress(_packets(blocks, np.arange(nch), np.full(nch, 2047), pos), np.arange(nch), nch, enc)     # 2047 bytes of history
    packets = _packets(blocks, ids, rng.integers(0, 900, ids.size), pos * 0)      # ... which the packets repeat
    streams = _compress(packets, ids, nch, enc)
    dec = lzs.new_channel_states(nch)
    for c, h in enumerate((0, 1, 2047, 5, 100)):
        dec[c, 64:64 + h] = torch.from_numpy(rng.integers(0, 256, h, dtype=np.uint8)).cuda()
        dec[c, :4] = torch.tensor([h & 0xFF, h >> 8, 0, 0], dtype=torch.uint8)
    _check("young channels", streams, ids, nch, 1024, dec)


def test_cut_capacity_inside_runs(monkeypatch):
    rng = np.random.default_rng(6)
    for split_min in ("0", "6000"):
        monkeypatch.setenv("LZS_BURST_SPLIT_MIN", split_min)
        ids, nch = _ids("uniform4", rng)
        packets = _packets(_blocks("text", 256), ids, np.full(ids.size, 1500), np.zeros(nch, dtype=np.int64))
        streams = _compress(packets, ids, nch)
        for room in (1500, 1499, 1460):
            _check(f"room {room}", streams, ids, nch, room, lzs.new_channel_states(nch))
        ids, nch = _ids("one300", rng)
        lens = rng.integers(0, 3001, ids.size)
        packets = _packets(_blocks("text", 256), ids, lens, np.zeros(nch, dtype=np.int64))
        streams = _compress(packets, ids, nch)
        for room in (700, 1):
            _check(f"one300 room {room}", streams, ids, nch, room, lzs.new_channel_states(nch))


def test_slots_that_are_not_states_and_ids_out_of_range(monkeypatch):
    monkeypatch.setenv("LZS_BURST_SPLIT_MIN", "0")
    rng = np.random.default_rng(8)
    nch, npk, bad = 32, 400, (3, 17)
    ids = rng.integers(0, nch + 4, npk)                    # ids nch .. nch + 3 are out of range
    lens = rng.integers(0, 1800, npk)
    packets = _packets(_blocks("text", nch + 4), ids, lens, np.zeros(nch + 4, dtype=np.int64))
    good = ids < nch
    some = _compress([packets[b] for b in np.nonzero(good)[0]], ids[good], nch)
    streams = [b"\x01\x02\x03"] * npk
    for k, b in enumerate(np.nonzero(good)[0]):
        streams[b] = some[k]
    states = lzs.new_channel_states(nch)
    for c in bad:
        states[c] = 0x77
        states[c, :4] = torch.tensor([0xA0, 0x0F, 0, 0], dtype=torch.uint8)        # hist_len 4000
    before = states.clone()
    after, got = _check("not states", streams, ids, nch, 4096, states, codec_ok=good)
    st, n = got[2].cpu().numpy(), got[1].cpu().numpy()
    assert (st[~good] == A.STATUS_ERROR).all() and (n[~good] == 0).all()
    for c in bad:
        assert (st[ids == c] == A.STATUS_ERROR).all() and (n[ids == c] == 0).all(), c
        assert torch.equal(after[c], before[c]), c


def test_malformed_packets_stay_in_their_slots(monkeypatch):
    rng = np.random.default_rng(11)
    ids, nch = _ids("zipf", rng)
    ids, cap = ids[:4096], 4096
    lens = rng.integers(0, 2500, ids.size)
    good = _compress(_packets(_blocks("text", 256), ids, lens, np.zeros(nch, dtype=np.int64)), ids, nch)
    bad = []
    for b in range(ids.size):
        if b % 3 == 0:
            bad.append(rng.integers(0, 256, int(rng.integers(1, 3000)), dtype=np.uint8).tobytes())
        elif b % 3 == 1:
            bad.append(good[b] + rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8).tobytes())
        else:
            bad.append(good[b][:int(rng.integers(0, len(good[b]) + 1))])
    for split_min in ("0", "6000"):
        monkeypatch.setenv("LZS_BURST_SPLIT_MIN", split_min)
        for room in (cap, 900):
            _check(f"malformed, room {room}", bad, ids, nch, room, lzs.new_channel_states(nch))


def test_graph_capture_equals_direct_calls(monkeypatch):
    monkeypatch.setenv("LZS_BURST_SPLIT_MIN", "3000")
    rng = np.random.default_rng(12)
    ids, nch = _ids("one300", rng)
    lens = rng.integers(0, 1600, ids.size)
    pos = np.zeros(nch, dtype=np.int64)
    blocks = _blocks("text", 256)
    enc = lzs.new_channel_states(nch)
    cap, stride = 1600, A.compressed_max(1600) + 15 & ~15
    ys = [_pack(_compress(_packets(blocks, ids, lens, pos), ids, nch, enc), stride) for _ in range(2)]
    ch = _ch(ids)
    dec_d = lzs.new_channel_states(nch)
    direct = []
    for y, yl in ys:
        o, ol, st = lzs.decompress_channels_burst(y, yl, ch, dec_d, cap)
        direct.append((o.clone(), ol.clone(), st.clone()))
    y_in, yl_in = ys[0][0].clone(), ys[0][1].clone()
    dec_g = lzs.new_channel_states(nch)
    out = torch.empty((ids.size, 1600), dtype=torch.uint8, device="cuda")
    out_len = torch.empty(ids.size, dtype=torch.int32, device="cuda")
    status = torch.empty(ids.size, dtype=torch.uint8, device="cuda")
    work = torch.empty(lzs.channels_burst_split_work_bytes(ids.size, nch, cap), dtype=torch.uint8, device="cuda")
    scratch = lzs.new_channel_states(nch)                  # a call outside the graph first: the library's start-up
    lzs.decompress_channels_burst(y_in, yl_in, ch, scratch, cap, out=out, out_len=out_len, status=status, work=work)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lzs.decompress_channels_burst(y_in, yl_in, ch, dec_g, cap, out=out, out_len=out_len, status=status, work=work)
    for r, (y, yl) in enumerate(ys):
        y_in.copy_(y)
        yl_in.copy_(yl)
        g.replay()
        torch.cuda.synchronize()
        _same(f"graph round {r}", (out, out_len, status), direct[r])
    assert torch.equal(dec_g, dec_d)


def test_which_route_ran_is_seen_in_the_work_area(monkeypatch):
    """Equal bytes cannot tell the routes apart; the work area can: filled with 0xA5, the part beyond the burst size is written
    by the split route (the origins) and by nothing else."""
    rng = np.random.default_rng(13)
    ids, nch = _ids("one300", rng)
    packets = _packets(_blocks("text", 256), ids, np.full(ids.size, 1500), np.zeros(nch, dtype=np.int64))
    streams = _compress(packets, ids, nch)
    y, yl = _pack(streams)
    n, cap = ids.size, 1500
    small, large = lzs.channels_burst_work_bytes(n, nch), lzs.channels_burst_split_work_bytes(n, nch, cap)

    def beyond_written(size):
        got, work = _decode(y, yl, ids, lzs.new_channel_states(nch), cap, size)
        assert _rows(got[0], got[1]) == packets
        return bool((work[small:] != FILL).any().item())

    monkeypatch.setenv("LZS_BURST_SPLIT_MIN", "0")
    assert beyond_written(large), "every run split: the origins were not written"
    assert not beyond_written(large - 1), "a work area one byte short of the split size must take the other route"
    assert not beyond_written(small)
    monkeypatch.setenv("LZS_BURST_SPLIT_MIN", str(int(sum(len(s) for s in streams)) + 1))
    assert not beyond_written(large), "a threshold above every run: nothing beyond the burst size may be written"
    monkeypatch.delenv("LZS_BURST_SPLIT_MIN")
    assert beyond_written(large), "the default threshold splits a run of 300 packets"
