"""lzs_decompressed_size_batch_device on the GPU (include/lzs/lzs_batch.h): the length and the status it reports
are those the decoders report.  The oracle is never the code under test: lzs.decompress_channels on fresh all-zero states
(length and status) and lzs.decompress_blocks (length), both at out_capacity = limit, and for whole streams the raw length.

A limit of 0xFFFFFFFF cannot be an out_capacity.  The oracles then decode at a capacity C above every true size of the batch
(a length nibble, 4 bits for 15 bytes, is the densest token: no stream of n bytes decodes to more than 30 n) and every block is
asserted to end below C without NO_OUTPUT_BUFFER_SPACE: the capacity took no part, so a larger one gives the same."""
import numpy as np
import pytest
import torch

import oracle
import lzs_compression_amd as lzs
from lzs_compression_amd import api as A
from lzs_compression_amd import workload
from conftest import golden_json

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
STARVED, END, FULL = 0x03, 0x04, 0x08
O = oracle.oracle()


# ---------------------------------------------------------------- helpers
def _pack(streams, stride=None, fill=0, rng=None, offset=0):
    """Rows of one tensor [n, stride] (viewed `offset` bytes behind an aligned base), what lies behind each stream filled
    with `fill` or with rng's bytes; and the lengths."""
    n = len(streams)
    longest = max([len(s) for s in streams] + [1])
    stride = stride or (longest + 15) // 16 * 16
    assert stride >= longest
    host = np.full((n, stride), fill, dtype=np.uint8) if rng is None else rng.integers(0, 256, (n, stride), dtype=np.uint8)
    for b, s in enumerate(streams):
        host[b, :len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    flat = torch.zeros(n * stride + 64, dtype=torch.uint8, device="cuda")
    flat[offset:offset + n * stride] = torch.from_numpy(host.reshape(-1)).cuda()
    x = flat[offset:offset + n * stride].view(n, stride)
    assert x.data_ptr() % 16 == offset % 16
    return x, torch.tensor([len(s) for s in streams], dtype=torch.int32, device="cuda")


def _u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def _oracle(x, xl, limit, bound=None, states=None):
    """(length, status) of the channel decoder on fresh channels (or `states`), the block decoder's length asserted equal."""
    n = x.shape[0]
    cap = limit
    if limit == NONE:
        cap = bound if bound is not None else 30 * x.shape[1] + 16
    st = lzs.new_channel_states(n) if states is None else states.clone()
    _, cl, cs = lzs.decompress_channels(x, xl, None, st, cap)
    _, bl = lzs.decompress_blocks(x, xl, cap)
    torch.cuda.synchronize()
    cl, cs, bl = _u32(cl), cs.cpu().numpy(), _u32(bl)
    assert (cl == bl).all(), "the oracles disagree"
    if limit == NONE:
        assert (cl < cap).all() and (cs != FULL).all(), "the oracle's capacity is not above every size"
    return cl, cs


def _query(x, xl, limit):
    size, status = lzs.decompressed_sizes(x, xl, None if limit == NONE else limit)
    torch.cuda.synchronize()
    return _u32(size), status.cpu().numpy()


def _check(x, xl, limit, what, bound=None, states=None):
    want = _oracle(x, xl, limit, bound, states)
    got = _query(x, xl, limit)
    bad = np.nonzero((got[0] != want[0]) | (got[1] != want[1]))[0]
    assert bad.size == 0, (what, limit, [(int(b), int(got[0][b]), int(got[1][b]), int(want[0][b]), int(want[1][b])) for b in bad[:8]])
    return got


def _bits(*tokens):
    s = "".join(tokens)
    assert len(s) % 8 == 0, len(s)
    return bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))


def _lit(c):
    return "0" + f"{c:08b}"


def _short(off):
    return "11" + f"{off:07b}"


def _long(off):
    return "10" + f"{off:011b}"


MARKER = "110000000"


# ---------------------------------------------------------------- 1. hand-built streams
HAND = {
    "empty": (b"", 0, STARVED),
    "lone marker": (b"\xC0\x00", 0, END),
    "marker then garbage": (b"\xC0\x00" + bytes(range(37, 90)), 0, END),
    "literal without its ninth bit": (b"\x20", 0, STARVED),
    "offset without its length": (_bits(_lit(65), _lit(66), _lit(67), _long(2)), 3, STARVED),
    "length 8 without its nibble": (_bits(_lit(65), _lit(66), _lit(67), _short(3), "1111"), 11, STARVED),
    "long length 8 without its nibble": (_bits(*[_lit(65 + i) for i in range(7)], _long(7), "1111"), 15, STARVED),
    "long offset 0 in mid-stream": (_bits(_lit(65), _long(0), _lit(66), MARKER), 2, END),
    "no end marker": (_bits(*[_lit(97 + i) for i in range(8)]), 8, STARVED),
    "marker after a match": (_bits(_lit(65), _short(1), "00", MARKER, "000"), 3, END),
}


def _hand_streams():
    """(name, stream, size and status or None) of every hand-built stream and of the streams of inc_garbage.json, each as a block"""
    cases = [(k, v[0], v[1], v[2]) for k, v in HAND.items()]
    chain = O.compress(bytes(1000))
    assert len(chain) < 60                                 # one literal, one offset and 66 nibbles of 15
    cases.append(("F nibbles", chain, 1000, END))
    for v in golden_json("inc_garbage.json"):
        cases.append(("inc_garbage " + v["in"][:16], bytes.fromhex(v["in"]), None, None))      # (garbage: the decoders say what)
    return cases


def test_hand_built_streams():
    cases = _hand_streams()
    x, xl = _pack([c[1] for c in cases], fill=0xFF)
    size, status = _check(x, xl, NONE, "hand-built")
    for b, (name, _, want_size, want_status) in enumerate(cases):
        assert want_size is None or (size[b], status[b]) == (want_size, want_status), (name, b, size[b], status[b])
    for limit in (0, 1, 2, 3, 8, 11, 999, 1000):
        _check(x, xl, limit, "hand-built")


def test_edge_vectors_of_the_decoder(edge_vectors):
    by_cap = {}
    for v in edge_vectors["decompress"]:
        for cap, out in v["out"].items():
            by_cap.setdefault(int(cap), []).append((bytes.fromhex(v["in"]), len(out) // 2, v["name"]))
    for cap, cases in sorted(by_cap.items()):
        x, xl = _pack([c[0] for c in cases], fill=0xA5)
        size, _ = _check(x, xl, cap, "edge vectors")
        for b, c in enumerate(cases):
            assert size[b] == c[1], (c[2], cap, size[b], c[1])


# ---------------------------------------------------------------- 2. limits
def test_limits_around_the_true_size():
    text = workload.fill("text", 1, 9000)[0]
    raws = [b"x" * 100,                                    # S - 1 falls inside a copy (the last token but the marker is one)
            b"x" * 24,                                     # ... a copy that ends on a closing length nibble 0
            bytes(range(200)),                             # S - 1 falls on a literal
            text[:5000].tobytes(), text[:1].tobytes(), workload.fill("lowent", 1, 9000)[0, :7777].tobytes()]
    streams = [O.compress(r) for r in raws]
    x, xl = _pack(streams)
    for b, r in enumerate(raws):
        S = len(r)
        for limit in sorted({S, S - 1, S // 2, 1, 0, S + 1, NONE}):
            size, status = _check(x[b:b + 1], xl[b:b + 1], limit, f"stream {b}", bound=16384)
            if limit >= S:
                assert (size[0], status[0]) == (S, END), (b, limit, size[0], status[0])       # S exactly: the marker needs no room
            else:
                assert (size[0], status[0]) == (limit, FULL), (b, limit, size[0], status[0])   # ... although the marker follows


# ---------------------------------------------------------------- 3. differential, seeded
STRIDE = 10144                                             # compressed_max(9000) = 10128


def _mixed_streams():
    rng = np.random.default_rng(20241)
    raw, raw_len = [], []
    for cls in ("text", "lowent", "random"):
        blk = workload.fill(cls, 445, 9000)
        for b in range(445):
            raw.append(blk[b])
            raw_len.append(int(rng.integers(0, 9001)))
    x = torch.from_numpy(np.stack(raw)).cuda()
    slots, lens = lzs.compress_blocks(x, torch.tensor(raw_len, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    slots, lens = slots.cpu().numpy(), lens.cpu().numpy()
    streams, whole = [], []
    for b in range(len(raw)):
        s = slots[b, :lens[b]].tobytes()
        if b % 2:                                          # a third of the batch: cut at a random byte
            s = s[:int(rng.integers(0, len(s) + 1))]
        streams.append(s)
        whole.append(raw_len[b] if b % 2 == 0 else -1)
    for _ in range(665):                                   # a third: uniform random bytes
        streams.append(rng.integers(0, 256, int(rng.integers(0, 301)), dtype=np.uint8).tobytes())
        whole.append(-1)
    order = rng.permutation(len(streams))
    return [streams[i] for i in order], np.array([whole[i] for i in order])


@pytest.fixture(scope="module")
def mixed():
    """About 2000 streams (a third whole, a third cut, a third garbage), packed twice with different bytes behind each stream,
    and the oracle's answers at the three limits -- computed once, never changed."""
    streams, whole = _mixed_streams()
    xa, xl = _pack(streams, STRIDE, rng=np.random.default_rng(1))
    xb, _ = _pack(streams, STRIDE, rng=np.random.default_rng(2))
    want = {limit: _oracle(xa, xl, limit, bound=16384) for limit in (NONE, 4096, 100)}
    return streams, whole, xa, xb, xl, want


def test_differential_against_the_decoders(mixed):
    streams, whole, xa, _, xl, want = mixed
    for limit in (NONE, 4096, 100):
        size, status = _query(xa, xl, limit)
        bad = np.nonzero((size != want[limit][0]) | (status != want[limit][1]))[0]
        assert bad.size == 0, (limit, [(int(b), len(streams[b]), int(size[b]), int(status[b]), int(want[limit][0][b]),
                                        int(want[limit][1][b])) for b in bad[:8]])
    size, status = _query(xa, xl, NONE)
    sel = whole >= 0
    assert (size[sel] == whole[sel]).all() and (status[sel] == END).all()       # whole streams: the raw length


def test_history_takes_no_part(mixed):
    _, _, xa, _, xl, want = mixed
    n = xa.shape[0]
    rng = np.random.default_rng(3)
    st = np.zeros((n, A.CHANNEL_STATE_BYTES), dtype=np.uint8)
    st[:, 64:64 + 2047] = rng.integers(0, 256, (n, 2047), dtype=np.uint8)
    st[:, :4] = np.frombuffer(np.uint32(2047).tobytes(), dtype=np.uint8)
    states = torch.from_numpy(st).cuda()
    for limit in (NONE, 4096, 100):
        _, cl, cs = lzs.decompress_channels(xa, xl, None, states.clone(), 16384 if limit == NONE else limit)
        size, status = _query(xa, xl, limit)
        assert (_u32(cl) == size).all() and (cs.cpu().numpy() == status).all()
        assert (size == want[limit][0]).all() and (status == want[limit][1]).all()


# ---------------------------------------------------------------- 4. shapes
def _short_valid():
    """30 literals, a match of 10, 5 literals, the marker: 43 bytes"""
    return O.compress(bytes(range(65, 95)) + b"ABCDEFGHIJ" + bytes(range(95, 100)))


def test_wavefront_and_grid_tails():
    rng = np.random.default_rng(4)
    text = workload.fill("text", 1, 9000)[0].tobytes()
    pool = [O.compress(text[i * 60:i * 60 + int(rng.integers(0, 200))]) for i in range(129)]
    for n in (1, 63, 64, 65, 129):
        x, xl = _pack(pool[:n], fill=0x5A)
        _check(x, xl, NONE, f"{n} blocks")
        _check(x, xl, 50, f"{n} blocks")
    # one long block among 127 of length 0 or 1
    streams = [bytes(int(rng.integers(0, 2))) for _ in range(128)]
    streams[77] = O.compress(text[:9000])
    x, xl = _pack(streams, fill=0xEE)
    size, status = _check(x, xl, NONE, "one long block", bound=16384)
    assert size[77] == 9000 and status[77] == END


def test_every_cut_of_a_short_stream_at_every_alignment():
    s = _short_valid()
    assert 40 <= len(s) <= 48
    cuts = [s[:k] for k in range(len(s) + 1)]              # in_len 0 .. 43: every refill of the bit buffer is some stream's last
    for stride, offset in ((48 + 1, 0), (64 + 1, 0), (64, 1), (64, 2), (64, 3), (64, 5), (1024 + 1, 3)):
        x, xl = _pack(cuts, stride=stride, fill=0xFF, offset=offset)
        size, status = _check(x, xl, NONE, (stride, offset))
        assert size[-1] == 45 and status[-1] == END
        _check(x, xl, 7, (stride, offset))


def test_uniform_length_without_a_length_array():
    rng = np.random.default_rng(6)
    text = workload.fill("text", 70, 3000)
    streams = [O.compress(text[b].tobytes()) for b in range(70)]
    n = min(len(s) for s in streams)                       # every row cut to the shortest: some whole, most cut
    x, _ = _pack([s[:n] for s in streams], stride=n + 17, rng=rng)
    assert x.shape[1] == n + 17
    xv = x[:, :n]                                          # rows of n bytes, stride n + 17
    want = _oracle(xv, None, NONE, bound=8192)
    got = _query(xv, None, NONE)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    got = _query(xv, None, 1000)
    want = _oracle(xv, None, 1000)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


def test_many_short_streams():
    """5000 streams of 0 .. 40 random bytes: 79 wavefronts, the last one with 8 streams."""
    rng = np.random.default_rng(7)
    pool = [rng.integers(0, 256, int(rng.integers(0, 41)), dtype=np.uint8).tobytes() for _ in range(5000)]
    x, xl = _pack(pool, stride=48, rng=rng)
    _check(x, xl, NONE, "5000 streams")


# ---------------------------------------------------------------- 5. nothing outside the block counts
def test_bytes_behind_a_stream_and_around_the_results(mixed):
    _, _, xa, xb, xl, want = mixed
    n = xa.shape[0]
    for limit in (NONE, 100):
        a, b = _query(xa, xl, limit), _query(xb, xl, limit)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    size = torch.full((n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    status = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    lzs.decompressed_sizes(xb, xl, None, size=size[8:8 + n], status=status[8:8 + n])
    torch.cuda.synchronize()
    assert (_u32(size[8:8 + n]) == want[NONE][0]).all() and (status[8:8 + n].cpu().numpy() == want[NONE][1]).all()
    for guard, v in ((size[:8], 0x5A5A5A5A), (size[8 + n:], 0x5A5A5A5A), (status[:8], 0xA5), (status[8 + n:], 0xA5)):
        assert bool((guard == v).all())


# ---------------------------------------------------------------- 6. no status array
def test_status_null_gives_the_same_sizes(mixed):
    _, _, xa, _, xl, want = mixed
    n = xa.shape[0]
    size = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc = A.lib().lzs_decompressed_size_batch_device(size.data_ptr(), None, xa.data_ptr(), xa.stride(0), xl.data_ptr(), xa.shape[1],
                                                    4096, n, A._stream_handle(None))
    torch.cuda.synchronize()
    assert rc == A.LZS_OK and (_u32(size) == want[4096][0]).all()


# ---------------------------------------------------------------- 7. graph capture
def test_graph_capture_equals_direct_calls():
    lzs.backend_info()                                     # the library's start-up, outside the graph
    rng = np.random.default_rng(8)
    text = workload.fill("text", 200, 2000)
    rounds = []
    for r in range(2):
        streams = [O.compress(text[(b + 100 * r) % 200, :int(rng.integers(0, 2001))].tobytes()) for b in range(100)]
        streams = [s[:int(rng.integers(0, len(s) + 1))] if b % 3 == 0 else s for b, s in enumerate(streams)]
        rounds.append(_pack(streams, stride=2304, rng=rng))
    direct = [tuple(t.clone() for t in lzs.decompressed_sizes(x, xl, 1500)) for x, xl in rounds]
    x_in, xl_in = rounds[0][0].clone(), rounds[0][1].clone()
    size = torch.empty(100, dtype=torch.int32, device="cuda")
    status = torch.empty(100, dtype=torch.uint8, device="cuda")
    lzs.decompressed_sizes(x_in, xl_in, 1500, size=size, status=status)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lzs.decompressed_sizes(x_in, xl_in, 1500, size=size, status=status)
    for r, (x, xl) in enumerate(rounds):
        x_in.copy_(x)
        xl_in.copy_(xl)
        size.fill_(-7)
        status.fill_(0xEE)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(size, direct[r][0]) and torch.equal(status, direct[r][1]), r
    assert not torch.equal(direct[0][0], direct[1][0])


# ---------------------------------------------------------------- 8. the dense decode
def test_dense_decode_round_trips_and_names_a_truncated_block():
    rng = np.random.default_rng(9)
    text = workload.fill("text", 300, 20000)
    raw_len = rng.integers(0, 20001, 300)
    raw_len[:3] = (0, 20000, 1)
    x = torch.from_numpy(text).cuda()
    slots, lens = lzs.compress_blocks(x, torch.tensor(raw_len, dtype=torch.int32, device="cuda"))
    dense, offsets = lzs.decompress_blocks_dense(slots, lens)
    torch.cuda.synchronize()
    offs = offsets.cpu().numpy()
    assert (offs == np.concatenate([[0], np.cumsum(raw_len)])).all()
    want = b"".join(text[b, :raw_len[b]].tobytes() for b in range(300))
    assert dense[:offs[-1]].cpu().numpy().tobytes() == want
    # nothing but empty blocks: every size is 0, the decode runs at a capacity of 0
    empty = torch.tensor([[0xC0, 0x00, 0x55, 0x55]] * 70, dtype=torch.uint8, device="cuda")
    dense0, offsets0 = lzs.decompress_blocks_dense(empty, torch.full((70,), 2, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert bool((offsets0 == 0).all()) and offsets0.numel() == 71
    cut = lens.clone()
    cut[137] -= 2                                          # the marker's bytes are gone
    with pytest.raises((ValueError, lzs.LzsError), match=r"\b137\b"):
        lzs.decompress_blocks_dense(slots, cut)
