"""The packed calls on the GPU (include/lzs/lzs_batch.h "PACKED streams"): lzs_offsets_from_sizes_device,
lzs_decompressed_size_packed_device, lzs_decompress_batch_packed_device and decompress_dense on top of them.

Expected bytes are the CPU oracle's (oracle.oracle().decompress), expected lengths and statuses those of the CPU model of the
decoders' rules (tests/test_decoded_size_host.py: model) -- never the code under test; the strided calls are a second witness.
Every decode is compared as ONE buffer: d_out and 64 bytes on either side are 0xA5 before the call, and afterwards every byte
is what the expectation says -- the blocks' bytes at their offsets, 0xA5 everywhere else (containment)."""
import functools
import random

import numpy as np
import pytest
import torch

import oracle
import lzs_compression_amd as lzs
from lzs_compression_amd import workload
from test_decoded_size_host import model
from test_gpu_decoded_size import HAND

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
STARVED, END, FULL, ERROR = 0x03, 0x04, 0x08, 0x10
FILL, GUARD = 0xA5, 64
BLOCK_MAX = 3 << 30
O = oracle.oracle()


# ---------------------------------------------------------------- the streams, made once
class Stream:
    """A stream, the bytes it decodes to without a limit, and its size and status there (the model's)."""

    def __init__(self, name, data):
        self.name, self.data = name, bytes(data)
        self.size, self.status = model(self.data, NONE)
        self.full = O.decompress(self.data, self.size + 1) if self.size else b""
        assert len(self.full) == self.size, (name, len(self.full), self.size)

    @functools.lru_cache(maxsize=None)
    def at(self, room):
        """(bytes, status) at a room of `room`: the oracle's prefix, of the model's length."""
        n, st = model(self.data, room)
        return self.full[:n], st


@functools.lru_cache(maxsize=None)
def pool():
    rng = random.Random(14)
    p = [Stream("hand: " + k, v[0]) for k, v in HAND.items()]
    for k, v in HAND.items():
        assert (p[list(HAND).index(k)].size, p[list(HAND).index(k)].status) == (v[1], v[2]), k
    text = O.compress(workload.fill("text", 1, 4000)[0].tobytes())
    p += [Stream(f"text cut to {n} bytes", text[:n]) for n in (0, 1, 3, 4, 5, 127, 128, 129)]   # the 128-byte chunk, the first word
    for cls in ("text", "lowent", "random"):
        blk = workload.fill(cls, 4, 9000)
        p += [Stream(f"{cls} block {b}", O.compress(blk[b, :rng.randrange(0, 9001)].tobytes())) for b in range(4)]
    return p


@functools.lru_cache(maxsize=None)
def big(cls):
    """One 64 KiB block: its lanes finish long after its neighbours', and its window wraps many times."""
    return Stream(f"{cls} 64 KiB", O.compress(workload.fill(cls, 1, 1 << 16)[0].tobytes()))


def batches():
    """(name, streams): 1, 7, 8, 9 and 17 blocks out of the pool, every stream of it in some batch; a large block of each class
    among tiny ones; the whole pool, and once more in reverse (with it every residue of an offset mod 16 occurs)."""
    p = pool()
    out, at = [], 0
    for n in (1, 7, 8, 9, 17):
        out.append((f"{n} blocks", [p[(at + i) % len(p)] for i in range(n)]))
        at += n
    assert at >= len(p)
    for cls in ("text", "lowent", "random"):
        tiny = [s for s in p if len(s.data) < 130][:8]
        out.append((f"64 KiB of {cls} among tiny ones", tiny[:3] + [big(cls)] + tiny[3:]))
    out.append(("the whole pool", list(p)))
    out.append(("the pool in reverse", list(reversed(p))))
    return out


# ---------------------------------------------------------------- layout and the one comparison
def round_up(v, a):
    return (v + a - 1) // a * a


def offsets_of(rooms, align=1):
    off = np.zeros(len(rooms) + 1, dtype=np.int64)
    off[1:] = np.cumsum([round_up(r, align) for r in rooms])
    return off


def place_input(streams, shuffle=None):
    """The streams back to back in one tensor whose first byte lies one byte behind an aligned address.  Returns (data, in_off
    [n + 1], in_len); with `shuffle` (a random.Random) the streams lie in a shuffled order and only in_len says how long they are."""
    order = list(range(len(streams)))
    if shuffle:
        shuffle.shuffle(order)
    start, at = [0] * len(streams), 0
    for b in order:
        start[b] = at
        at += len(streams[b].data)
    host = np.zeros(at + 1 + 64, dtype=np.uint8)
    for b, s in enumerate(streams):
        host[1 + start[b]:1 + start[b] + len(s.data)] = np.frombuffer(s.data, dtype=np.uint8)
    flat = torch.from_numpy(host).cuda()
    assert flat.data_ptr() % 16 == 0
    data = flat[1:1 + at]
    in_off = torch.tensor(start + [at], dtype=torch.int64, device="cuda")
    in_len = torch.tensor([len(s.data) for s in streams], dtype=torch.int32, device="cuda")
    return data, in_off, in_len


def decode(data, in_off, in_len, out_off_host, total):
    """One packed decode into a buffer of 0xA5 with guards.  Returns (the whole buffer, out_len) on the host."""
    buf = torch.full((GUARD + 1 + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[GUARD + 1:GUARD + 1 + total]
    out_off = torch.from_numpy(np.asarray(out_off_host, dtype=np.int64)).cuda()
    _, out_len = lzs.decompress_packed(data, in_off, out, out_off, in_len=in_len)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), out_len.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def expect(tag, got, got_len, out_off, want):
    """`want`: per block the bytes it must have written (b"" for none)."""
    buf = np.full(got.shape, FILL, dtype=np.uint8)
    for b, w in enumerate(want):
        at = GUARD + 1 + int(out_off[b])
        buf[at:at + len(w)] = np.frombuffer(w, dtype=np.uint8)
    want_len = np.array([len(w) for w in want], dtype=np.int64)
    assert np.array_equal(got_len, want_len), (tag, np.nonzero(got_len != want_len)[0][:8].tolist(), got_len[:20].tolist(), want_len[:20].tolist())
    bad = np.nonzero(got != buf)[0]
    if bad.size:
        i = int(bad[0]) - GUARD - 1
        b = int(np.searchsorted(np.asarray(out_off), i, side="right")) - 1
        raise AssertionError(f"{tag}: {bad.size} bytes differ, the first at d_out[{i}] (block {b}, its offset {int(out_off[max(b, 0)])}, "
                             f"its length {int(want_len[max(b, 0)])}): {got[bad[0]:bad[0] + 8].tobytes().hex()}, expected "
                             f"{buf[bad[0]:bad[0] + 8].tobytes().hex()}")


# ---------------------------------------------------------------- 1. group edges, alignments, containment
@pytest.mark.parametrize("align", (1, 4, 16))
def test_group_edges_and_containment(align):
    """Batches of 1, 7, 8, 9 and 17 blocks (a wavefront takes eight), input lengths 0, 1, 3, 4, 5, 127, 128, 129, a 64 KiB block
    among tiny ones, every room exactly the block's size (rounded up to `align`), in_len absent and given."""
    seen_out, seen_in = set(), set()
    for name, streams in batches():
        rooms = [s.size for s in streams]
        off = offsets_of(rooms, align)
        for shuffled in (False, True):
            data, in_off, in_len = place_input(streams, random.Random(len(streams)) if shuffled else None)
            got, got_len = decode(data, in_off, in_len if shuffled else None, off, int(off[-1]))
            expect(f"{name}, align {align}, {'shuffled with lengths' if shuffled else 'dense'}", got, got_len, off, [s.full for s in streams])
            seen_in |= {int(v) % 4 for v in in_off.cpu().numpy()[:-1]}
        seen_out |= {int(v) % 16 for v in off[:-1]}
    assert seen_in == set(range(4))
    assert seen_out == (set(range(16)) if align == 1 else set(range(0, 16, align)))


def test_cut_rooms():
    """Each block's room its size, its size - 1, half of it, 0 -- mixed within one wavefront: the oracle's prefix, the model's
    length; the next block's first byte lies right behind the room."""
    for name, streams in batches():
        for shift in range(4):
            rooms = [(s.size, max(s.size - 1, 0), s.size // 2, 0)[(b + shift) % 4] for b, s in enumerate(streams)]
            off = offsets_of(rooms)
            data, in_off, _ = place_input(streams)
            got, got_len = decode(data, in_off, None, off, int(off[-1]))
            expect(f"{name}, cut rooms, shift {shift}", got, got_len, off, [s.at(r)[0] for s, r in zip(streams, rooms)])


def test_sizes_and_statuses():
    """The packed size query: the model's length and status at limits none, 100, 1 and 0, streams dense and shuffled."""
    for name, streams in batches():
        for shuffled in (False, True):
            data, in_off, in_len = place_input(streams, random.Random(7) if shuffled else None)
            for limit in (NONE, 100, 1, 0):
                size, status = lzs.decompressed_sizes_packed(data, in_off, in_len if shuffled else None, None if limit == NONE else limit)
                torch.cuda.synchronize()
                want = [s.at(limit) for s in streams]
                got = list(zip((size.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist(), status.cpu().numpy().tolist()))
                assert got == [(len(w), st) for w, st in want], (name, shuffled, limit)


def test_equal_to_the_strided_calls():
    """A second witness beside the oracle: the same streams through decompress_blocks and decompressed_sizes, one call per
    distinct room -- lengths and bytes equal, and for the size query the statuses."""
    _, streams = batches()[4]                                      # 17 blocks
    rooms = [(s.size, max(s.size - 1, 0), s.size // 2, 0)[b % 4] for b, s in enumerate(streams)]
    off = offsets_of(rooms)
    data, in_off, in_len = place_input(streams)
    got, got_len = decode(data, in_off, None, off, int(off[-1]))
    stride = round_up(max(len(s.data) for s in streams) + 1, 16)
    host = np.zeros((len(streams), stride), dtype=np.uint8)
    for b, s in enumerate(streams):
        host[b, :len(s.data)] = np.frombuffer(s.data, dtype=np.uint8)
    x = torch.from_numpy(host).cuda()
    for room in sorted(set(rooms)):
        out, out_len = lzs.decompress_blocks(x, in_len, room)
        size, status = lzs.decompressed_sizes(x, in_len, room)
        psize, pstatus = lzs.decompressed_sizes_packed(data, in_off, None, room)
        torch.cuda.synchronize()
        assert torch.equal(size, psize) and torch.equal(status, pstatus), room
        out, out_len = out.cpu().numpy(), out_len.cpu().numpy()
        for b in (b for b, r in enumerate(rooms) if r == room):
            at = GUARD + 1 + int(off[b])
            assert got_len[b] == out_len[b], (room, b)
            assert np.array_equal(got[at:at + got_len[b]], out[b, :out_len[b]]), (room, b)


# ---------------------------------------------------------------- 2. entries that are not blocks
def test_entries_that_are_not_blocks():
    """A decreasing pair in in_off, a decreasing pair in out_off, an in_len above LZS_BLOCK_MAX: length 0, ERROR from the size
    query, nothing written, and the other blocks right."""
    good = [s for s in pool() if s.status == END and s.size > 0][:8]
    g = [s.data for s in good]
    # (a) in_off = [p0, p1, p3, p2, p3, ...]: entry 2 starts behind where entry 3 starts, its pair decreases; entry 1 runs on
    # over stream 2, behind its own end marker, which the decoders ignore; entry 3 is stream 2
    blob = b"".join(g)
    p, at = [], 0
    for d in g:
        p.append(at)
        at += len(d)
    in_off_host = [p[0], p[1], p[3], p[2]] + p[3:] + [len(blob)]
    entry = [good[0], good[1], None] + good[2:]
    assert len(in_off_host) == len(entry) + 1
    flat = torch.from_numpy(np.concatenate([np.zeros(1, dtype=np.uint8), np.frombuffer(blob, dtype=np.uint8), np.zeros(16, dtype=np.uint8)])).cuda()
    data = flat[1:1 + len(blob)]
    in_off = torch.tensor(in_off_host, dtype=torch.int64, device="cuda")
    rooms = [e.size if e else 5 for e in entry]
    off = offsets_of(rooms)
    got, got_len = decode(data, in_off, None, off, int(off[-1]))
    expect("decreasing in_off", got, got_len, off, [e.full if e else b"" for e in entry])
    size, status = lzs.decompressed_sizes_packed(data, in_off)
    torch.cuda.synchronize()
    assert size.cpu().numpy().tolist() == [e.size if e else 0 for e in entry]
    assert status.cpu().numpy().tolist() == [e.status if e else ERROR for e in entry]

    # (b) out_off decreases at entry 3; (c) in_len[5] is above LZS_BLOCK_MAX
    data, in_off, in_len = place_input(good)
    rooms = [s.size for s in good]
    off = offsets_of(rooms)
    off_b = off.copy()
    off_b[3] = off[4] + 7                                          # entry 2's room grows, entry 3's pair decreases
    total = int(off_b.max())
    got, got_len = decode(data, in_off, None, off_b, total)
    expect("decreasing out_off", got, got_len, off_b, [s.full if b != 3 else b"" for b, s in enumerate(good)])
    lens = np.array([len(s.data) for s in good], dtype=np.uint32)
    lens[5] = BLOCK_MAX + 1
    in_len_c = torch.from_numpy(lens.view(np.int32).copy()).cuda()
    got, got_len = decode(data, in_off, in_len_c, off, int(off[-1]))
    expect("a length above LZS_BLOCK_MAX", got, got_len, off, [s.full if b != 5 else b"" for b, s in enumerate(good)])
    size, status = lzs.decompressed_sizes_packed(data, in_off, in_len_c)
    torch.cuda.synchronize()
    assert size.cpu().numpy().tolist() == [s.size if b != 5 else 0 for b, s in enumerate(good)]
    assert status.cpu().numpy().tolist() == [s.status if b != 5 else ERROR for b, s in enumerate(good)]


# ---------------------------------------------------------------- 3. more than 32 bits apart
def test_far_apart():
    """Two short streams 5 GiB apart with six empty ones between them in one wavefront: its input extent exceeds 32 bits.
    Then two outputs 5 GiB apart.  The large tensor is never filled."""
    far = 5 << 30
    raw = workload.fill("text", 2, 1500)
    a, b = (Stream(f"far {k}", O.compress(raw[k].tobytes())) for k in range(2))
    assert a.size == b.size == 1500 and max(len(a.data), len(b.data)) < 2000
    space = torch.empty(far + 4096, dtype=torch.uint8, device="cuda")
    for at, s in ((64, a), (far + 64, b)):
        space[at:at + len(s.data)] = torch.from_numpy(np.frombuffer(s.data, dtype=np.uint8).copy()).cuda()
    in_off = torch.tensor([64] + [64 + len(a.data)] * 6 + [far + 64], dtype=torch.int64, device="cuda")
    in_len = torch.tensor([len(a.data)] + [0] * 6 + [len(b.data)], dtype=torch.int32, device="cuda")
    rooms = [a.size] + [3] * 6 + [b.size]
    off = offsets_of(rooms)
    got, got_len = decode(space, in_off, in_len, off, int(off[-1]))
    expect("inputs 5 GiB apart", got, got_len, off, [a.full] + [b""] * 6 + [b.full])
    size, status = lzs.decompressed_sizes_packed(space, in_off, in_len)
    torch.cuda.synchronize()
    assert size.cpu().numpy().tolist() == [a.size] + [0] * 6 + [b.size]

    data, in_off2, _ = place_input([a, b])
    out_off = torch.tensor([65, 65 + a.size, far + 65, far + 65 + b.size], dtype=torch.int64, device="cuda")   # entry 1: a room of 5 GiB, clamped
    in_off3 = torch.tensor([int(in_off2[0]), int(in_off2[1]), int(in_off2[1]), int(in_off2[2])], dtype=torch.int64, device="cuda")
    for at, n in ((1, a.size + 128), (far + 1, b.size + 128)):
        space[at:at + n] = FILL
    _, out_len = lzs.decompress_packed(data, in_off3, space, out_off)
    torch.cuda.synchronize()
    assert out_len.cpu().numpy().tolist() == [a.size, 0, b.size]
    for at, s in ((65, a), (far + 65, b)):
        region = space[at - 64:at + s.size + 64].cpu().numpy()
        want = np.full(region.shape, FILL, dtype=np.uint8)
        want[64:64 + s.size] = np.frombuffer(s.full, dtype=np.uint8)
        assert np.array_equal(region, want), at


# ---------------------------------------------------------------- 4. offsets from sizes
@pytest.mark.parametrize("n", (0, 1, 1023, 1024, 1025, 70000))
def test_offsets_from_sizes(n):
    """Against numpy.cumsum: sizes with 0 and 0xFFFFFFFF among them (the sum needs 64 bits), align 1, 16 and 256."""
    rng = np.random.default_rng(n)
    size = rng.integers(0, 70000, n, dtype=np.uint64)
    size[rng.random(n) < 0.1] = 0
    size[rng.random(n) < 0.1] = 0xFFFFFFFF
    if n:
        size[0], size[-1] = 0xFFFFFFFF, 0 if n > 1 else 0xFFFFFFFF
    dev = torch.from_numpy(size.astype(np.uint32).view(np.int32)).cuda()
    for align in (1, 16, 256):
        want = np.zeros(n + 1, dtype=np.uint64)
        want[1:] = np.cumsum((size + np.uint64(align - 1)) & ~np.uint64(align - 1), dtype=np.uint64)
        got = lzs.offsets_from_sizes(dev, align)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy().view(np.uint64), want), (n, align)
    if n:
        assert int(want[-1]) > 0xFFFFFFFF


# ---------------------------------------------------------------- 5. decompress_dense
def _compressed_batch(nb, longest, seed):
    """(raw rows, their lengths, the compressed streams compacted: dense, offsets)"""
    rng = np.random.default_rng(seed)
    raw = np.concatenate([workload.fill(cls, (nb + 2) // 3, longest) for cls in ("text", "lowent", "random")])[:nb]
    lens = rng.integers(0, longest + 1, nb)
    lens[:3] = (0, 1, longest)
    x = torch.from_numpy(raw).cuda()
    slots, clen = lzs.compress_blocks(x, torch.tensor(lens, dtype=torch.int32, device="cuda"))
    dense, offsets = lzs.compact(slots, clen)
    torch.cuda.synchronize()
    return raw, lens, dense[:int(offsets[-1])].clone(), offsets


@pytest.mark.parametrize("align", (1, 16))
def test_decompress_dense_round_trip(align):
    raw, lens, dense, offsets = _compressed_batch(100, 5000, 3)
    out, off = lzs.decompress_dense(dense, offsets, align=align)
    torch.cuda.synchronize()
    o, off = out.cpu().numpy(), off.cpu().numpy()
    want = offsets_of(lens.tolist(), align)
    assert np.array_equal(off, want) and o.size == want[-1]
    for b in range(len(lens)):
        assert np.array_equal(o[off[b]:off[b] + lens[b]], raw[b, :lens[b]]), b


def test_decompress_dense_names_the_truncated_block():
    raw, lens, dense, offsets = _compressed_batch(20, 3000, 4)
    in_len = (offsets[1:] - offsets[:-1]).to(torch.int32)
    in_len[13] -= 2                                                # its end marker is gone
    with pytest.raises(ValueError, match="block 13 does not end in an end marker"):
        lzs.decompress_dense(dense, offsets, in_len=in_len)


def test_decompress_dense_of_no_blocks():
    out, off = lzs.decompress_dense(torch.empty(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert out.numel() == 0 and off.cpu().numpy().tolist() == [0]


def test_decompress_dense_peak_memory():
    """The stated peak is the result and two small arrays, the sizes (int32 [nblocks]) and the offsets (int64 [nblocks + 1]).
    The condition: what the call allocates at its peak, above what was allocated before it, is at most the result plus TWICE
    those two arrays -- the second time for what the check of the statuses holds for a moment --, every allocation rounded up
    to the allocator's 512 bytes.  The slots decompress_blocks_dense needs beside its result, nblocks * max(size) bytes, are
    twice this whole bound here (the blocks' mean size is half the largest)."""
    nb, longest = 4096, 5000
    raw, lens, dense, offsets = _compressed_batch(nb, longest, 5)
    total = int(lens.sum())
    r512 = lambda v: round_up(v, 512)
    bound = r512(total) + 2 * (r512(4 * nb) + r512(8 * (nb + 1)))
    assert 1.8 * bound < nb * longest
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, off = lzs.decompress_dense(dense, offsets)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"decompress_dense: peak {peak} bytes above the inputs, bound {bound}, result {total}")
    assert out.numel() == total
    assert peak <= bound, (peak, bound, total)
