"""Packed compression on the GPU (include/lzs/lzs_batch.h "PACKED COMPRESSION"): lzs_compressed_bound_packed_device,
lzs_compress_batch_packed_device, lzs_compact_packed_device and compress_dense on top of them.

Expected bytes are the CPU oracle's alone -- oracle.oracle().compress(data, room) -- never the code under test; the strided call
is a second witness.  The blocks lie back to back in one tensor whose first byte is one byte behind a 16-aligned address
(place_input of tests/test_gpu_packed.py); d_out and 64 guard bytes on either side are 0xA5 before every call."""
import functools
import random

import numpy as np
import pytest
import torch

import oracle
import lzs_compression_amd as lzs
from lzs_compression_amd import workload
from test_gpu_packed import FILL, GUARD, BLOCK_MAX, offsets_of, place_input, round_up

pytestmark = pytest.mark.gpu

O = oracle.oracle()
EDGES = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4000)      # 2048 | 2049: the classifier's threshold
CLASSES = ("text", "lowent", "random")


# ---------------------------------------------------------------- the blocks, made once
class Block:
    """A block, the oracle's stream of it, and the oracle's stream at any room."""

    def __init__(self, name, data):
        self.name, self.data = name, bytes(data)
        self.full = O.compress(self.data)
        self.L = len(self.full)

    @functools.lru_cache(maxsize=None)
    def at(self, room):
        got = self.full if room >= self.L else O.compress(self.data, room)
        assert len(got) == min(self.L, room)
        return got


@functools.lru_cache(maxsize=None)
def pool():
    """The edge lengths, the classes in turn, and four random lengths to 9000 of each class."""
    rng = random.Random(15)
    raw = {cls: workload.fill(cls, 12, 9000) for cls in CLASSES}
    p = [Block(f"{CLASSES[i % 3]} of {n} bytes", raw[CLASSES[i % 3]][i // 3, :n].tobytes()) for i, n in enumerate(EDGES)]
    for cls in CLASSES:
        p += [Block(f"{cls} block {b}", raw[cls][6 + b, :rng.randrange(0, 9001)].tobytes()) for b in range(4)]
    return p


@functools.lru_cache(maxsize=None)
def big(cls):
    return Block(f"{cls} 64 KiB", workload.fill(cls, 1, 1 << 16)[0].tobytes())


@functools.lru_cache(maxsize=None)
def classified(n, seed=16):
    """`n` blocks of 2049 to 5000 bytes, the three classes in turn: in a launch of kClassifyMinBlocks blocks and more every
    variant of the kernel serves some of them."""
    rng = random.Random(seed + n)
    raw = {cls: workload.fill(cls, (n + 2) // 3, 5000, first_block=40) for cls in CLASSES}
    return [Block(f"{CLASSES[i % 3]} classified {i}", raw[CLASSES[i % 3]][i // 3, :rng.choice((2049, 2049 + rng.randrange(2952)))].tobytes())
            for i in range(n)]


def batches():
    """(name, blocks): 1, 7 and 63 blocks out of the pool (every block of it in some batch), 64 and 65 blocks of at least 2049
    bytes of all three classes (64 is kClassifyMinBlocks), a 64 KiB block of each class among tiny ones."""
    p = pool()
    out, at = [], 0
    for n in (1, 7, 63):
        out.append((f"{n} blocks", [p[(at + i) % len(p)] for i in range(n)]))
        at += n
    assert at >= len(p)
    out += [(f"{n} classified blocks", classified(n)) for n in (64, 65)]
    tiny = [b for b in p if len(b.data) < 70][:8]
    out += [(f"64 KiB of {cls} among tiny ones", tiny[:3] + [big(cls)] + tiny[3:]) for cls in CLASSES]
    return out


# ---------------------------------------------------------------- one launch, one comparison
def launch(data, in_off, in_len, out_off_host, total):
    """One packed compression into a buffer of 0xA5 with guards.  Returns (the whole buffer, out_len) on the host."""
    buf = torch.full((GUARD + 1 + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[GUARD + 1:GUARD + 1 + total]
    out_off = torch.from_numpy(np.asarray(out_off_host, dtype=np.int64)).cuda()
    out_len = torch.full((len(out_off_host) - 1,), 0x55555555, dtype=torch.int32, device="cuda")       # (no length: an entry nobody wrote shows)
    lzs.compress_packed(data, in_off, out, out_off, in_len=in_len, out_len=out_len)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), out_len.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def expect(tag, got, got_len, out_off, rooms, want):
    """`want`: per block the bytes it must have written (b"" for none); rooms[b]: its room, of which the bytes past the length
    are unspecified -- every other byte of the buffer is compared: the streams, and 0xA5 outside all rooms."""
    buf = np.full(got.shape, FILL, dtype=np.uint8)
    known = np.ones(got.shape, dtype=bool)
    for b, w in enumerate(want):
        at = GUARD + 1 + int(out_off[b])
        known[at + len(w):at + rooms[b]] = False
    for b, w in enumerate(want):                                   # (after all the rooms: what a block must have written is known)
        at = GUARD + 1 + int(out_off[b])
        buf[at:at + len(w)] = np.frombuffer(w, dtype=np.uint8)
        known[at:at + len(w)] = True
    want_len = np.array([len(w) for w in want], dtype=np.int64)
    assert np.array_equal(got_len, want_len), (tag, np.nonzero(got_len != want_len)[0][:8].tolist(), got_len[:20].tolist(), want_len[:20].tolist())
    bad = np.nonzero((got != buf) & known)[0]
    if bad.size:
        i = int(bad[0]) - GUARD - 1
        b = int(np.argmax([int(out_off[k]) <= i < int(out_off[k]) + max(rooms[k], 1) for k in range(len(want))]))
        raise AssertionError(f"{tag}: {bad.size} bytes differ, the first at d_out[{i}] (near block {b}, its offset {int(out_off[b])}, its "
                             f"length {int(want_len[b])}, its room {rooms[b]}): {got[bad[0]:bad[0] + 8].tobytes().hex()}, expected "
                             f"{buf[bad[0]:bad[0] + 8].tobytes().hex()}")


def bounds_and_rooms(in_off, in_len, align, blocks):
    """The rooms as a caller makes them: compressed_bounds_packed, offsets_from_sizes.  The bounds are LZS_COMPRESSED_MAX."""
    bound = lzs.compressed_bounds_packed(in_off, in_len)
    off = lzs.offsets_from_sizes(bound, align)
    torch.cuda.synchronize()
    bound = bound.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert bound.tolist() == [lzs.compressed_max(len(b.data)) for b in blocks]
    off = off.cpu().numpy()
    assert np.array_equal(off, offsets_of(bound.tolist(), align))
    return bound.tolist(), off


# ---------------------------------------------------------------- 1. lengths and alignments
@pytest.mark.parametrize("align", (1, 4, 16))
def test_lengths_and_alignments(align):
    """Every batch with rooms from compressed_bounds_packed at `align`, with in_len in shuffled order and without in_len: out_len,
    bytes [0, len) of every room, and every byte outside all rooms."""
    seen_in = set()
    for name, blocks in batches():
        for shuffled in (False, True):
            data, in_off, in_len = place_input(blocks, random.Random(len(blocks)) if shuffled else None)
            lens = in_len if shuffled else None
            rooms, off = bounds_and_rooms(in_off, lens, align, blocks)
            got, got_len = launch(data, in_off, lens, off, int(off[-1]))
            expect(f"{name}, align {align}, {'shuffled with lengths' if shuffled else 'dense'}", got, got_len, off, rooms, [b.full for b in blocks])
            seen_in |= {(data.data_ptr() + int(v)) % 16 for v in in_off.cpu().numpy()[:-1]}
    assert len(seen_in) == 16


# ---------------------------------------------------------------- 2. cut rooms, to the byte
def test_cut_rooms_to_the_byte():
    """Rooms of L, L - 1, 1 and 0 bytes (L: the oracle's length) laid at align 1: every room is full or cut, so every byte of
    d_out is determined and the whole buffer is one comparison -- a block's last byte lies right before its neighbour's first."""
    for name, blocks in batches():
        for shift in range(4):
            rooms = [(b.L, b.L - 1, 1, 0)[(k + shift) % 4] for k, b in enumerate(blocks)]
            off = offsets_of(rooms)
            data, in_off, _ = place_input(blocks)
            got, got_len = launch(data, in_off, None, off, int(off[-1]))
            want = [b.at(r) for b, r in zip(blocks, rooms)]
            assert [len(w) for w in want] == rooms
            expect(f"{name}, cut rooms, shift {shift}", got, got_len, off, rooms, want)


# ---------------------------------------------------------------- 3. the strided call as a second witness
def test_equal_to_the_strided_call():
    """The same blocks through compress_blocks with out_capacity = the room, one call per distinct room: lengths and bytes equal."""
    blocks = pool()[:17] + classified(64)[:4]
    rooms = [(b.L, b.L - 1, lzs.compressed_max(len(b.data)), 1, 0)[k % 5] for k, b in enumerate(blocks)]
    off = offsets_of(rooms)
    data, in_off, in_len = place_input(blocks)
    got, got_len = launch(data, in_off, None, off, int(off[-1]))
    stride = round_up(max(len(b.data) for b in blocks) + 1, 16)
    host = np.zeros((len(blocks), stride), dtype=np.uint8)
    for k, b in enumerate(blocks):
        host[k, :len(b.data)] = np.frombuffer(b.data, dtype=np.uint8)
    x = torch.from_numpy(host).cuda()
    for room in sorted(set(rooms)):
        out, out_len = lzs.compress_blocks(x, in_len, room)
        torch.cuda.synchronize()
        out, out_len = out.cpu().numpy(), out_len.cpu().numpy()
        for k in (k for k, r in enumerate(rooms) if r == room):
            at = GUARD + 1 + int(off[k])
            assert got_len[k] == out_len[k], (room, k)
            assert np.array_equal(got[at:at + got_len[k]], out[k, :out_len[k]]), (room, k)


# ---------------------------------------------------------------- 4. entries that are not blocks
@pytest.mark.parametrize("n", (9, 70))
def test_entries_that_are_not_blocks(n):
    """A decreasing pair in in_off, an in_len above 3 GiB, a decreasing pair in out_off, in a batch of 9 and in one of 70 (the
    classifier's route): length 0, nothing written, the neighbours right; the bounds say 0 for the two input cases."""
    good = classified(70)[:n - 1]
    # (a) in_off = [p0, p1, p3, p2, p3, ...]: entry 2 starts behind where entry 3 starts, its pair decreases; entry 1 is
    # blocks 1 and 2 as one; entry 3 is block 2
    g = [b.data for b in good]
    blob = b"".join(g)
    p = np.concatenate([[0], np.cumsum([len(d) for d in g])]).tolist()
    in_off_host = [p[0], p[1], p[3], p[2]] + p[3:]
    entry = [good[0], Block("blocks 1 and 2 as one", g[1] + g[2]), None] + good[2:]
    assert len(in_off_host) == len(entry) + 1 == n + 1
    flat = torch.from_numpy(np.concatenate([np.zeros(1, dtype=np.uint8), np.frombuffer(blob, dtype=np.uint8), np.zeros(16, dtype=np.uint8)])).cuda()
    data = flat[1:1 + len(blob)]
    in_off = torch.tensor(in_off_host, dtype=torch.int64, device="cuda")
    bound = lzs.compressed_bounds_packed(in_off)
    torch.cuda.synchronize()
    rooms = [lzs.compressed_max(len(e.data)) if e else 0 for e in entry]
    assert (bound.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist() == rooms
    rooms[2] = 5                                                   # (a room it must not touch)
    off = offsets_of(rooms)
    got, got_len = launch(data, in_off, None, off, int(off[-1]))
    expect(f"decreasing in_off, {n} entries", got, got_len, off, rooms, [e.full if e else b"" for e in entry])

    # (b) in_len[5] is above LZS_BLOCK_MAX
    good = classified(70)[:n]
    data, in_off, in_len = place_input(good)
    lens = np.array([len(b.data) for b in good], dtype=np.uint32)
    lens[5] = BLOCK_MAX + 1
    in_len_b = torch.from_numpy(lens.view(np.int32).copy()).cuda()
    bound = lzs.compressed_bounds_packed(in_off, in_len_b)
    torch.cuda.synchronize()
    rooms = [lzs.compressed_max(len(b.data)) if k != 5 else 0 for k, b in enumerate(good)]
    assert (bound.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist() == rooms
    rooms[5] = 5
    off = offsets_of(rooms)
    got, got_len = launch(data, in_off, in_len_b, off, int(off[-1]))
    expect(f"a length above LZS_BLOCK_MAX, {n} entries", got, got_len, off, rooms, [b.full if k != 5 else b"" for k, b in enumerate(good)])

    # (c) out_off decreases at entry 3: entries 0..2 lie in an upper part of d_out, entry 3's pair leads from there back to 0,
    # entries 4.. lie in the lower part -- no two rooms overlap
    rooms = [lzs.compressed_max(len(b.data)) for b in good]
    low = offsets_of(rooms[4:])
    high = int(low[-1]) + 3 + offsets_of(rooms[:3])
    off_c = np.concatenate([high, low])                            # [h0, h1, h2, h3 | 0, l5, ...]: n + 1 entries
    assert len(off_c) == n + 1 and off_c[3] > off_c[4] == 0
    rooms[3] = 0
    got, got_len = launch(data, in_off, None, off_c, int(high[-1]))
    expect(f"decreasing out_off, {n} entries", got, got_len, off_c, rooms, [b.full if k != 3 else b"" for k, b in enumerate(good)])


# ---------------------------------------------------------------- 5. more than 32 bits apart, a room beyond 32 bits
def test_far_apart_and_a_room_of_more_than_4_gib():
    """Two blocks 5 GiB apart in the input; then outputs 5 GiB apart, the first block's room 5 GiB long (its out_cap is that
    clamped to 0xFFFFFFFF: the whole stream fits), an empty block between them.  The large tensor is never filled."""
    far = 5 << 30
    raw = workload.fill("text", 2, 3000)
    a, b = (Block(f"far {k}", raw[k].tobytes()) for k in range(2))
    space = torch.empty(far + 8192, dtype=torch.uint8, device="cuda")
    for at, blk in ((63, a), (far + 63, b)):
        space[at:at + len(blk.data)] = torch.from_numpy(np.frombuffer(blk.data, dtype=np.uint8).copy()).cuda()
    in_off = torch.tensor([63, far + 63], dtype=torch.int64, device="cuda")
    in_len = torch.tensor([3000, 3000], dtype=torch.int32, device="cuda")
    rooms = [lzs.compressed_max(3000)] * 2
    off = offsets_of(rooms)
    got, got_len = launch(space, in_off, in_len, off, int(off[-1]))
    expect("inputs 5 GiB apart", got, got_len, off, rooms, [a.full, b.full])

    # entry 0's room is 4 GiB and 64 bytes: clamped to 0xFFFFFFFF the stream fits; its low 32 bits alone would cut it at 64
    data, in_off2, _ = place_input([a, b])
    wide = (1 << 32) + 64
    in_off3 = torch.tensor([int(in_off2[0]), int(in_off2[1]), int(in_off2[1]), int(in_off2[2])], dtype=torch.int64, device="cuda")
    out_off = torch.tensor([65, wide + 65, wide + 65, wide + 65 + b.L], dtype=torch.int64, device="cuda")
    for at, n in ((1, a.L + 64), (wide + 65, b.L + 64)):
        space[at:at + n] = FILL
    out_len = torch.full((3,), 0x55555555, dtype=torch.int32, device="cuda")
    lzs.compress_packed(data, in_off3, space, out_off, out_len=out_len)
    torch.cuda.synchronize()
    assert out_len.cpu().numpy().tolist() == [a.L, 0, b.L]
    head = space[1:65 + a.L].cpu().numpy()                          # (what follows the stream in its room is unspecified)
    assert (head[:64] == FILL).all() and head[64:].tobytes() == a.full
    tail = space[wide + 65:wide + 65 + b.L + 64].cpu().numpy()
    assert tail[:b.L].tobytes() == b.full and (tail[b.L:] == FILL).all()


# ---------------------------------------------------------------- 6. compact_packed
@pytest.mark.parametrize("n", (0, 1, 255, 256, 257, 5000))
def test_compact_packed(n):
    """Random lengths with zeros among them, rooms at least as long laid with gaps at any alignment: offsets and dense bytes are
    numpy's."""
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 700, n)
    lens[rng.random(n) < 0.2] = 0
    rooms = lens + rng.integers(0, 9, n)
    src_off = offsets_of(rooms.tolist())
    src_host = rng.integers(0, 256, int(src_off[-1]) + 1, dtype=np.uint8)
    src = torch.from_numpy(src_host).cuda()[1:]
    dense, offsets = lzs.compact_packed(src, torch.from_numpy(src_off).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    want_off = offsets_of(lens.tolist())
    assert np.array_equal(offsets.cpu().numpy(), want_off)
    want = np.concatenate([src_host[1 + src_off[b]:1 + src_off[b] + lens[b]] for b in range(n)] + [np.zeros(0, dtype=np.uint8)])
    assert np.array_equal(dense[:want.size].cpu().numpy(), want)


# ---------------------------------------------------------------- 7. compress_dense
def _packed_rows(nb, longest, seed):
    """(blocks' bytes, data, in_off): `nb` blocks of the three classes, 0 .. `longest` bytes, back to back."""
    rng = np.random.default_rng(seed)
    raw = np.concatenate([workload.fill(cls, (nb + 2) // 3, longest) for cls in CLASSES])[:nb]
    lens = rng.integers(0, longest + 1, nb)
    lens[:3] = (0, 1, longest)
    rows = [raw[b, :lens[b]] for b in range(nb)]
    off = offsets_of(lens.tolist())
    flat = torch.from_numpy(np.concatenate([np.zeros(1, dtype=np.uint8)] + rows)).cuda()
    return rows, flat[1:], torch.from_numpy(off).cuda()


@pytest.mark.parametrize("align", (1, 16))
def test_compress_dense_is_the_oracles_streams_and_decodes_back(align):
    rows, data, in_off = _packed_rows(100, 5000, 6)
    dense, offsets = lzs.compress_dense(data, in_off, align=align)
    back, back_off = lzs.decompress_dense(dense, offsets)
    torch.cuda.synchronize()
    want = [O.compress(r.tobytes()) for r in rows]
    assert np.array_equal(offsets.cpu().numpy(), offsets_of([len(w) for w in want]))
    assert dense.cpu().numpy().tobytes() == b"".join(want)
    assert torch.equal(back, data) and torch.equal(back_off, in_off)


def test_compress_dense_of_no_blocks():
    dense, off = lzs.compress_dense(torch.empty(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert dense.numel() == 0 and off.cpu().numpy().tolist() == [0]


def test_compress_dense_peak_memory():
    """The stated peak: the rooms, the result and three small arrays (int32 [nblocks], two int64 [nblocks + 1]), every allocation
    rounded up to the allocator's 512 bytes, plus 1 MiB.  The strided route's slots alone, nblocks * (max(len) +
    LZS_COMPRESSED_MAX(max(len))) bytes, are more than one and a half times that here (the blocks' mean size is half the largest)."""
    nb, longest, align = 4096, 5000, 16
    rows, data, in_off = _packed_rows(nb, longest, 7)
    lens = [r.size for r in rows]
    r512 = lambda v: round_up(v, 512)
    rooms = sum(round_up(lzs.compressed_max(n), align) for n in lens)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dense, offsets = lzs.compress_dense(data, in_off, align=align)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    total = dense.numel()
    bound = r512(rooms) + r512(total) + r512(4 * nb) + 2 * r512(8 * (nb + 1)) + (1 << 20)
    print(f"compress_dense: peak {peak} bytes above the inputs, bound {bound}, rooms {rooms}, result {total}")
    assert 1.5 * bound < nb * (longest + lzs.compressed_max(longest))
    assert peak <= bound, (peak, bound, rooms, total)
    back, _ = lzs.decompress_dense(dense, offsets)
    assert torch.equal(back, data)


# ---------------------------------------------------------------- 8. graph capture
def test_compress_packed_captures_into_a_graph():
    """compress_packed of 70 blocks (the classifier's route: every variant is launched while capturing) captured once on one
    stream, replayed on text, then random, then lowent written into the same buffers: the oracle's bytes each time."""
    lzs.backend_info()                                             # (the one-time LDS ordering check happens here, not inside the capture)
    rng = random.Random(17)
    lens = [rng.randrange(2049, 6000) for _ in range(70)]
    in_off_host = offsets_of(lens)
    flat = torch.zeros(1 + int(in_off_host[-1]), dtype=torch.uint8, device="cuda")
    data = flat[1:]
    in_off = torch.from_numpy(in_off_host).cuda()
    rooms = [lzs.compressed_max(n) for n in lens]
    off = offsets_of(rooms)
    out_off = torch.from_numpy(off).cuda()
    buf = torch.full((GUARD + 1 + int(off[-1]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    out = buf[GUARD + 1:GUARD + 1 + int(off[-1])]
    out_len = torch.empty(70, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        lzs.compress_packed(data, in_off, out, out_off, out_len=out_len)       # once outside the capture (lazy module loading)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            lzs.compress_packed(data, in_off, out, out_off, out_len=out_len)
    for cls in ("text", "random", "lowent"):
        raw = workload.fill(cls, 70, 6000, first_block=7)
        blocks = [Block(f"{cls} {b}", raw[b, :n].tobytes()) for b, n in enumerate(lens)]
        data.copy_(torch.from_numpy(np.concatenate([raw[b, :n] for b, n in enumerate(lens)])))
        buf.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        expect(f"replay on {cls}", buf.cpu().numpy(), out_len.cpu().numpy().astype(np.int64), off, rooms, [b.full for b in blocks])
