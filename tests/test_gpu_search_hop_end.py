"""SEARCH of the default (text) variant of the compress kernel where a walk ENDS: on the farthest candidate of the window, on a
3-byte chain that holds nothing but candidates the one-byte probe rejects (the restart on the 2-byte chain), from an offset-1
seed, across a pool border, and in blocks and segments so short that lanes never take a position.  These are the places where a
change of the loop's rules -- a hop that may pass over the last candidate of a walk, say (profiles/r07/README.md) -- can go wrong
without the seeded classes noticing.  Every block: length and bytes against the oracle.

The contents are BUILT for the kernel's tables: grams that share a bucket of head3[1152] / head2[512] under the product's
multipliers are found by brute force here, and what the builders meant -- which token the parse takes at the position in
question -- is asserted on the oracle's token list before anything runs on the device.
"""
import ctypes

import numpy as np
import pytest

import oracle
import lzs_compression_amd as lzs
from lzs_compression_amd import workload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
O = oracle.oracle()

LENGTHS = (1, 2, 3, 4, 12, 13, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 2048 + 512 + 1, 4096 + 13, 65536)
BLOCK = 65536
HASH3_MUL, HEAD3 = 0x897397, 1152          # kernels/wgv_text_shape.inc
HASH2_MUL, HEAD2, HEAD2_SHIFT = 0x64EBAD33, 512, 7


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (no fallback exists)")
    assert "gfx950" in lzs.backend_info()


def bucket3(g: bytes) -> int:
    """wg_hash3x4 / 4: a 24-bit multiply mixes, a high multiply scales into the table."""
    t = g[0] | g[1] << 8 | g[2] << 16
    return ((((t * HASH3_MUL) & 0xFFFFFFFF) * (4 * HEAD3)) >> 32) >> 2


def bucket2(g: bytes) -> int:
    t = g[0] | g[1] << 8
    return (((t * HASH2_MUL) & 0xFFFFFFFF) >> HEAD2_SHIFT) & (HEAD2 - 1)


_text = None


def filler(n: int, at: int = 0) -> bytearray:
    """Seeded text (the class the default variant is chosen for); its bytes are printable ASCII and the line feed, so the
    builders' own grams -- the other bytes below 32 and those from 128 on -- occur nowhere else."""
    global _text
    if _text is None:
        _text = workload.fill("text", 4).tobytes()
        assert all(c == 10 or 32 <= c < 128 for c in set(_text))
    return bytearray(_text[at:at + n])


RARE = bytes(c for c in range(1, 32) if c != 10) + bytes(range(128, 256))


def grams_in_bucket3(g: bytes, count: int, third_equal: bool) -> list:
    """Other 3-grams of rare bytes in g's bucket whose third byte is (not) g's: the probe at offset 2 passes (fails) on them."""
    want, found = bucket3(g), []
    for a in RARE:
        for b in RARE:
            for c in ((g[2],) if third_equal else RARE):
                h = bytes((a, b, c))
                if h[:2] != g[:2] and (c == g[2]) == third_equal and a != g[0] and bucket3(h) == want:
                    found.append(h)
                    if len(found) == count:
                        return found
    raise AssertionError("not enough grams in the bucket")


def grams_in_bucket2(g: bytes, count: int) -> list:
    want, found = bucket2(g), []
    for a in RARE:
        for b in RARE:
            h = bytes((a, b))
            if h != g[:2] and a != g[0] and b != g[1] and bucket2(h) == want:
                found.append(h)
                if len(found) == count:
                    return found
    raise AssertionError("not enough 2-grams in the bucket")


def put(buf: bytearray, at: int, s: bytes) -> None:
    buf[at:at + len(s)] = s


def token_at(data: bytes, pos: int):
    """(offset, length) of the oracle's token that STARTS at pos (offset 0: a literal); None if the parse steps over pos."""
    for p, off, ln in O.trace(data):
        if p == pos:
            return int(off), int(ln)
        if p > pos:
            break
    return None


# ------------------------------------------------------------------------------------------------ the contents
# (every builder keeps its structure inside the first 2048 + 512 positions, so that the lengths from 2561 on hold all of it and
# the shorter ones cut through it: a position whose cap is what is left of the block)
G = bytes((0x81, 0x92, 0xA3))


def farthest_candidate(dist: int, long: bool) -> bytes:
    """G (or 12 bytes that begin with it) at position 1 and again `dist` further on; between them, nearer on the same chain,
    grams of the same bucket: some the probe rejects, some it lets through to a full step that finds no match."""
    b = filler(BLOCK)
    s = G + (bytes(range(0xB0, 0xB9)) if long else b"")
    put(b, 1, s + b"\x05")
    p = 1 + dist
    put(b, p, s + b"\x06")
    hits = grams_in_bucket3(G, 3, True) + grams_in_bucket3(G, 5, False)
    for k, h in enumerate(hits):                      # nearest first from p: a mixed order of the two kinds
        put(b, p - 40 - 37 * k, h)
    return bytes(b)


def rejectable_chain(with_2gram: bool) -> bytes:
    """At position p the 3-byte chain holds only grams of G's bucket whose third byte differs (a hop passes over every one of
    them, the last included); the 2-gram of G stands twice in the window, behind collisions of ITS bucket: the walk restarts
    on the 2-byte chain and the NEARER of the two is the answer.  Without the 2-gram: a literal."""
    b = filler(BLOCK)
    p = 1900
    put(b, p, G + b"\x07")
    for k, h in enumerate(grams_in_bucket3(G, 7, False)):
        put(b, p - 30 - 41 * k, h)
    if with_2gram:
        put(b, p - 700, G[:2] + b"\x08")
        put(b, p - 1500, G[:2] + b"\x09")
    for k, h in enumerate(grams_in_bucket2(G, 4)):
        put(b, p - 100 - 123 * k, h + b"\x0E")
    return bytes(b)


def seeded_with_longer_match_last(run: int, dist: int) -> bytes:
    """x r^run T at p - 1: position p, the run's second byte, is seeded by offset 1 with run - 1 bytes (2 .. 11); the same
    string stands `dist` before -- the last candidate of the window when dist is 2047 -- and matches to the cap; nearer on the
    chain of r r r, runs that end in another byte (what the probe at offset run - 1 rejects)."""
    b = filler(BLOCK)
    r = 0x9C
    T = bytes(range(0xC0, 0xCC))
    s = b"\x0B" + bytes([r]) * run + T
    p = 2100
    put(b, p - 1, s)
    put(b, p - 1 - dist, s)
    if run >= 4:
        for k in range(5):
            put(b, p - 60 - 97 * k, b"\x0C" + bytes([r]) * (run - 1) + bytes([0x0D + k]))
    return bytes(b)


BORDER_WALKERS = tuple(range(1536 + 500, 1536 + 531, 15))


def walks_over_a_pool_border() -> bytes:
    """Positions 500, 515 and 530 of the pool that begins at 1536 each hold a string of 12 bytes of their own, and before each
    ten candidates, every one a byte longer than the one before and FARTHER: each passes the probe and costs a full step, and
    the deciding one -- to the cap -- comes last.  Walks that the pool's SEARCH leaves unfinished and the next pool's ends."""
    b = filler(BLOCK)
    for j, p in enumerate(BORDER_WALKERS):
        g = bytes((0x81 + j, 0x92, 0xA3))
        tail = bytes(range(0xD0 + 16 * j, 0xDC + 16 * j))
        for k in range(10):                           # candidate k matches 3 + k bytes of g tail
            put(b, 1500 - 140 * k - 20 * j, g + tail[:k] + bytes([0x10 + k]))
        put(b, p, g + tail[:9] + bytes([0x1B + j]))
    return bytes(b)


CONTENTS = {
    "3-gram at 2047": lambda: farthest_candidate(2047, False),
    "3-gram at 2048": lambda: farthest_candidate(2048, False),
    "12 bytes at 2047": lambda: farthest_candidate(2047, True),
    "12 bytes at 2048": lambda: farthest_candidate(2048, True),
    "rejectable chain, 2-gram": lambda: rejectable_chain(True),
    "rejectable chain, no 2-gram": lambda: rejectable_chain(False),
    "seed 2, longer last": lambda: seeded_with_longer_match_last(3, 2047),
    "seed 5, longer last": lambda: seeded_with_longer_match_last(6, 2047),
    "seed 11, longer last": lambda: seeded_with_longer_match_last(12, 2040),
    "pool border": walks_over_a_pool_border,
    "text": lambda: bytes(filler(BLOCK, 65536)),
}


def test_the_builders_build_what_they_say():
    """No device: the oracle's parse takes the token each content was built for."""
    assert token_at(farthest_candidate(2047, False), 2048) == (2047, 3)
    assert token_at(farthest_candidate(2048, False), 2049) == (0, 1)
    assert token_at(farthest_candidate(2047, True), 2048) == (2047, 12)
    assert token_at(farthest_candidate(2048, True), 2049) == (0, 1)
    assert token_at(rejectable_chain(True), 1900) == (700, 2)
    assert token_at(rejectable_chain(False), 1900) == (0, 1)
    for run, dist in ((3, 2047), (6, 2047), (12, 2040)):
        d = seeded_with_longer_match_last(run, dist)
        assert token_at(d, 2100 - 1 - dist + 1) is not None
        # (x and the run's first byte are copied from `dist` before; so is everything up to the end of T)
        assert token_at(d, 2099) == (dist, 1 + run + 12)
    d = walks_over_a_pool_border()
    for j, p in enumerate(BORDER_WALKERS):
        assert token_at(d, p) == (p - (1500 - 140 * 9 - 20 * j), 12), p
    # the collisions are collisions: same bucket, other gram
    for h in grams_in_bucket3(G, 3, True) + grams_in_bucket3(G, 5, False):
        assert bucket3(h) == bucket3(G) and h != G
    for h in grams_in_bucket2(G, 4):
        assert bucket2(h) == bucket2(G) and h != G[:2]


def _compress_rows(rows, lens):
    x = torch.from_numpy(rows).cuda()
    slots, n = lzs.compress_blocks(x, torch.from_numpy(lens.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    return slots.cpu().numpy(), n.cpu().numpy()


def _variant_codes(rows, lens):
    L = lzs.lib()
    L.lzs_hip_classify_blocks.restype = ctypes.c_int
    L.lzs_hip_classify_blocks.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    x = torch.from_numpy(rows).cuda()
    n = torch.from_numpy(lens.astype(np.int32)).cuda()
    codes = torch.zeros(len(rows), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert L.lzs_hip_classify_blocks(codes.data_ptr(), x.data_ptr(), rows.shape[1], n.data_ptr(), rows.shape[1], len(rows), None) == 0
    torch.cuda.synchronize()
    return (codes.cpu().numpy().astype(np.int64) & 0xF).tolist()


@pytest.mark.parametrize("name", list(CONTENTS))
def test_every_length_of_a_built_content_gives_the_oracles_bytes(name):
    """One launch: the content cut to each of the lengths, a block each.  All of them are the default variant's."""
    data = CONTENTS[name]()
    rows = np.tile(np.frombuffer(data, dtype=np.uint8), (len(LENGTHS), 1))
    lens = np.array(LENGTHS, dtype=np.uint32)
    assert _variant_codes(rows, lens) == [1] * len(LENGTHS)
    out, n = _compress_rows(rows, lens)
    for b, ln in enumerate(LENGTHS):
        want = O.compress(data[:ln])
        assert int(n[b]) == len(want) and out[b, :n[b]].tobytes() == want, (name, ln)


@pytest.mark.parametrize("cls", workload.CLASS_NAMES)
def test_32_seeded_blocks_of_each_class(cls):
    blocks = workload.fill(cls, 32, first_block=1000)
    out, n = _compress_rows(blocks, np.full(32, BLOCK, dtype=np.uint32))
    for b in range(32):
        want = O.compress(blocks[b].tobytes())
        assert int(n[b]) == len(want) and out[b, :n[b]].tobytes() == want, (cls, b)


def test_short_last_segments_of_one_stream():
    """Guards the path that did NOT change: lzs_compress_stream_device cuts a stream of this size into segments of 512 bytes,
    a workgroup each, and the segments kernel keeps the plain hop rule (wg_search<false>).  A last segment of 1 .. 40 bytes
    leaves most lanes of its workgroup without a position in SEARCH.  The same for the rule that hops may end a walk is the
    blocks of 1 .. 63 bytes in test_every_length_of_a_built_content_gives_the_oracles_bytes.  The built contents, so that what
    ends a walk lies in segments of its own."""
    for name in ("text", "rejectable chain, 2-gram", "seed 5, longer last", "pool border"):
        data = CONTENTS[name]()
        for n in (512 * 5 + 1, 512 * 5 + 40, 512 * 12 + 5, 512 * 40 + 63):
            x = torch.from_numpy(np.frombuffer(data[:n], dtype=np.uint8).copy()).cuda()
            buf, got = lzs.compress_stream(x)
            assert buf[:got].cpu().numpy().tobytes() == O.compress(data[:n]), (name, n)
