"""Contents BUILT for each table shape of the compress kernel (no device).

kernels/compress_wg.inc is compiled four times for the block and packed entries (lzs_kernels.hip): wgv_text, wgv_few, wgv_lit and
wgv_safe differ in their bucket counts, their multipliers, whether a 3-byte chain exists at all (LZS_WGV_NO3) and how many hops
and full steps a pass of SEARCH takes.  tests/test_gpu_search_hop_end.py builds its contents for wgv_text's tables alone; under
another shape its "collisions" share no bucket and its walks never end where the builders meant.  Here the same builders take a
Shape: grams of the SHAPE's bucket are found by brute force over the rare bytes, and what each content was built for -- which
token the parse takes at which position, what stands on the chain the shape walks there -- is recorded beside its bytes, so that
tests/test_compress_variant_programs.py can hold every content of every shape to the oracle's token list and to chain(), the
small model of a bucket's chain below.  With the default shape the contents are byte for byte those of test_gpu_search_hop_end.py.

Every builder keeps its structure inside the first 2048 + 512 positions, so that the cut lengths cut through it.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

from lzs_compression_amd import workload

BLOCK = 65536
WINDOW = 2047
CLASSIFY_POSITIONS = 2048                 # compress_aux.inc: the classifier counts the 2-grams of a block's first 2048 positions
CLASS_FEW_MAX, CLASS_MANY_MIN = 160, 1200


class Shape(NamedTuple):
    """The tables and the pass shape of one inclusion of compress_wg.inc (hash3_mul / head3 None: LZS_WGV_NO3)."""
    name: str
    hash3_mul: Optional[int]
    head3: Optional[int]
    hash2_mul: int
    head2: int
    head2_shift: int
    hops: int
    hops_last: int
    substeps: int

    @property
    def no3(self) -> bool:
        return self.head3 is None

    def bucket3(self, g: bytes) -> int:
        """wg_hash3x4 / 4: a 24-bit multiply mixes, a high multiply scales into the table."""
        t = g[0] | g[1] << 8 | g[2] << 16
        return ((((t * self.hash3_mul) & 0xFFFFFFFF) * (4 * self.head3)) >> 32) >> 2

    def bucket2(self, g: bytes) -> int:
        t = g[0] | g[1] << 8
        return (((t * self.hash2_mul) & 0xFFFFFFFF) >> self.head2_shift) & (self.head2 - 1)


def head2_shift(head2: int) -> int:
    """kWgHead2Shift: bits 15.. of the product down."""
    return {4096: 4, 2048: 5, 1024: 6, 512: 7}.get(head2, 8)


TEXT = Shape("text", 0x897397, 1152, 0x64EBAD33, 512, 7, hops=2, hops_last=3, substeps=2)
FEW = Shape("few", None, None, 0xCFC8AE9B, 1024, 6, hops=0, hops_last=0, substeps=2)
LIT = Shape("lit", None, None, 0xCFC8AE9B, 1024, 6, hops=2, hops_last=2, substeps=1)
SAFE = Shape("safe", 0x1EB419, 1792, 0xCFC8AE9B, 1024, 6, hops=2, hops_last=2, substeps=2)
SHAPES = {s.name: s for s in (TEXT, FEW, LIT, SAFE)}
DEFAULT = TEXT


class At(NamedTuple):
    """What a content was built for at position p: the token the parse takes there, and -- `which`, 3 or 2 -- what stands on the
    chain the shape walks from p: the answer `answer` positions back is its LAST candidate inside the window (`last`), and at
    least `others` candidates of other grams stand nearer than it."""
    p: int
    token: tuple
    which: Optional[int] = None
    answer: int = 0
    last: bool = False
    others: int = 0


class Built(NamedTuple):
    data: bytes
    at: tuple


_text = None


def filler(n: int, at: int = 0) -> bytearray:
    """Seeded text; its bytes are printable ASCII and the line feed, so the builders' own grams -- the other bytes below 32 and
    those from 128 on -- occur nowhere else."""
    global _text
    if _text is None:
        _text = workload.fill("text", 4).tobytes()
        assert all(c == 10 or 32 <= c < 128 for c in set(_text))
    return bytearray(_text[at:at + n])


RARE = bytes(c for c in range(1, 32) if c != 10) + bytes(range(128, 256))
G = bytes((0x81, 0x92, 0xA3))


@functools.lru_cache(maxsize=None)
def grams_in_bucket3(shape: Shape, g: bytes, count: int, third_equal: bool) -> tuple:
    """Other 3-grams of rare bytes in g's bucket whose third byte is (not) g's: the probe at offset 2 passes (fails) on them."""
    want, found = shape.bucket3(g), []
    for a in RARE:
        for b in RARE:
            for c in ((g[2],) if third_equal else RARE):
                h = bytes((a, b, c))
                if h[:2] != g[:2] and (c == g[2]) == third_equal and a != g[0] and shape.bucket3(h) == want:
                    found.append(h)
                    if len(found) == count:
                        return tuple(found)
    raise AssertionError("not enough grams in the bucket")


@functools.lru_cache(maxsize=None)
def grams_in_bucket2(shape: Shape, g: bytes, count: int) -> tuple:
    """Other 2-grams of rare bytes in the bucket of g's first two bytes; both bytes differ from g's, so the probe at offset 1
    fails on every one of them."""
    want, found = shape.bucket2(g), []
    for a in RARE:
        for b in RARE:
            h = bytes((a, b))
            if h != g[:2] and a != g[0] and b != g[1] and shape.bucket2(h) == want:
                found.append(h)
                if len(found) == count:
                    return tuple(found)
    raise AssertionError("not enough 2-grams in the bucket")


def put(buf: bytearray, at: int, s: bytes) -> None:
    buf[at:at + len(s)] = s


# ------------------------------------------------------------------------------------------------ the chain model
def chain(data: bytes, p: int, shape: Shape, which: int) -> list:
    """The positions before p, inside its window, whose `which`-byte gram falls in the bucket of p's, nearest first: what a walk
    from p on that chain visits, in order.  (The kernel leaves the interior of a run of one byte value out of its chains; the
    contents this model is asked about have no such run before p.)"""
    bucket = shape.bucket3 if which == 3 else shape.bucket2
    want = bucket(data[p:p + which])
    return [q for q in range(p - 1, max(p - WINDOW, 0) - 1, -1) if bucket(data[q:q + which]) == want]


def walked(shape: Shape) -> int:
    """The chain a position without an offset-1 seed walks first under this shape."""
    return 2 if shape.no3 else 3


# ------------------------------------------------------------------------------------------------ the contents
SAME_2GRAM_BACK = (500, 1200)          # NO3's farthest candidate: G's 2-gram with another third byte, this far before p


def farthest_candidate(shape: Shape, dist: int, long: bool) -> Built:
    """G (or 12 bytes that begin with it) at position 1 and again `dist` further on; between them, nearer on the chain the shape
    walks, grams of the same bucket.  With a 3-byte chain: some the probe rejects, some it lets through to a full step that finds
    no match.  NO3: eight 2-grams of the bucket the probe rejects -- more than the hops of a pass, so a full step lands on one --
    and G's own 2-gram twice with another third byte: a match of 2 that the far one must beat at 2047, and that is the answer at
    2048."""
    b = filler(BLOCK)
    s = G + (bytes(range(0xB0, 0xB9)) if long else b"")
    put(b, 1, s + b"\x05")
    p = 1 + dist
    put(b, p, s + b"\x06")
    if shape.no3:
        hits = grams_in_bucket2(shape, G, 8)
        for k, back in enumerate(SAME_2GRAM_BACK):
            put(b, p - back, G[:2] + bytes((0x0F + 2 * k,)))
    else:
        hits = grams_in_bucket3(shape, G, 3, True) + grams_in_bucket3(shape, G, 5, False)
    for k, h in enumerate(hits):                      # nearest first from p: a mixed order of the two kinds
        put(b, p - 40 - 37 * k, h)
    inside = dist <= WINDOW
    near = (SAME_2GRAM_BACK[0], 2) if shape.no3 else (0, 1)
    return Built(bytes(b), (At(p, (dist, len(s)) if inside else near, walked(shape), dist if inside else 0, inside, len(hits)),))


def rejectable_chain(shape: Shape, with_2gram: bool) -> Built:
    """At position p the 3-byte chain holds only grams of G's bucket whose third byte differs (a hop passes over every one of
    them, the last included); the 2-gram of G stands twice in the window, behind collisions of ITS bucket: the walk restarts
    on the 2-byte chain and the NEARER of the two is the answer.  Without the 2-gram: a literal."""
    assert not shape.no3
    b = filler(BLOCK)
    p = 1900
    put(b, p, G + b"\x07")
    for k, h in enumerate(grams_in_bucket3(shape, G, 7, False)):
        put(b, p - 30 - 41 * k, h)
    if with_2gram:
        put(b, p - 700, G[:2] + b"\x08")
        put(b, p - 1500, G[:2] + b"\x09")
    for k, h in enumerate(grams_in_bucket2(shape, G, 4)):
        put(b, p - 100 - 123 * k, h + b"\x0E")
    return Built(bytes(b), (At(p, (700, 2) if with_2gram else (0, 1), 3, 0, False, 7),
                            At(p, (700, 2) if with_2gram else (0, 1), 2, 700 if with_2gram else 0, False, 4)))


@functools.lru_cache(maxsize=None)
def lone_gram(shape: Shape, n: int) -> bytes:
    """A gram of n rare bytes (3 or 2) that meets nothing of its bucket between positions 1 and 2048 of the filler, on either
    chain: by brute force, with the chain model."""
    text = bytes(filler(2048 + 16))
    taken2 = {shape.bucket2(text[q:q + 2]) for q in range(2052)}          # (a quick sieve; the model decides below)
    taken3 = set() if shape.no3 else {shape.bucket3(text[q:q + 3]) for q in range(2052)}
    for a in RARE[40:]:
        for b in RARE[60:]:
            g = bytes((a, b, 0xA4))
            if shape.bucket2(g) in taken2 or (not shape.no3 and any(shape.bucket3(g[:2] + bytes((c,))) in taken3 for c in (5, 6, 0xA4))):
                continue
            if all(lone_chains(shape, _lone(g[:n], dist), 1 + dist) == lone_chains_wanted(shape, dist, n) for dist in (2047, 2048)):
                return g[:n]
    raise AssertionError("no lone gram")


def lone_chains(shape: Shape, data: bytes, p: int) -> tuple:
    """(the 2-byte chain, the 3-byte chain or None) of position p, by the chain model."""
    return chain(data, p, shape, 2), None if shape.no3 else chain(data, p, shape, 3)


def lone_chains_wanted(shape: Shape, dist: int, n: int) -> tuple:
    one = [1] if dist <= WINDOW else []
    return one, None if shape.no3 else (one if n == 3 else [])


def _lone(g: bytes, dist: int) -> bytes:
    b = filler(BLOCK)
    put(b, 1, g + b"\x05")
    put(b, 1 + dist, g + b"\x06")
    return bytes(b)


def lone_candidate(shape: Shape, dist: int, n: int) -> Built:
    """A gram of n bytes at position 1 and `dist` further on, and NOTHING else of its bucket between them: the first link of the
    walk from p is the window's reach itself (the refill pass's l <= reach), or one more.  n = 2 under a shape with a 3-byte
    chain: that chain is empty inside the window, and the walk begins on the 2-byte chain."""
    p = 1 + dist
    return Built(_lone(lone_gram(shape, n), dist), (At(p, (dist, n) if dist <= WINDOW else (0, 1), 2, dist if dist <= WINDOW else 0, dist <= WINDOW, 0),))


LADDER_P, LADDER_STEP = 1900, 150


def ladder(shape: Shape) -> Built:
    """Before position p eleven candidates of 2 .. 12 bytes of p's string, each a byte longer and FARTHER than the one before:
    each passes the probe and costs a full step, and the deciding one -- to the cap -- comes last.  A twelfth stands farther
    still and is as long: it must not win.  (The candidate of 2 bytes stands on the 2-byte chain alone: a shape with a 3-byte
    chain walks the other ten.)"""
    del shape                                         # (the same bytes for every shape: the grams are the ladder's own)
    b = filler(BLOCK)
    s = G + bytes(range(0xD0, 0xD9))
    for k in range(11):                               # candidate k matches 2 + k bytes
        put(b, LADDER_P - 100 - LADDER_STEP * k, s[:2 + k] + bytes((0x10 + k,)))
    put(b, LADDER_P - 100 - LADDER_STEP * 11, s + b"\x1C")
    put(b, LADDER_P, s + b"\x1B")
    return Built(bytes(b), (At(LADDER_P, (100 + LADDER_STEP * 10, 12)),))


def seeded_with_longer_match_last(shape: Shape, run: int, dist: int) -> Built:
    """x r^run T at p - 1: the run's second byte is seeded by offset 1 with run - 1 bytes (2 .. 11); the same string stands `dist`
    before -- the last candidate of the window when dist is 2047 -- and matches to the cap; nearer on the chain of r r r, runs
    that end in another byte (what the probe at offset run - 1 rejects)."""
    del shape
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
    # (x and the run's first byte are copied from `dist` before; so is everything up to the end of T)
    return Built(bytes(b), (At(p - 1, (dist, 1 + run + 12)),))


SEED_P = 2100


def seed_at_a_token_start(shape: Shape, run: int, dist: int) -> Built:
    """A B r at p - 3, a string that stands once before with another byte behind it: a token of 3 that ends on the run's first
    byte, so that the parse takes its next token at p, the run's second byte -- the position the offset-1 seed of run - 1 bytes
    belongs to (in the contents above the parse steps over it).  r^(run - 1) T stands `dist` before p and matches to the cap:
    the walk from the seed -- on the 3-byte chain, NO3 on the 2-byte chain -- has to find it.  With run - 1 >= 12 the seed is
    capped (len1 == lim), no walk starts, and the far string, as long under the cap, must not win."""
    del shape
    b = filler(BLOCK)
    r = 0x9C
    T = bytes(range(0xC0, 0xCC))
    p = SEED_P
    put(b, p - 3 - 1000, b"\x0B\x0C" + bytes([r]) + b"\x0D")
    put(b, p - 3, b"\x0B\x0C" + bytes([r]) * run + T + b"\x0E")
    put(b, p - dist - 1, b"\x0F" + bytes([r]) * (run - 1) + T + b"\x11")
    capped = run - 1 >= 12
    return Built(bytes(b), (At(p - 3, (1000, 3)), At(p, (1, run - 1) if capped else (dist, run - 1 + 12))))


BORDER_WALKERS = tuple(range(1536 + 500, 1536 + 531, 15))


def walks_over_a_pool_border(shape: Shape) -> Built:
    """Positions 500, 515 and 530 of the pool that begins at 1536 each hold a string of 12 bytes of their own, and before each
    ten candidates, every one a byte longer than the one before and FARTHER: each passes the probe and costs a full step, and
    the deciding one -- to the cap -- comes last.  Walks that the pool's SEARCH leaves unfinished and the next pool's ends.
    NO3: the same walkers, on the 2-byte chain."""
    del shape
    b = filler(BLOCK)
    for j, p in enumerate(BORDER_WALKERS):
        g = bytes((0x81 + j, 0x92, 0xA3))
        tail = bytes(range(0xD0 + 16 * j, 0xDC + 16 * j))
        for k in range(10):                           # candidate k matches 3 + k bytes of g tail
            put(b, 1500 - 140 * k - 20 * j, g + tail[:k] + bytes([0x10 + k]))
        put(b, p, g + tail[:9] + bytes([0x1B + j]))
    return Built(bytes(b), tuple(At(p, (p - (1500 - 140 * 9 - 20 * j), 12)) for j, p in enumerate(BORDER_WALKERS)))


def builders(shape: Shape) -> dict:
    """name -> a function that builds the content, for this shape.  The names test_gpu_search_hop_end.py has keep its bytes under
    the default shape."""
    c = {
        "3-gram at 2047": lambda: farthest_candidate(shape, 2047, False),
        "3-gram at 2048": lambda: farthest_candidate(shape, 2048, False),
        "12 bytes at 2047": lambda: farthest_candidate(shape, 2047, True),
        "12 bytes at 2048": lambda: farthest_candidate(shape, 2048, True),
    }
    if not shape.no3:
        c["rejectable chain, 2-gram"] = lambda: rejectable_chain(shape, True)
        c["rejectable chain, no 2-gram"] = lambda: rejectable_chain(shape, False)
    c.update({
        "lone 3-gram at 2047": lambda: lone_candidate(shape, 2047, 3),
        "lone 3-gram at 2048": lambda: lone_candidate(shape, 2048, 3),
        "lone 2-gram at 2047": lambda: lone_candidate(shape, 2047, 2),
        "lone 2-gram at 2048": lambda: lone_candidate(shape, 2048, 2),
        "ladder": lambda: ladder(shape),
        "seed 2, longer last": lambda: seeded_with_longer_match_last(shape, 3, 2047),
        "seed 5, longer last": lambda: seeded_with_longer_match_last(shape, 6, 2047),
        "seed 11, longer last": lambda: seeded_with_longer_match_last(shape, 12, 2040),
        "seed 2 at a token start": lambda: seed_at_a_token_start(shape, 3, 2047),
        "seed 5 at a token start": lambda: seed_at_a_token_start(shape, 6, 2047),
        "seed 11 at a token start": lambda: seed_at_a_token_start(shape, 12, 2040),
        "seed capped at a token start": lambda: seed_at_a_token_start(shape, 20, 2047),
        "pool border": lambda: walks_over_a_pool_border(shape),
        "text": lambda: Built(bytes(filler(BLOCK, 65536)), ()),
    })
    return c


@functools.lru_cache(maxsize=None)
def contents(shape_name: str) -> dict:
    """name -> Built, every content of the shape (built once a process)."""
    return {name: build() for name, build in builders(SHAPES[shape_name]).items()}


# ------------------------------------------------------------------------------------------------ a class change after the horizon
HORIZON = 2100                         # the bytes that steer the class: the classifier reads 2049 of them
NO_DIGRAM_TWICE = bytes(0xC0 + (k * i - 1) % 29 for k in range(1, 29) for i in range(1, 30))   # 28 rows of 29 letters


def _rng(seed: int):
    return np.random.default_rng(seed)


def _lead(kind: str) -> bytes:
    if kind == "zeros":
        return bytes(HORIZON)
    if kind == "repeat16":
        return (bytes(range(0x40, 0x50)) * (HORIZON // 16 + 1))[:HORIZON]
    if kind == "random":
        return _rng(11).integers(0, 256, HORIZON, dtype=np.uint8).tobytes()
    assert kind == "text"
    return bytes(filler(HORIZON, 3 * BLOCK))


def _follow(kind: str) -> bytes:
    if kind == "text":
        return bytes(filler(5000, 2 * BLOCK + 777))
    if kind == "random":
        return _rng(12).integers(0, 256, 5000, dtype=np.uint8).tobytes()
    if kind == "run":                                 # longer than 4080: an open match, then run mode
        return b"\x55" * 4500
    if kind == "period":
        return _rng(13).integers(0, 256, 1800, dtype=np.uint8).tobytes() * 3
    if kind == "dense":                               # matches of 2 and a little more wherever the parse stands; more than a window of it
        return (_rng(14).integers(0, 2, 2400, dtype=np.uint8) + ord("a")).astype(np.uint8).tobytes()
    assert kind == "literals"                         # (behind `dense`: nothing in the window shares a byte with it)
    return NO_DIGRAM_TWICE[:LITERALS]


LITERALS = 600                         # literals in a row: more than a pool of 512 positions, through the bit ring
FOLLOW_UPS = ("text", "random", "run", "period", "dense", "literals")
CLASS_CHANGES = {                      # name -> (the class its first 2100 bytes steer to, what they are, the first follow-up)
    "text, then random": (1, "text", "random"),
    "text, then a run": (1, "text", "run"),
    "zeros, then text": (2, "zeros", "text"),
    "16-byte repeat, then random": (2, "repeat16", "random"),
    "random, then text": (3, "random", "text"),
    "random, then a run": (3, "random", "run"),
}
CLASS_CHANGE_LENGTHS = (2048, 2049, HORIZON + 513)    # ... and the full length


@functools.lru_cache(maxsize=None)
def class_change(name: str) -> bytes:
    """The first 2100 bytes steer the classifier; behind them every other kind of content, back to back, the named one first
    and the 600 literals behind the dense 2-byte matches."""
    _, lead, first = CLASS_CHANGES[name]
    order = [first] + [k for k in FOLLOW_UPS if k != first]
    data = _lead(lead) + b"".join(_follow(k) for k in order)
    assert len(data) <= 40 * 1024
    return data


def literals_at(name: str) -> int:
    """Where the 600 literals of a class-change block begin (they are its last part)."""
    return len(class_change(name)) - LITERALS


def classify(data: bytes) -> int:
    """lzs_classify_blocks_kernel as plain code: the distinct 2-grams among the first 2048 positions in a 4096-bit hashed set;
    1 the default variant, 2 few distinct grams, 3 nearly all literals.  A block below 2049 bytes: 1."""
    if len(data) < CLASSIFY_POSITIONS + 1:
        return 1
    seen = {(((data[i] | data[i + 1] << 8) * 40503) >> 4) & 4095 for i in range(CLASSIFY_POSITIONS)}
    return 2 if len(seen) <= CLASS_FEW_MAX else (3 if len(seen) >= CLASS_MANY_MIN else 1)
