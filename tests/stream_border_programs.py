"""A token assembler for LZS streams, and the directed streams ("border programs") that hold the many-wavefront stream decoders
 to oracle.scan_segments, the plain model of a segment border.

The assembler writes the stream directly, a token at a time: no compressor decides what a literal is, and malformed streams are as
easy as valid ones.  A border program is one stream that carries one designed case at each of its borders: filler tokens bring the
cursor to the next border at the phase the case needs.  The cases are designed for segments of SEG bytes (the smallest the host
allows); at twice that every other one lies in the middle of a segment.

tests/test_stream_border_model.py proves with the model's counters that the streams reach what they are built for;
tests/test_gpu_stream_border_model.py decodes them on the device.  Helper module, not a conftest: nothing here is a test.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

SEG = 256                      # bytes: LZS_DEC_SEG=256
SEG_BITS = 8 * SEG
MIN_SEGMENTS = 70              # every program is at least this long: its second half is a piece for the incremental decoder's device route


class Assembler:
    """An MSB-first bit writer with one method a token.  ``starts``: the bit position of every step -- a token or a length
    nibble -- in the order written; ``at``: the bit cursor; ``out``: the bytes a decoder with room for all of them has produced so
    far if every token written lies on its walk."""

    def __init__(self):
        self._parts = []
        self.at = 0
        self.out = 0
        self.starts = []

    def _put(self, value, width):
        assert 0 <= value < (1 << width)
        self._parts.append(format(value, "0%db" % width))
        self.at += width

    def _step(self):
        self.starts.append(self.at)

    def lit(self, c):
        self._step()
        self._put(c & 0xFF, 9)
        self.out += 1

    def _length(self, length):
        assert 2 <= length <= 8
        if length <= 4:
            self._put(length - 2, 2)
        else:
            self._put(0xC + length - 5, 4)
        self.out += length

    def short(self, off, length):
        """1 1 ooooooo + length code (2..8; 8 leaves an extension open: nibbles() follows)."""
        assert 1 <= off <= 127
        self._step()
        self._put(0x180 | off, 9)
        self._length(length)

    def long(self, off, length):
        """1 0 ooooooooooo + length code.  Any offset from 1 on: small ones in the long form are legal."""
        assert 1 <= off <= 2047
        self._step()
        self._put(0x1000 | off, 13)
        self._length(length)

    def nibbles(self, k, closing):
        """k length nibbles of 15, then the closing one (0..14; None: the extension stays open)."""
        for _ in range(k):
            self._step()
            self._put(15, 4)
            self.out += 15
        if closing is not None:
            assert 0 <= closing <= 14
            self._step()
            self._put(closing, 4)
            self.out += closing

    def match(self, off, length, long_form=None):
        """A whole match of ``length`` >= 2 bytes with all its nibbles."""
        form = self.long if (off > 127 if long_form is None else long_form) else self.short
        form(off, min(length, 8))
        if length >= 8:
            self.nibbles((length - 8) // 15, (length - 8) % 15)

    def marker(self):
        self._step()
        self._put(0x180, 9)

    def long_zero(self):
        """1 0 00000000000: thirteen bits, no copy, not an end marker."""
        self._step()
        self._put(0x1000, 13)

    def raw(self, bits):
        """Bits as a string of 0 and 1, written as they are: no step is recorded."""
        assert set(bits) <= {"0", "1"}
        self._parts.append(bits)
        self.at += len(bits)

    def pad_to_bit(self, phase=0):
        """Zero bits up to the next position that is ``phase`` modulo 8 (what follows an end marker under the file rule)."""
        self.raw("0" * ((phase - self.at) % 8))

    def bytes(self):
        bits = "".join(self._parts)
        bits += "0" * (-len(bits) % 8)
        return int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""


@dataclass
class Stream:
    name: str
    family: str                 # "A" .. "F"
    data: bytes
    starts: tuple               # the assembler's steps (bit positions); () for streams not assembled here
    file_rule: bool = True      # decoded under the file rule too (lzs_decompress_concat)
    cut: bool = False           # the stream was cut after it was assembled: only a prefix of the steps is there
    notes: dict = field(default_factory=dict)


class Program(Assembler):
    """An assembler that knows where the borders are."""

    def __init__(self, seed, text=False, behind_marker=False):
        super().__init__()
        self.rng = np.random.default_rng(seed)
        self.text = text         # fillers are mostly short matches, so that the stream expands like text (the TWO decoder's band)
        if behind_marker:        # a short stream of its own in front: all that follows is the file rule's (and a piece that begins
            for _ in range(60):  # right behind a marker, for the incremental decoder)
                self.filler_lit()
            self.marker()
            self.pad_to_bit(0)

    def filler_lit(self):
        self.lit(int(self.rng.integers(0, 256)))

    def filler_match(self, width):
        """A match token of 11 or 13 bits whose source lies in what was produced (or in front of out[0] at the very start)."""
        off = int(self.rng.integers(1, min(max(self.out, 1), 127) + 1))
        self.short(off, int(self.rng.integers(2, 5)) if width == 11 else int(self.rng.integers(5, 8)))

    def fill_to(self, target):
        """Whole tokens up to bit ``target`` exactly: literals (9 bits) and short matches (11, 13)."""
        d = target - self.at
        assert d == 0 or d >= 9, d
        while d > 120:
            if self.text and self.rng.random() < 0.7:
                w = 11 if self.rng.random() < 0.6 else 13
                self.filler_match(w)
            else:
                w = 9
                self.filler_lit()
            d -= w
        # the rest exactly: 9 a + 11 b + 13 c
        for c in range(0, d // 13 + 1):
            for b in range(0, (d - 13 * c) // 11 + 1):
                if (d - 13 * c - 11 * b) % 9 == 0:
                    a = (d - 13 * c - 11 * b) // 9
                    kinds = [9] * a + [11] * b + [13] * c
                    self.rng.shuffle(kinds)
                    for w in kinds:
                        self.filler_lit() if w == 9 else self.filler_match(w)
                    assert self.at == target
                    return
        raise AssertionError("no filler for %d bits" % d)

    def next_border(self, lead, gap=130):
        """The first border that leaves at least ``gap`` bits for fillers in front of a case that begins ``lead`` bits before it."""
        k = (self.at + gap + lead + SEG_BITS - 1) // SEG_BITS
        return max(k, 1) * SEG_BITS

    def at_border(self, lead, gap=130):
        """Fill up to ``lead`` bits in front of the next border; returns the border's bit."""
        border = self.next_border(lead, gap)
        self.fill_to(border - lead)
        return border

    def segments(self):
        return (self.at + SEG_BITS - 1) // SEG_BITS

    def finish(self, name, family, lead, tail=40, **kw):
        """Fillers up to MIN_SEGMENTS, the end marker with ``lead`` (0..9) of its bits in front of a border, zero bits to the
        next byte, and ``tail`` more tokens: what a one-shot decoder must ignore and the file rule decodes."""
        if self.segments() < MIN_SEGMENTS:
            self.fill_to(MIN_SEGMENTS * SEG_BITS + 99)
        self.at_border(lead)
        self.marker()
        self.pad_to_bit(0)
        for _ in range(tail):
            self.filler_lit()
        if tail:
            self.marker()
        return Stream(name, family, self.bytes(), tuple(self.starts), **kw)


# ---------------------------------------------------------------------------------------------------------------- A: phase sweep
def _emit(p, kind):
    """One step of ``kind`` (a name of oracle.STEP_KINDS) at the cursor, with whatever has to stand before or behind it elsewhere."""
    rng = p.rng
    far = int(rng.integers(128, 200))
    near = int(rng.integers(1, 100))
    if kind == "lit":
        p.filler_lit()
    elif kind == "short2":
        p.short(near, int(rng.integers(2, 5)))
    elif kind == "long2":
        p.long(far, int(rng.integers(2, 5)))
    elif kind == "short4":
        p.short(near, int(rng.integers(5, 8)))
    elif kind == "long4":
        p.long(far, int(rng.integers(5, 8)))
    elif kind == "short8":                       # a length 8 with its first nibble
        p.short(near, 8)
        p.nibbles(0, int(rng.integers(0, 15)))
    elif kind == "long8":
        p.long(far, 8)
        p.nibbles(0, int(rng.integers(0, 15)))
    elif kind == "marker":
        p.marker()
        p.pad_to_bit(0)
    elif kind == "long_zero":
        p.long_zero()
    else:
        raise AssertionError(kind)


SWEEP = {"lit": 9, "short2": 11, "long2": 15, "short4": 13, "long4": 17, "short8": 17, "long8": 21, "long_zero": 13}
NIBBLE_SWEEP = {"nib15": None, "close0": 0, "close1": 1, "close14": 14}


def _sweep(seed, name, with_markers):
    p = Program(seed)
    if with_markers:                             # (first: what follows the first of them is long enough for a piece of its own)
        for b in range(10):
            p.at_border(b)
            _emit(p, "marker")
    for kind, width in SWEEP.items():
        for b in range(width + 1):
            p.at_border(b)
            _emit(p, kind)
    for kind, closing in NIBBLE_SWEEP.items():
        for b in range(5):
            # an extension of three nibbles of 15 and a closing one; the second 15 (or the closing one) begins b bits before the border
            lead_bits = 13 + 4 + (0 if closing is None else 8)
            p.at_border(b + lead_bits)
            p.short(int(p.rng.integers(1, 100)), 8)
            p.nibbles(3, 0 if closing is None else closing)
    return p.finish(name, "A", lead=1)


# ---------------------------------------------------------------------------------------------------------------- B: extensions
EXT_OFFSETS = ((1, False), (2, False), (127, False), (127, True), (128, True), (1024, True), (2047, True))


def _extensions(seed, name, shift, lead, behind_marker=False):
    """Every offset x 0..3 whole segments of 0xFF under the extension; the closing nibble at each of the sixteen bit positions round a
    border (-8 .. 7), its value 0, 1, 14 or another in turn.  The token ends on the first border or up to three bits before it: the
    bits from there to the closing nibble are all ones."""
    p = Program(seed, behind_marker=behind_marker)
    # enough in front for the farthest offset to read real bytes
    p.fill_to(p.next_border(0, gap=11 * SEG_BITS))
    def extension(off, long_form, whole, d, closing):
        head = 17 if long_form else 13
        first = p.next_border(head + 3)
        close_at = first + (whole if d >= 0 else whole + 1) * SEG_BITS + d
        end = first - (first - close_at) % 4                          # where the token ends: on the nibble grid of close_at
        p.fill_to(end - head)
        (p.long if long_form else p.short)(off, 8)
        p.nibbles((close_at - end) // 4, closing)
        assert p.at == close_at + 4

    case = shift
    for whole in (0, 1, 2, 3):
        for off, long_form in EXT_OFFSETS:
            extension(off, long_form, whole, (case * 5 + shift) % 16 - 8, (0, 1, 14, 7)[(case + shift) % 4])
            case += 1
    # a closing nibble that begins one, two, three bits before a border with ones in front of the border: the segment it begins in
    # is all 0xFF, and its last nibble is not 15 -- what the host may not skip (tests/test_gpu_parity.py:
    # test_long_match_ending_at_a_segment_border_of_all_ones has the bug this was)
    for i, (d, closing) in enumerate(((-1, 14), (-1, 8), (-2, 14), (-2, 12), (-3, 14), (-1, 11), (-2, 13))):
        off, long_form = EXT_OFFSETS[(i + shift) % len(EXT_OFFSETS)]
        extension(off, long_form, (i + shift // 8) % 2, d, closing)
    # the short token whose own bits are ones, 11 1111111 1111, across a border with b of its bits in front
    for b, whole in ((1, 1), (4, 2), (7, 0), (9, 1), (12, 3), (13, 1)):
        first = p.at_border(b)
        p.short(127, 8)
        k = (first + whole * SEG_BITS + 8 * b - p.at) // 4 + 1
        p.nibbles(k, (0, 1, 14)[b % 3])
    return p.finish(name, "B", lead=lead)


# ---------------------------------------------------------------------------------------------------------------- C: no merge, phantoms
def _low(p):
    p.lit(int(p.rng.integers(0, 0x40)))


def _phantoms(seed, name, count, ending, behind_marker=False):
    """Segments entered one bit into a literal, in runs of literals below 0x40: a walk from the border's own bit reads every one of
    them as a literal one bit late, and a literal 0xC0 as an end marker.  ``count`` of those a segment, then a match and literals of
    every value, which bring the walks together.  In every other segment they stand where the marker ends on a byte boundary -- the
    file rule's realignment then moves nothing and the walk reads the next one too -- in the others one behind the other, where it
    does.  ``ending``: the true end marker later in the last such segment, in the segment after it, or nowhere (the stream is cut)."""
    p = Program(seed, behind_marker=behind_marker)
    nseg = MIN_SEGMENTS + 2
    for s in range(nseg):
        border = p.at_border(1)
        first = len(p.starts)
        _low(p)                                                        # begins one bit before the border
        aligned = s % 2 == 0
        placed = 0
        j = 1
        while placed < count:
            t = border - 1 + 9 * j
            if (t % 8 == 6) if aligned else (j <= count):
                p.lit(0xC0)
                placed += 1
            else:
                _low(p)
            j += 1
        for _ in range(3):
            _low(p)
        assert p.at < border + SEG_BITS - 700 and len(p.starts) - first == j + 3
        p.short(int(p.rng.integers(1, 100)), 3)
        for _ in range(12):
            p.filler_lit()
    if ending == "same":
        p.marker()
    elif ending == "next":
        p.at_border(0)
        p.at_border({1: 6, 3: 7, 4: 8, 8: 9}[count])                  # (its bits in front of the border after: the streams' markers
        p.marker()                                                     # between them lie at every bit, tests/test_stream_border_model.py)
    if ending == "none":
        p.at_border(0)
        for _ in range(30):
            p.filler_lit()
        p.long(300, 8)                                                 # the input ends inside this token's offset
        data = p.bytes()[:-2]
        return Stream(name, "C", data, tuple(p.starts), cut=True)
    p.pad_to_bit(0)
    for _ in range(300):
        p.filler_lit()
    p.marker()
    return Stream(name, "C", p.bytes(), tuple(p.starts))


def _isolated_phantoms(seed=11):
    """Three phantom markers in every third segment, as in _phantoms(), between segments of ordinary tokens in which a walk from the
    border's own bit falls in step at once: what SCAN settles in three rounds -- all segments from their guessed bit; all from the
    state their predecessor left in, which is the true one but behind a segment whose first walk ended at a phantom marker, for an
    end read by a walk that was itself entered at a guess is not believed; those, from what their predecessor's second walk left."""
    p = Program(seed)                            # (a seed with which no filler token happens to read as a marker from a border's bit:
    where = []                                   # tests/test_stream_border_model.py holds the model to that)
    for s in range(22):
        border = p.at_border(1)
        where.append(border // SEG_BITS)
        _low(p)
        for j in range(1, 3 * 8 + 1):
            p.lit(0xC0) if (border - 1 + 9 * j) % 8 == 6 else _low(p)
        for _ in range(3):
            _low(p)
        p.short(int(p.rng.integers(1, 100)), 3)
        p.fill_to(border + 2 * SEG_BITS + 300)
    return p.finish("C-isolated-phantoms", "C", lead=7, notes={"phantom_segments": tuple(where)})


def _zeros():
    """64 segments of zero bytes: literals 0x00 at every one of the nine bit phases, so a walk from a border's own bit is in step
    only where the border happens to be a token start -- every ninth segment -- and otherwise never falls in step."""
    a = Assembler()
    for _ in range(64 * SEG_BITS // 9):
        a.lit(0)
    data = a.bytes()
    assert data == bytes(64 * SEG)
    return Stream("C-zeros-64-segments", "C", data, tuple(a.starts), cut=True)


def _locked(seed=0):
    """Zero literals again, but every segment is entered six bits in: 223 literals, one long match at offset 1024 (1 0 1 and zeros: a
    walk three bits late reads its ones as a literal's value) and two long offsets of zero make 2048 bits.  No walk from a border's
    own bit ever stands on a token: the truth moves one segment a round, and the rounds are as many as the segments."""
    a = Assembler()
    for _ in range(220):
        a.lit(0)
    for _ in range(5):
        a.long_zero()
    assert a.at == SEG_BITS - 3
    for _ in range(MIN_SEGMENTS):
        a.lit(0)
        a.long(1024, 2)
        a.long_zero()
        a.long_zero()
        for _ in range(222):
            a.lit(0)
    assert a.at % SEG_BITS == SEG_BITS - 3
    a.lit(0x55)
    a.marker()
    return Stream("C-locked-%d-segments" % MIN_SEGMENTS, "C", a.bytes(), tuple(a.starts))


def de_bruijn(k=64, n=2):
    """B(k, n): every n-gram over k symbols once (the standard Lyndon-word construction)."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return bytes(seq)


def _de_bruijn_stream(O):
    """Valid compressor output that is literals only: a de Bruijn sequence over the 64 symbols below 0x40 (4096 bytes, every pair of
    symbols once), five times over, through the oracle's own compressor -- a pair's earlier occurrence is always out of the window's
    reach."""
    plain = de_bruijn() * 5
    return Stream("C-de-bruijn-literals", "C", O.compress(plain), (), notes={"plain": plain})


def _low_literal_run(seed):
    """Runs of literals below 0x40 (phases 1 and 2 never leave them) and of 0x00 (no phase does), several segments long, between
    ordinary tokens."""
    p = Program(seed)
    for run in range(10):
        p.at_border(1 + run % 2)
        for i in range(int(p.rng.integers(2, 6)) * SEG_BITS // 9):
            p.lit(0) if run % 3 == 0 else _low(p)
    return p.finish("C-low-literal-runs", "C", lead=4)


# ---------------------------------------------------------------------------------------------------------------- D: origins, window
WINDOW_EDGES = (1023, 1024, 1025, 2046, 2047)


def _window(seed, name="D-window-edges", behind_marker=False):
    p = Program(seed, behind_marker=behind_marker)
    # segments 1, 2 and 8 begin with a copy from in front of out[0] (segments of literals produce ~227 bytes each)
    for k, (off, length) in ((1, (2047, 5)), (2, (1024, 8 + 15 + 3)), (8, (2047, 7))):
        p.fill_to(k * SEG_BITS)
        p.match(off, length)
        p.match(min(p.out + 3, 2047), 7)                               # three bytes of nothing, four of out[0..]
    assert p.segments() <= 10
    p.fill_to(14 * SEG_BITS)
    # every edge offset from the first byte of a segment's output, short, long and extended; then a copy that straddles the start
    for off in WINDOW_EDGES:
        for length in (2, 7, 8 + 15 + 14, 8 + 15 * 80):
            p.at_border(0)
            p.match(off, length)
            p.filler_lit()
            p.match(off, 9)
    # copies whose source begins in front of the segment's output start and ends behind it
    for own, off, length in ((2, 5, 7), (1, 130, 8 + 15 * 9), (3, 1025, 8 + 15 * 70), (2, 2047, 8 + 15 * 137), (1, 1024, 8 + 15 * 69)):
        p.at_border(0)
        for _ in range(own):
            p.filler_lit()
        p.match(off, length)
    # a segment's own output past 1024 bytes, then the edge offsets inside it: entries i and i + 1024 of the window share a byte
    for off in WINDOW_EDGES[:3]:
        for opener in (2047, 30):
            p.at_border(0)
            p.match(opener, 8 + 15 * 75)                                # 1133 bytes: with offset 2047 all from other segments (origins)
            for length in (3, 7, 8 + 15 + 2):
                p.match(off, length)
                p.filler_lit()
            p.match(2046, 8 + 15 * 3)
            p.match(off + 1 if off < 1025 else off - 2, 40)
    return p.finish(name, "D", lead=5)


def _solve_segment(total_bytes, head):
    """(literals, long zeros, nibbles of 15, closing nibble) of a segment of exactly SEG_BITS bits -- literals, one extended match with
    a ``head``-bit token, long offsets of zero -- that produces exactly ``total_bytes``."""
    for a in range(1, 228):
        length = total_bytes - a
        if length < 8:
            break
        m, c = (length - 8) // 15, (length - 8) % 15
        rest = SEG_BITS - (9 * a + head + 4 * (m + 1))
        if rest >= 0 and rest % 13 == 0:
            return a, rest // 13, m, c
    raise AssertionError("no such segment")


def _chain(seed=4):
    """A chain of copies at offset 2047 through every segment: each segment is exactly 2048 bits and produces exactly 2047 bytes -- some
    literals, then a copy at offset 2047 of the rest -- so byte x of a segment is a copy of byte x of the one before, back to
    segment 0."""
    p = Program(seed)
    a, z, m, c = _solve_segment(2047, 13)
    for _ in range(a):
        p.filler_lit()
    p.short(min(a, 100), 8)
    p.nibbles(m, c)
    for _ in range(z):
        p.long_zero()
    a, z, m, c = _solve_segment(2047, 17)
    for _ in range(MIN_SEGMENTS):
        assert p.at % SEG_BITS == 0 and p.out % 2047 == 0
        for _ in range(a):
            p.filler_lit()
        p.long(2047, 8)
        p.nibbles(m, c)
        for _ in range(z):
            p.long_zero()
    p.marker()
    return Stream("D-chain-2047-every-segment", "D", p.bytes(), tuple(p.starts))


def _chain_with_tails(seed=5):
    """The same chain with eight segments of literals only (216 bytes each) between its links: a link produces 319 bytes, so the 2047
    bytes in front of a segment -- its tail -- span nine segments, and byte x of a link is a copy of byte x of the link before."""
    p = Program(seed)
    for _ in range(9):
        for _ in range(216):
            p.filler_lit()
        for _ in range(8):
            p.long_zero()
    a, z, m, c = _solve_segment(2047 - 8 * 216, 17)
    for _ in range(16):
        assert p.at % SEG_BITS == 0
        for _ in range(a):
            p.filler_lit()
        p.long(2047, 8)
        p.nibbles(m, c)
        for _ in range(z):
            p.long_zero()
        for _ in range(8):
            for _ in range(216):
                p.filler_lit()
            for _ in range(8):
                p.long_zero()
    p.marker()
    return Stream("D-chain-tails-of-nine-segments", "D", p.bytes(), tuple(p.starts))


# ---------------------------------------------------------------------------------------------------------------- E: two tokens a trip
FIRSTS = tuple(("lit", r) for r in (1, 2, 3, 4)) + tuple(("match", n) for n in (2, 3, 4, 5, 6, 7))
SECONDS = ("sum", "sum-1", "sum+1", "16", "17", "len8", "marker", "long_zero")


def _pair(p, first, second, second_len):
    """An extension closed (the next trip begins at the next token), the trip's first token(s), the second."""
    p.short(int(p.rng.integers(20, 100)), 8)
    p.nibbles(0, int(p.rng.integers(0, 15)))
    kind, n = first
    if kind == "lit":
        for _ in range(n):
            p.filler_lit()
    else:
        p.short(int(p.rng.integers(20, 100)), n)
    _second(p, n, second, second_len)


def _second(p, n, second, second_len):
    both = n + second_len
    if second == "len8":
        p.short(both + 3, 8)
        p.nibbles(1, 2)
    elif second == "marker":
        p.marker()
        p.pad_to_bit(0)
    elif second == "long_zero":
        p.long_zero()
    else:
        off = {"sum": both, "sum-1": both - 1, "sum+1": both + 1, "16": 16, "17": 17}[second]
        (p.long if p.rng.random() < 0.3 else p.short)(off, second_len)


def _pairs(seed, name, turn, behind_marker=False):
    """Every first token with every second one, anywhere in a stream of mostly short matches; then, for every first token, the second
    on the last bit of a segment and on the first bit of the next; at the end every first token with an end marker behind it (the
    first of them ends the stream under the one-shot rule: ``turn`` says which that is)."""
    p = Program(seed, text=True, behind_marker=behind_marker)
    for _ in range(40):
        p.filler_lit()
    for first in FIRSTS:
        for second in SECONDS:
            if second == "marker":
                continue
            for _ in range(10):
                p.filler_lit() if p.rng.random() < 0.4 else p.filler_match(11)
            _pair(p, first, second, int(p.rng.integers(2, 8)))
    for first in FIRSTS:
        for lead in (1, 0):
            for second in ("sum", "sum+1", "len8"):
                width = 17 + (9 * first[1] if first[0] == "lit" else 11 if first[1] <= 4 else 13)
                p.at_border(lead + width)
                _pair(p, first, second, int(p.rng.integers(2, 8)))
    if p.segments() < MIN_SEGMENTS:
        p.fill_to(MIN_SEGMENTS * SEG_BITS + 99)
    for first in FIRSTS[turn:] + FIRSTS[:turn]:
        for _ in range(5):
            p.filler_match(11)
        _pair(p, first, "marker", 0)
    return p.finish(name, "E", lead=0)


# ---------------------------------------------------------------------------------------------------------------- F: length edges
def _length_edges(seed):
    """One program of mixed tokens, cut: at k seg - 1, k seg, k seg + 1 bytes; so that the last segment is one byte, and pad bits only;
    and inside every field of a last token of every kind, at every bit phase (a cut is a whole byte: the phases move the fields
    across it)."""
    p = Program(seed, text=True)
    p.fill_to(MIN_SEGMENTS * SEG_BITS + 77)
    base, starts = p.bytes(), tuple(p.starts)
    out = []
    for k in (MIN_SEGMENTS - 1, MIN_SEGMENTS):
        for d in (-1, 0, 1):
            out.append(Stream("F-cut-at-%d-segments%+d" % (k, d), "F", base[:k * SEG + d], starts, cut=True))
    # the end marker with eight of its bits in front of the border: the last segment is one byte -- one bit of marker, seven pad bits
    q = Program(seed + 1)
    q.fill_to(q.next_border(8, gap=(MIN_SEGMENTS - 1) * SEG_BITS) - 8)
    q.marker()
    out.append(Stream("F-last-segment-of-one-byte", "F", q.bytes(), tuple(q.starts), cut=True))
    assert len(out[-1].data) % SEG == 1
    q = Program(seed + 2)
    q.fill_to(q.next_border(9, gap=(MIN_SEGMENTS - 1) * SEG_BITS) - 9)
    q.marker()
    out.append(Stream("F-last-segment-of-pad-bits", "F", q.bytes() + b"\0", tuple(q.starts), cut=True))
    assert len(out[-1].data) % SEG == 1
    # a last token of every kind at every phase, the stream cut one and two bytes short of its end
    # (twenty segments: there are many of these)
    for kind in ("lit", "short2", "long2", "short4", "long4", "short8", "long8", "marker", "long_zero", "nibbles"):
        q = Program(seed + 3 + len(out), text=True)
        q.fill_to(19 * SEG_BITS + 55)
        head, hstarts, hat, hout = list(q._parts), list(q.starts), q.at, q.out
        for phase in range(8):
            q._parts, q.starts, q.at, q.out = list(head), list(hstarts), hat, hout
            q.fill_to(q.at + 200 + (phase - q.at - 200) % 8)
            assert q.at % 8 == phase
            mark = q.at
            if kind == "nibbles":
                q.short(9, 8)
                q.nibbles(2, 5)
            else:
                _emit(q, kind)
            data = q.bytes()
            for short_by in (1, 2):
                out.append(Stream("F-%s-phase-%d-cut-%d" % (kind, phase, short_by), "F", data[:len(data) - short_by],
                                  tuple(q.starts), cut=True, notes={"last_token": mark}))
    return out


# ---------------------------------------------------------------------------------------------------------------- all of them
@functools.lru_cache(maxsize=None)
def directed_streams():
    import oracle
    O = oracle.oracle()
    streams = [_sweep(11, "A-phase-sweep", False), _sweep(12, "A-phase-sweep-with-markers", True),
               _extensions(21, "B-extensions", 0, 2), _extensions(22, "B-extensions-shifted", 8, 3)]
    for count in (1, 3, 4, 8):
        for ending in ("same", "next", "none"):
            streams.append(_phantoms(300 + 10 * count + len(ending), "C-%d-phantoms-true-marker-%s" % (count, ending), count, ending))
    streams += [_isolated_phantoms(), _zeros(), _locked(), _de_bruijn_stream(O), _low_literal_run(35)]
    streams += [_window(41), _chain(), _chain_with_tails()]
    streams += [_pairs(51 + i, "E-pairs-%d" % i, turn) for i, turn in enumerate((0, 3, 5, 8))]
    # four of them once more behind a short stream of their own: under the one-shot rule that is all there is
    streams += [_extensions(23, "B-extensions-behind-a-marker", 4, 6, True), _phantoms(399, "C-3-phantoms-behind-a-marker", 3, "next", True),
                _window(43, "D-window-edges-behind-a-marker", True), _pairs(57, "E-pairs-behind-a-marker", 2, True)]
    streams += _length_edges(61)
    assert len({s.name for s in streams}) == len(streams)
    return tuple(streams)
