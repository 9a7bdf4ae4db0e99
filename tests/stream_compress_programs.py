"""Directed inputs ("compress programs") that hold the segmented stream compressor to oracle.compress_segments, the
plain model of what a segment border is for it.

These are DATA, not token streams: the parser decides what a token is, so it is steered.  A Builder writes a filler in which no
2-gram repeats inside the window -- the parser finds nothing there and writes literals -- and plants copies in it: the bytes at p
repeat the bytes `off` before them for `length` bytes, and a byte that breaks the match follows.  Stray tokens do appear, so
nothing here ASSUMES what the parser does with an input: what an input reaches is read off the model's counters, in
tests/test_stream_compress_model.py, and nowhere else.  tests/test_gpu_stream_compress_model.py compresses the same inputs on the
device.  The cases are laid out at borders that are multiples of 512, so that a segment size of 256 and one of 512 both see them
as borders.  Helper module, not a conftest: nothing here is a test.
"""
import functools
from dataclasses import dataclass

WINDOW = 2047
FRESH = WINDOW + 65            # a 2-gram is new if it was last seen this far back (beyond any offset a token can name)
SAME = -1                      # Builder.lit(then=SAME)


@dataclass(frozen=True)
class Input:
    name: str
    family: str                # "A" .. "G"
    data: bytes


class Builder:
    """A byte buffer with a filler that the parser can only take as literals, and copies planted in it."""

    def __init__(self, seed=1):
        self.d = bytearray()
        self.seen = {}                                   # 2-gram -> where it last starts
        self.x = (seed * 2654435761 + 12345) & 0xFFFFFFFF

    def __len__(self):
        return len(self.d)

    def _rand(self):
        self.x = (self.x * 1664525 + 1013904223) & 0xFFFFFFFF
        return self.x >> 24

    def _fresh(self, a, b, at):
        p = self.seen.get((a << 8) | b)
        return p is None or at - p > FRESH

    def _push(self, b):
        self.d.append(b)
        i = len(self.d) - 2
        if i >= 0:
            self.seen[(self.d[i] << 8) | b] = i

    def lit(self, count=1, then=None, avoid=()):
        """``count`` filler bytes.  ``then``: the byte that will follow them (a planted copy's first), so that the last filler byte
        makes no known 2-gram with it (SAME: that byte again, a run begins); ``avoid``: values the last byte must not take (a byte that would carry a match on)."""
        for i in range(count):
            last = i == count - 1
            start = self._rand()
            for j in range(256):
                b = (start + 97 * j) & 0xFF
                at = len(self.d)
                if self.d and not self._fresh(self.d[-1], b, at - 1):
                    continue
                if last and (b in avoid or (then is not None and not self._fresh(b, b if then == SAME else then, at))):
                    continue
                self._push(b)
                break
            else:
                raise AssertionError("no filler byte left")
        return self

    def to(self, pos, then=None, avoid=()):
        assert pos >= len(self.d), (pos, len(self.d))
        return self.lit(pos - len(self.d), then, avoid) if pos > len(self.d) else self

    def copy(self, off, length):
        """The next ``length`` bytes repeat what lies ``off`` before them (not broken off yet: brk())."""
        assert 1 <= off <= len(self.d) and off <= WINDOW
        for _ in range(length):
            self._push(self.d[-off])
        return self

    def brk(self, off):
        """A filler byte that ends a copy at offset ``off``."""
        return self.lit(1, avoid=(self.d[-off],))

    def plant(self, at, off, length):
        """Filler up to ``at``, then a copy of ``length`` bytes from ``off`` back, then the byte that breaks it."""
        assert at - off >= 0
        if at > len(self.d):
            self.to(at - 1)
            self.lit(1, then=self.d[at - off] if off > 1 else SAME)
        assert len(self.d) == at, (len(self.d), at)
        return self.copy(off, length).brk(off)

    def run(self, period, length):
        """``period`` filler bytes and ``length`` more that repeat them: one token of offset ``period`` (behind ``period`` literals)."""
        return self.lit(period - 1).lit(1, then=SAME if period == 1 else self.d[-(period - 1)]).copy(period, length).brk(period)

    def bytes(self):
        return bytes(self.d)


def _mixed(seed, n, alphabet=b"abcdefgh "):
    """Seeded bytes of a small alphabet: short matches everywhere, walks that merge after a few tokens."""
    x, out = (seed * 2654435761 + 1) & 0xFFFFFFFF, bytearray()
    while len(out) < n:
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out.append(alphabet[(x >> 16) % len(alphabet)])
        if (x >> 8) % 23 == 0 and len(out) > 40:        # now and then a longer repeat
            back = 1 + (x >> 3) % min(len(out) - 1, 900)
            for _ in range(3 + (x >> 20) % 40):
                out.append(out[-back])
    return bytes(out[:n])


def de_bruijn(k, n):
    """B(k, n): every n-gram over k symbols once (the standard Lyndon-word construction)."""
    a, seq = [0] * k * n, []

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


# ---------------------------------------------------------------- A: the last token of a segment against its border
def _crossings(name, cases, seed, first=2560, most=6):
    """Inputs of ``most`` cases each: case i is a copy of ``length`` bytes from ``off`` back that starts ``before`` bytes in front of
    a border; 300 literals and more lie between one case and the next border."""
    out = []
    for part in range(0, len(cases), most):
        b = Builder(seed + 1000 * part)
        for before, length, off in cases[part:part + most]:
            border = max(first, (len(b) + 300 + before + 511) // 512 * 512)
            b.plant(border - before, off, length)
        b.lit(300)
        out.append(Input(f"{name}-part-{part // most}", "A", b.bytes()))
    return out


def _family_a():
    out = []
    # length 2 .. 7, short and long offsets: ending 0 .. 6 bytes past the border, starting 1 .. 7 before it
    for form, off in (("short", 60), ("short", 127), ("long", 128), ("long", 1500), ("long", 2047)):
        cases = [(length - past, length, off) for length in range(2, 8) for past in range(0, length)]
        out.extend(_crossings(f"A-{form}-{off}-lengths-2-7", cases, seed=len(out) + 1))
    # length 8 and more by their nibbles of 15 (0, 1, 2, 3-39): ending 0 .. 16 bytes past the border and farther, closing nibbles
    # 0, 1 and 14 among them, starting 1 .. 8 bytes before the border where the length allows
    for nib, lo, hi in ((0, 8, 22), (1, 23, 37), (2, 38, 52), (5, 83, 97)):
        cases = []
        for past in range(0, 17):
            length = (lo, lo + 1, hi)[past % 3]                          # closing nibble 0, 1, 14
            length = max(length, past + 1)
            cases.append((length - past, length, 200 + 37 * past))
        cases.append((1, hi, 90))                                         # as far past the border as it reaches
        for before in range(1, 9):
            cases.append((before, lo + before, 1800 + before))
        out.extend(_crossings(f"A-length-8-nibbles-{nib}", cases, seed=10 + nib))
    # long copies over whole segments: empty runs of 1, 2, >= 3 (at 256 and at 512), 3-39 nibbles and 40 and more
    cases = [(8, 400, 1900), (4, 600, 1900), (8, 530, 2000),            # 3-39 nibbles: one and two empty segments of 256, one of 512
             (250, 608, 1700), (8, 700, 1700), (8, 1040, 1800), (8, 1100, 1900), (8, 1600, 2000), (3, 2100, 2047), (500, 1200, 1300)]
    out.extend(_crossings("A-copies-over-whole-segments", cases, seed=20))
    cases = [(1, 8 + 15 * 40 + c, 1000 + c) for c in (0, 1, 14)]       # 40 nibbles, each closing nibble
    out.extend(_crossings("A-forty-nibbles-closing-0-1-14", cases, seed=21))
    # an entry at the last byte of its segment: a copy from in front of a border to one byte short of the next (256, and 512)
    cases = [(3, 3 + 255, 1500), (5, 5 + 511, 1600), (2, 2 + 255, 1)]
    out.extend(_crossings("A-entry-at-the-last-byte", cases, seed=22))
    # a last segment shorter than the copy that crosses into it: run over, the input ends with the copy (at 512 the longest of them
    # runs over a whole segment and six bytes, at 256 over two and six)
    for name, off, length in (("short", 60, 4), ("long", 600, 5), ("nibbles-0", 700, 12), ("nibbles-1", 800, 30), ("nibbles-2", 900, 45),
                              ("nibbles-3-39", 1900, 520)):
        b = Builder(30 + length)
        b.to(2560 - 3).lit(1, then=b.d[2560 - 2 - off]).copy(off, length)
        out.append(Input(f"A-tail-run-over-{name}", "A", b.bytes()))
    # entries at every c0 & 63: a copy that ends 0 .. 63 bytes past its border
    for half in (0, 1):
        cases = [(2, 2 + past, 300 + 5 * past) for past in range(32 * half, 32 * half + 32)]
        out.extend(_crossings(f"A-entries-at-{32 * half}-to-{32 * half + 31}", cases, seed=23 + half))
    return out


# ---------------------------------------------------------------- B: the first token of a segment and the window
def _family_b():
    out = []
    # borders whose warm-up begins at 0 (2048), the first beyond (2304 at 256, 2560 at 512) and far ones; the first token of the
    # segment is the planted copy: the filler before it ends on the border.
    for off in (2047, 2046, 2040, 1):
        for shift in (0, 1, 63):                                         # the entry's c0 & 63: the previous token ends `shift` past the border
            b = Builder(100 + off + shift)
            for border in (2048, 2304, 2560, 4096, 6144, 7424):
                at = border + shift
                length = (5, 2, 3, 9, 300, 30)[(border // 256) % 6] if off != 1 else (5, 9, 40)[(border // 256) % 3]
                if shift:
                    # the token before: a copy from two bytes in front of the border to `at`, from x back -- an x at which the
                    # planted copy's first byte is not the byte that would carry this one on (val: the bytes once it is written)
                    b.to(border - 3)
                    val = lambda i, x: b.d[i] if i < border - 2 else b.d[i - x]
                    x = next(x for x in range(700, 900) if val(at - off, x) != b.d[at - x])
                    b.lit(1, then=b.d[border - 2 - x], avoid=(b.d[border - 3 - x],)).copy(x, 2 + shift)
                else:
                    b.to(at - 1).lit(1, then=b.d[at - off] if off != 1 else SAME)
                assert len(b) == at
                b.copy(off, length).brk(off)
            b.lit(200)
            out.append(Input(f"B-first-token-offset-{off}-entry-{shift}", "B", b.bytes()))
    # a source reached only through a 2-byte gram and one only through a 3-byte gram, at the window's far edge, warm-up not at 0
    b = Builder(190)
    for border, length in ((2304, 2), (2560, 3), (4608, 2), (5120, 3), (6656, 2), (7168, 3)):
        b.plant(border, 2047, length)
    b.lit(150)
    out.append(Input("B-far-edge-grams-of-2-and-3", "B", b.bytes()))
    return out


# ---------------------------------------------------------------- C: rounds
def _family_c():
    out = [Input("C-every-border-a-token-start", "C", Builder(200).lit(256 * 13 + 17).bytes())]
    for seed in (1, 2, 3):
        out.append(Input(f"C-mixed-{seed}", "C", _mixed(seed, 7000 + 300 * seed)))
    # B(16, 3) twice: in its second half every token is a match of two, a walk entered one byte off stays one byte off
    out.append(Input("C-walks-that-never-merge", "C", de_bruijn(16, 3) * 2))
    out.append(Input("C-walks-that-never-merge-longer", "C", b"\xff" + de_bruijn(16, 3) * 4))
    for name, period in (("one-byte", 1), ("period-2", 2), ("period-300", 300)):
        b = Builder(210 + period)
        b.lit(700).run(period, 12 * 512 + 77).lit(600)
        out.append(Input(f"C-long-match-{name}", "C", b.bytes()))
    return out


# ---------------------------------------------------------------- D: stitch
def _family_d():
    out = []
    for seed in (11, 12, 13, 14):
        out.append(Input(f"D-mixed-{seed}", "D", _mixed(seed, 9000, alphabet=b"abcdefghijklmnop")))
    # the end marker at every bit of a word: literals only, 9 bits a byte
    for i in range(32):
        out.append(Input(f"D-marker-at-total-{(9 * (520 + i)) % 32:02d}", "D", Builder(300 + i).lit(520 + i).bytes()))
    # three segments in one word: a copy that runs over a whole segment but for its last byte, which is a literal of nine bits --
    # at several phases (literals before it move the bits by nine, a match of two by eleven)
    for seg in (256, 512):
        b = Builder(340 + seg)
        border = 4096
        for i in range(12):
            if i % 3:
                b.plant(border - 40 - i, 50, 2)
            b.plant(border - 3 - i % 4, 1900, 3 + i % 4 + seg - 1)
            border = (len(b) + 400 + 511) // 512 * 512
        b.lit(100)
        out.append(Input(f"D-one-literal-segments-of-{seg}", "D", b.bytes()))
    # an empty segment between two that share a word, the marker behind an empty last segment: a copy to the very end
    for tail in (1, 300, 600, 1100):
        b = Builder(350 + tail)
        b.lit(1500)
        for j in range(1 + tail % 3):                                    # (matches of two: eleven bits where literals have eighteen)
            b.plant(1600 + 40 * j, 50, 2)
        b.plant(3072 - 5, 1400, 5 + 700)
        b.to(4096 - 9).copy(900, 9 + tail)
        out.append(Input(f"D-marker-behind-{tail}-bytes-of-a-copy", "D", b.bytes()))
    return out


# ---------------------------------------------------------------- E: oversized segments
def _oversized_segment(b, seg, delta, closing=9, extra_nibbles=0, to_the_end=False):
    """From a border on: a segment of literals, ``delta % 4`` matches of two and, from its last byte on, one run at offset 1 whose
    nibbles bring the segment's bits to its slot's + ``delta``.  bits = 9 a + 11 m + 13 + 4 q with a + 2 m = seg - 1."""
    slot = 8 * ((seg + (seg + 7) // 8 + 3 + 15) & ~15)
    m = delta % 4
    a = seg - 1 - 2 * m
    q, rest = divmod(slot + delta - (9 * a + 11 * m + 13), 4)
    assert rest == 0 and q >= 1
    q += extra_nibbles
    start = len(b)
    assert start % seg == 0
    for i in range(m):
        b.plant(start + 20 + 30 * i, 15, 2)
    b.to(start + seg - 2).lit(1, then=SAME)
    length = 8 + 15 * (q - 1) + closing                                  # from the segment's last byte on
    b.copy(1, length)
    return b if to_the_end else b.brk(1)


def _prefix_at_phase(b, lo, hi):
    """Filler with m matches of two in it, one run and filler again, ending on a border of 512 with the bits so far in [lo, hi]
    mod 2048 (9 bits a literal, 11 a match of two, a run of r bytes at offset 1 in 13 + 4 * ((r - 8) // 15 + 1))."""
    for j in range(2, 12):
        for m in range(0, 20):
            for r in range(8, 250):
                bits = 9 * (512 * j - r - 2 * m) + 11 * m + 13 + 4 * ((r - 8) // 15 + 1)
                if lo <= bits % 2048 <= hi:
                    for i in range(m):
                        b.plant(100 + 30 * i, 15, 2)
                    b.to(719).lit(1, then=SAME).copy(1, r).brk(1)
                    return b.to(512 * j)
    raise AssertionError((lo, hi))


def _family_e():
    out = []
    for delta in range(-8, 9):
        b = Builder(400 + delta)
        b.lit(2048)
        _oversized_segment(b, 256, delta, closing=(0, 1, 14, 9)[delta % 4]).lit(200)
        out.append(Input(f"E-256-slot{delta:+d}", "E", b.bytes()))
    for delta in (-1, 0, 1, 5):
        b = Builder(430 + delta)
        b.lit(2048)
        _oversized_segment(b, 512, delta).lit(200)
        out.append(Input(f"E-512-slot{delta:+d}", "E", b.bytes()))
    # far past the slot: all of it comes from the second pass
    b = Builder(440)
    b.lit(1024)
    _oversized_segment(b, 256, 3, extra_nibbles=1300).lit(100)
    out.append(Input("E-256-large", "E", b.bytes()))
    b = Builder(441)
    b.lit(1024)
    _oversized_segment(b, 512, 2, extra_nibbles=1200).lit(100)
    out.append(Input("E-512-large", "E", b.bytes()))
    # the oversized segment's first bit at bit 0, 1 .. 31 and >= 2017 of its 256-byte granule
    for name, lo, hi in (("0", 0, 0), ("1-31", 1, 31), ("5", 5, 5), ("31", 31, 31), ("2017-2047", 2017, 2047), ("2047", 2047, 2047)):
        for seg in (256, 512):
            b = _prefix_at_phase(Builder(450 + lo + seg), lo, hi)
            _oversized_segment(b, seg, 6, extra_nibbles=40).lit(300)
            out.append(Input(f"E-{seg}-first-bit-at-{name}", "E", b.bytes()))
    # segment 0 oversized; two in one stream; one followed by empty segments and then a one-token segment
    for seg in (256, 512):
        b = Builder(470 + seg)
        _oversized_segment(b, seg, 4, extra_nibbles=3).lit(150)
        out.append(Input(f"E-{seg}-segment-0", "E", b.bytes()))
        b = Builder(472 + seg)
        b.lit(1024)
        _oversized_segment(b, seg, 1, extra_nibbles=2)
        b.to((len(b) + 600) // 512 * 512 + 512)
        _oversized_segment(b, seg, 7, extra_nibbles=70).lit(100)
        out.append(Input(f"E-{seg}-two-oversized", "E", b.bytes()))
        b = Builder(476 + seg)
        b.lit(1024)
        _oversized_segment(b, seg, 3, extra_nibbles=50, to_the_end=True)
        out.append(Input(f"E-{seg}-oversized-to-the-end", "E", b.bytes()))
        b = Builder(474 + seg)
        b.lit(1536)
        b.to(1536 + seg - 2).lit(1, then=SAME).copy(1, 3 * seg).brk(1).lit(2 * seg)        # to one byte short of a border: that byte's segment has one token
        out.append(Input(f"E-{seg}-then-empty-then-one-token", "E", b.bytes()))
    return out


# ---------------------------------------------------------------- F: lengths
def _family_f():
    out = []
    for rest in (1, 63, 64, 255, 0):
        for kind in ("literals", "mixed"):
            n = 2048 + rest
            data = Builder(500 + rest).lit(n).bytes() if kind == "literals" else _mixed(500 + rest, n)
            out.append(Input(f"F-{kind}-length-{n}", "F", data))
    for n in (6144, 6145):                                               # the route's own threshold (no LZS_FORCE_STREAM needed)
        out.append(Input(f"F-threshold-{n}", "F", _mixed(n, n)))
    for closing in (0, 14):
        for lead in (1000, 1024 - 8 - closing - 3):                      # the match crosses the last border, or not
            b = Builder(520 + closing + lead)
            b.lit(lead).copy(700, 8 + 15 + closing)
            out.append(Input(f"F-match-reaches-the-end-closing-{closing}-from-{lead}", "F", b.bytes()))
    b = Builder(530)
    b.lit(1019).copy(600, 30).brk(600)
    out.append(Input("F-match-one-byte-short-of-the-end", "F", b.bytes()))
    b = Builder(531)
    b.lit(1024 - 10).copy(300, 10).brk(300)
    out.append(Input("F-last-segment-of-one-byte", "F", b.bytes()))
    return out


# ---------------------------------------------------------------- G: pieces of the incremental interface
def _family_g():
    out = []
    # short pieces (the low-memory block: every call with 16 bytes and more to decide reaches the device)
    b = Builder(600)
    b.lit(600).run(1, 700).lit(200).run(300, 900).lit(100)
    for i in range(12):
        b.plant(len(b) + 20 + i, 40 + 100 * i, 2 + i)
    for i in range(15):
        b.plant(len(b) + 70, 500 + 90 * i, 16 + i)
    b.lit(300)
    out.append(Input("G-short-pieces", "G", b.bytes()))
    # long pieces (the full block collects 10 KiB before it asks the device): one match open across three of them
    b = Builder(601)
    b.lit(3000).run(300, 36000).lit(3000)
    for i in range(15):
        b.plant(len(b) + 70, 100 + 120 * i, 16 + i)
    b.lit(11000)
    out.append(Input("G-long-pieces", "G", b.bytes()))
    return out


def piece_cuts(tokens, n, least):
    """Where to cut an input of ``n`` bytes into pieces of ``least`` bytes and more, from the model's token list [(position,
    offset, bytes covered, bit position)]: {label: [cut, ...]} -- every list is one way to feed the input.

    A piece that is not the last decides the tokens that start before its end - 15 (the look-ahead rule) and the full nibbles of
    15 of a match that reaches its end; so a cut x falls into the match that starts at s if s < x - 15 and x < its end, its
    nibbles stand at (x - s - 8) % 15, and the next piece begins at the bit of the first token not decided yet; the bytes from
    there to the cut wait for their look-ahead."""
    cuts = {}
    starts = [int(t[0]) for t in tokens]
    long_matches = [(int(t[0]), int(t[0]) + int(t[2])) for t in tokens if int(t[2]) >= 3 * least + 64]
    assert long_matches
    s, e = long_matches[0]
    first = max(s + 40, least)
    for r in range(15):                                                  # inside a long match at every residue of (cut - start - 8) % 15
        x = first + (r - (first - s - 8)) % 15
        assert s + 23 < x < e - least
        cuts[f"residue-{r:02d}"] = [x, x + least + r]                    # (and the piece behind is nothing but nibbles)
    cuts["open-across-three"] = [first, first + least, first + 2 * least + 7]
    assert cuts["open-across-three"][-1] < e
    by_bit0 = {}
    for i, t in enumerate(tokens):                                       # the next piece begins at this token's bit
        pos = int(t[0])
        if pos >= least + 16 and n - pos > least and int(t[2]) < 8:
            by_bit0.setdefault(int(t[3]) % 8, pos)
    for bit0, pos in by_bit0.items():
        # a cut 15 bytes behind a token start: that token is the first the piece does not decide
        cuts[f"bit0-{bit0}"] = [pos + 15]
    # 1 .. 15 bytes past a token start that is the end of a decided match: that many bytes wait for their look-ahead
    ends = [int(t[0]) + int(t[2]) for t in tokens if 16 <= int(t[2]) <= 40 and int(t[0]) >= least and n - int(t[0]) > least + 64]
    assert len(ends) >= 15
    for j in range(1, 16):
        cuts[f"past-a-token-start-{j:02d}"] = [ends[j - 1] + j]
    return cuts


@functools.lru_cache(maxsize=None)
def directed_inputs():
    inputs = _family_a() + _family_b() + _family_c() + _family_d() + _family_e() + _family_f() + _family_g()
    names = [i.name for i in inputs]
    assert len(set(names)) == len(names)
    assert all(1 <= len(i.data) <= 65536 for i in inputs)
    return tuple(inputs)
