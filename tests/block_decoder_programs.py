"""Directed streams for the eight-streams-per-wavefront decoder (lzs_decompress_blocks_grp, csrc/kernels/decompress_blocks.inc,
DESIGN.md 3.3), and the composer that puts any of them into any of the decoder's three forms.

The decoder is compiled as TWO (a second token in the same trip), WIDE (a 96-bit buffer fed two words a trip) and plain, and a
wavefront picks its form from the compressed bytes of its eight streams against their room -- something the caller controls.  So the
streams here are built token by token (the Assembler of tests/stream_border_programs.py), each for the cases its family names, and
a wavefront is composed around the stream under test: rows that are empty lower the ratio, rows that begin with an end marker and
are never read past it raise it.  form_of() is the kernels' two inequalities; every composed wavefront is checked against it.

tests/test_block_decoder_programs.py proves from the oracle's traces that the families reach what they claim and that the
composer yields every form; tests/test_gpu_block_decoder_forms.py decodes everything on the device through every entry that
instantiates the template.  Helper module, not a conftest: nothing here is a test.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

import oracle
from stream_border_programs import FIRSTS, SECONDS, Assembler, Program, _emit, _pair

O = oracle.oracle()
BIG = 1 << 22
SEG = 1 << 20                                   # one segment: the model's true walk is all that is asked of it here
K = {name: i for i, name in enumerate(oracle.STEP_KINDS)}
CLOSING = frozenset(K[k] for k in ("close0", "close1", "close14", "close_other"))
NIBBLES = CLOSING | {K["nib15"], K["first_nibble"]}
SHORT_MATCHES = frozenset(K[k] for k in ("short2", "long2", "short4", "long4"))
COPY_TOKENS = SHORT_MATCHES | {K["short8"], K["long8"]}
FORMS = ("plain", "two", "wide")
# the kernel's constants (tests/test_block_decoder_programs.py reads them back from the source)
LANES, DRAIN, RING, TWO_MAX, CHUNK = 8, 128, 2304, 16, 128
FORM_FACTORS = (4, 10, 9)


def form_of(total, full):
    """The form a wavefront takes: ``total`` compressed bytes of its streams against ``full`` bytes of room."""
    a, b, c = FORM_FACTORS
    if a * total > full and b * total < c * full:
        return "two"
    if b * total >= c * full:
        return "wide"
    return "plain"


@dataclass
class Stream:
    name: str
    family: str                 # "A" .. "I"
    data: bytes
    cases: tuple                # what the stream was built for, in order
    uncut: bytes = None         # family F: the stream before it was cut
    notes: dict = field(default_factory=dict)


@functools.lru_cache(maxsize=None)
def steps_of(data, cap=BIG, file_rule=False):
    """(bytes produced, the true walk's steps [(bit, kind, offset, bytes, output position)]) from the model."""
    total, _, steps = O.scan_segments(data, SEG, cap, file_rule=file_rule, trace=True)
    return total, steps


# ---------------------------------------------------------------------------------------------------------------- builders
def _off(p, hi=2047, lo=1):
    return int(p.rng.integers(lo, max(min(p.out, hi), lo) + 1))


def _warm(p, nbytes):
    """At least ``nbytes`` of output that no two offsets read alike: a few literals, a copy from anywhere, again."""
    while p.out < nbytes:
        for _ in range(int(p.rng.integers(1, 4))):
            p.filler_lit()
        p.match(_off(p), int(p.rng.integers(3, 30)))


def _fill_out_to(p, target):
    """Exactly ``target`` bytes of output."""
    assert p.out <= target, (p.out, target)
    while target - p.out > 40:
        for _ in range(int(p.rng.integers(1, 4))):
            p.filler_lit()
        p.match(_off(p), int(p.rng.integers(3, 30)))
    while p.out < target:
        p.filler_lit()


def _closing(p):
    p.short(_off(p, 127), 8)
    p.nibbles(0, int(p.rng.integers(0, 15)))


A_FOLLOWERS = ("short", "long", "long_zero", "marker", "end")


def _family_a():
    """Runs of 1 .. 16 literals behind a closing nibble, beginning at each bit phase, followed by a short match, a long match, a
    long offset 0 and -- last in the stream -- an end marker or the end of the input."""
    out = []
    for r in range(1, 17):
        for phase in range(8):
            for last in ("marker", "end"):
                p = Program([1, r, phase, len(last)])
                for _ in range(5):
                    p.filler_lit()
                cases = []
                for follower in ("short", "long", "long_zero", last):
                    for _ in range((phase - p.at - 17) % 8):            # (a literal moves the phase by one)
                        p.filler_lit()
                    _closing(p)
                    assert p.at % 8 == phase
                    for _ in range(r):
                        p.filler_lit()
                    if follower == "short":
                        p.short(_off(p, 127), int(p.rng.integers(2, 5)))
                    elif follower == "long":
                        p.long(_off(p), int(p.rng.integers(5, 8)))
                    elif follower == "long_zero":
                        p.long_zero()
                    elif follower == "marker":
                        p.marker()
                    cases.append("run of %d at phase %d, then %s" % (r, phase, follower))
                out.append(Stream("A-run%02d-phase%d-%s" % (r, phase, last), "A", p.bytes(), tuple(cases)))
    return out


B_OFFSETS = tuple((o, False) for o in range(1, 18)) + ((127, False), (127, True), (128, True), (1023, True), (1024, True),
                                                       (2046, True), (2047, True))
B_LENGTHS = tuple(range(2, 24)) + (38,)         # 2 .. 8; 9 .. 23: the closing nibbles 1 .. 15 behind the first; 8, 23, 38 close on 0


def _family_b():
    """Copies: every offset form with every length, a literal between them."""
    out = []
    for off, long_form in B_OFFSETS:
        p = Program([2, off, int(long_form)])
        _warm(p, off + 40)
        for length in B_LENGTHS:
            p.filler_lit()
            p.match(off, length, long_form)
        p.marker()
        out.append(Stream("B-offset%d-%s" % (off, "long" if long_form else "short"), "B", p.bytes(),
                          tuple("offset %d length %d" % (off, n) for n in B_LENGTHS)))
    return out


def c_copies(q):
    return ((q + 1, 30), (q + 3, 6), (q + 9, 23), (q + 16, 40), (2047, 9))


def _family_c():
    """The stream's first copy at output positions 0 .. 16, its source wholly or partly in front of out[0]."""
    out = []
    for q in range(17):
        for off, length in c_copies(q):
            p = Program([3, q, off])
            for _ in range(q):
                p.filler_lit()
            p.match(off, length)
            for _ in range(3):
                p.filler_lit()
            p.match(min(p.out + 2, 2047), 5)
            p.marker()
            out.append(Stream("C-at%02d-offset%d-length%d" % (q, off, length), "C", p.bytes(),
                              ("first copy at %d, offset %d, length %d" % (q, off, length),)))
    return out


D_POINTS = (DRAIN, 2 * DRAIN, RING, RING + DRAIN, 2 * RING)
D_KINDS = ("lits7", "nib15-offset1", "copy2047", "copy2047-extended", "pair")
PAIR_SECONDS = tuple(s for s in SECONDS if s != "marker")


def _family_d():
    """Filler up to P - d bytes of output, for every drain and ring position P in turn, and there one token kind a stream."""
    out = []
    for d in range(16):
        for ki, kind in enumerate(D_KINDS):
            p = Program([4, d, ki])
            cases = []
            for i, point in enumerate(D_POINTS):
                at = point - d
                if kind == "lits7":
                    _fill_out_to(p, at - 8)
                    _closing_exact(p)
                    for _ in range(7):
                        p.filler_lit()
                    p.short(_off(p, 127), 3)
                elif kind == "nib15-offset1":
                    _fill_out_to(p, at - 8)
                    p.short(1, 8)
                    p.nibbles(1, 3)
                elif kind == "copy2047":
                    _fill_out_to(p, at)
                    p.match(2047, 7)
                elif kind == "copy2047-extended":
                    _fill_out_to(p, at)
                    p.match(2047, 8 + 15 * 6)
                else:
                    _fill_out_to(p, at)
                    _pair(p, FIRSTS[(d + 3 * i) % len(FIRSTS)], PAIR_SECONDS[(d + i) % len(PAIR_SECONDS)], int(p.rng.integers(2, 8)))
                cases.append("%s at %d - %d" % (kind, point, d))
            _fill_out_to(p, max(p.out, 2 * RING + 60))
            for _ in range(3):
                p.filler_lit()
            p.marker()
            out.append(Stream("D-%s-d%02d" % (kind, d), "D", p.bytes(), tuple(cases),
                              notes={"kind": kind, "d": d, "pair_points": tuple(pt - d for pt in D_POINTS) if kind == "pair" else ()}))
    return out


def _closing_exact(p):
    """A copy of exactly eight bytes that ends on a closing nibble 0."""
    p.short(_off(p, 127), 8)
    p.nibbles(0, 0)


def _family_e():
    """Every first token with every second one (the builder of tests/stream_border_programs.py), and for every first token a
    second whose last field the end of the input cuts off."""
    out = []
    for i, first in enumerate(FIRSTS):
        p = Program([5, i], text=True)
        _warm(p, 120)
        cases = []
        for second in PAIR_SECONDS:
            for _ in range(4):
                p.filler_lit() if p.rng.random() < 0.4 else p.filler_match(11)
            _pair(p, first, second, int(p.rng.integers(2, 8)))
            cases.append("%s %d, then %s" % (first[0], first[1], second))
        for _ in range(3):
            p.filler_match(11)
        _pair(p, first, "marker", 0)
        cases.append("%s %d, then marker" % first)
        out.append(Stream("E-%s%d" % first, "E", p.bytes(), tuple(cases)))
        p = Program([6, i], text=True)
        _warm(p, 120)
        n2 = int(p.rng.integers(2, 8))
        _pair(p, first, "sum", n2)
        data = p.bytes()
        out.append(Stream("E-%s%d-second-cut" % first, "E", data[:-1], ("%s %d, then a second token cut by the end" % first,),
                          uncut=data, notes={"second_len": n2}))
    return out


F_KINDS = ("lit", "short2", "long2", "short4", "long4", "short8", "long8", "marker", "long_zero", "nibbles")


def _family_f():
    """A last token of every kind at every bit phase, the stream cut one and two bytes short."""
    out = []
    for ki, kind in enumerate(F_KINDS):
        for phase in range(8):
            p = Program([7, ki, phase], text=True)
            _warm(p, 210)
            for _ in range((phase - p.at) % 8):
                p.filler_lit()
            assert p.at % 8 == phase
            mark = p.at
            if kind == "nibbles":
                p.short(9, 8)
                p.nibbles(2, 5)
            else:
                _emit(p, kind)
            data = p.bytes()
            for short_by in (1, 2):
                out.append(Stream("F-%s-phase%d-cut%d" % (kind, phase, short_by), "F", data[:len(data) - short_by],
                                  ("last token %s at phase %d, cut %d short" % (kind, phase, short_by),), uncut=data,
                                  notes={"last_token": mark, "kind": kind, "phase": phase, "short_by": short_by}))
    return out


G_LENGTHS = tuple(range(120, 141)) + tuple(range(250, 263))
G_COPY = 8 + 15 * 20


def _family_g():
    """All-literal streams of each compressed length round the 128-byte chunk border and the next one, each ending in a copy of
    8 + 15 * 20 bytes and the end marker."""
    out = []
    for length in G_LENGTHS:
        built = None
        for long_form in (False, True):
            fixed = (17 if long_form else 13) + 4 * 21 + 9
            k = (8 * length - fixed) // 9
            if 9 * k + fixed > 8 * length - 8:
                p = Program([8, length])
                for _ in range(k):
                    p.filler_lit()
                p.match(_off(p, 127), G_COPY, long_form)
                p.marker()
                built = p.bytes()
                break
        assert built is not None and len(built) == length, length
        out.append(Stream("G-%d-bytes" % length, "G", built, ("%d compressed bytes, then a copy of %d" % (length, G_COPY),)))
    return out


H_COPY = 4700


def _family_h():
    """Long extensions: one copy of about 4700 bytes, and the same in two halves with literals between."""
    out = []
    for off in (1, 3, 2047):
        p = Program([9, off])
        for _ in range(5):
            p.filler_lit()
        p.match(off, H_COPY)
        p.marker()
        out.append(Stream("H-offset%d-one-copy" % off, "H", p.bytes(), ("a copy of %d at offset %d" % (H_COPY, off),)))
        p = Program([10, off])
        for _ in range(5):
            p.filler_lit()
        p.match(off, H_COPY // 2)
        for _ in range(3):
            p.filler_lit()
        p.match(off, H_COPY // 2)
        for _ in range(2):
            p.filler_lit()
        p.marker()
        out.append(Stream("H-offset%d-two-copies" % off, "H", p.bytes(), ("two copies of %d at offset %d, literals between" % (H_COPY // 2, off),)))
    return out


I_PROGRAMS = (("literals", 4), ("text", 5), ("runs", 6))


def _family_i():
    """The file rule: programs of 4 .. 6 streams back to back, each ending in a first token of one FIRSTS kind, the end marker and
    its pad bits; later streams copy from earlier ones."""
    out = []
    count = 0
    for pi, (kind, nstreams) in enumerate(I_PROGRAMS):
        p = Program([11, pi], text=kind == "text")
        cases = []
        for si in range(nstreams):
            if kind == "literals":
                for _ in range(120 if si else 520):           # (the first stream is more than half of all: a capacity in it can be n / 2)
                    p.filler_lit()
                if si:
                    p.match(_off(p, lo=130), 5)                          # from an earlier stream
            elif kind == "text":
                for _ in range(12):
                    p.filler_lit()
                for _ in range(70 if si else 160):
                    p.filler_lit() if p.rng.random() < 0.62 else p.filler_match(11 if p.rng.random() < 0.6 else 13)
                if si:
                    p.match(_off(p, lo=150), 6)
            else:
                for _ in range(6):
                    p.filler_lit()
                p.match(_off(p, 9) if si else 3, 330)
                if si:
                    p.match(_off(p, lo=340), 150)
            first = FIRSTS[count % len(FIRSTS)]
            pad = count % 8
            width = 17 + (9 * first[1] if first[0] == "lit" else 11 if first[1] <= 4 else 13) + 9
            for _ in range((-pad - p.at - width) % 8):
                p.filler_lit()
            _pair(p, first, "marker", 0)
            assert p.at % 8 == 0
            cases.append("stream %d ends in %s %d, the marker and %d pad bits" % (si, first[0], first[1], pad))
            count += 1
        out.append(Stream("I-%s" % kind, "I", p.bytes(), tuple(cases)))
    return out


@functools.lru_cache(maxsize=None)
def streams():
    all_streams = (_family_a() + _family_b() + _family_c() + _family_d() + _family_e() + _family_f() + _family_g() + _family_h()
                   + _family_i())
    assert len({s.name for s in all_streams}) == len(all_streams)
    return tuple(all_streams)


FAMILIES = "ABCDEFGHI"


def by_family(*families):
    return [s for s in streams() if s.family in families]


@functools.lru_cache(maxsize=None)
def by_name(name):
    return next(s for s in streams() if s.name == name)


def total_of(s):
    return steps_of(s.data)[0]


# ---------------------------------------------------------------------------------------------------------------- pairs, cuts
def pairs_in(steps):
    """[(first, second, index of the second's step)] of every two steps that a decoder taking two tokens a trip could take
    together: the first is a run of 1 .. 4 literals behind something that is no literal, or a match of 2 .. 7, behind a closing
    nibble (tests/test_stream_border_model.py: _pairs_seen, which this is)."""
    found = []
    kinds, offs, lens = steps[:, 1], steps[:, 2], steps[:, 3]
    i, n = 1, len(steps)
    while i < n - 1:
        if kinds[i - 1] not in CLOSING:
            i += 1
            continue
        j, first = i, None
        if kinds[i] == K["lit"]:
            while j < n and kinds[j] == K["lit"]:
                j += 1
            if j - i <= 4:
                first = ("lit", j - i)
        elif kinds[i] in SHORT_MATCHES:
            j, first = i + 1, ("match", int(lens[i]))
        if first and j < n:
            k, both = int(kinds[j]), first[1] + int(lens[j])
            if k in SHORT_MATCHES:
                for name, off in (("sum", both), ("sum-1", both - 1), ("sum+1", both + 1), ("16", 16), ("17", 17)):
                    if offs[j] == off:
                        found.append((first, name, j))
            elif k in (K["short8"], K["long8"]):
                found.append((first, "len8", j))
            elif k == K["marker"]:
                found.append((first, "marker", j))
            elif k == K["long_zero"]:
                found.append((first, "long_zero", j))
        i = max(j, i + 1)
    return found


CUT_PLACES = ("inside a literal run", "inside a first copy", "inside a nibble run", "second token of a pair -1",
              "second token of a pair +0", "second token of a pair +1", "exactly at the size")


def _pairs_to_cut(s, steps):
    """The second tokens whose ends get capacities.  Family E: the first pair of every (first, second).  Family D's pair streams:
    the pair at each of their points.  Elsewhere the fillers make pairs by the dozen: the first two."""
    found = pairs_in(steps)
    if s.family == "E":
        first_of = {}
        for first, second, j in found:
            first_of.setdefault((first, second), j)
        return sorted(first_of.values())
    if s.family == "D":
        points = s.notes.get("pair_points", ())
        pos = steps[:, 4]
        return sorted({min((j for _, _, j in found if pos[j] >= at), default=None) for at in points} - {None})
    return sorted({j for _, _, j in found})[:2]


@functools.lru_cache(maxsize=None)
def cut_capacities(name):
    """((capacity, places)) of a stream, read from the model's trace of the whole stream: a capacity inside its first run of two
    literals or more, inside its first copy, inside its first nibble of fifteen, at the end of the second token of its pairs
    (_pairs_to_cut) -1, 0 and +1, and exactly at its size.  Capacities above the size are whole decodes and are not listed."""
    s = by_name(name)
    total, steps = steps_of(s.data)
    kinds, lens, pos = steps[:, 1], steps[:, 3], steps[:, 4]
    caps = {}

    def add(cap, place):
        if 0 <= cap <= total:
            caps.setdefault(int(cap), []).append(place)

    i = 0
    while i < len(steps):
        if kinds[i] == K["lit"]:
            j = i
            while j < len(steps) and kinds[j] == K["lit"]:
                j += 1
            if j - i >= 2:
                add(int(pos[i]) + (j - i) // 2, CUT_PLACES[0])
                break
            i = j
        else:
            i += 1
    for i in range(len(steps)):
        if kinds[i] in COPY_TOKENS and lens[i] >= 2:
            add(int(pos[i]) + 1, CUT_PLACES[1])
            break
    for i in range(len(steps)):
        if kinds[i] == K["nib15"]:
            add(int(pos[i]) + 7, CUT_PLACES[2])
            break
    for j in _pairs_to_cut(s, steps):
        end = int(pos[j]) + int(lens[j])
        for d in (-1, 0, 1):
            add(end + d, CUT_PLACES[4 + d])
    add(total, CUT_PLACES[6])
    return tuple((cap, tuple(places)) for cap, places in sorted(caps.items()))


WHOLE_CLASSES = (64, 512, 2048, 8192)


def whole_capacity(s):
    """A capacity above the stream's output: the next of a few sizes, so that whole decodes share their launches -- and no less than
    half the stream's length (family I: most of it lies behind the first marker), below which eight rows cannot be plain."""
    total = total_of(s)
    return next(c for c in WHOLE_CLASSES if c > total and 2 * c >= len(s.data))


def capacities(s):
    """[(capacity, whole, places)]: the whole decode first, then the cut capacities."""
    return [(whole_capacity(s), True, ("whole",))] + [(cap, False, places) for cap, places in cut_capacities(s.name)]


# ---------------------------------------------------------------------------------------------------------------- the file rule
def replay(data, cap):
    """The bytes of ``data`` under the file rule at capacity ``cap``: the model's step trace replayed -- a literal's value is read
    from the stream at the step's bit, a copy takes its bytes from what was replayed so far (zeros in front of the first byte)."""
    total, steps = steps_of(data, cap, True)
    word, nbits = int.from_bytes(data, "big"), 8 * len(data)
    out = bytearray()
    for bit, kind, off, n, pos in steps.tolist():
        assert pos == len(out)
        if kind == K["lit"]:
            if n:
                out.append((word >> (nbits - bit - 9)) & 0xFF)
        else:
            for _ in range(n):
                out.append(out[-off] if off <= len(out) else 0)
    assert len(out) == total
    return bytes(out)


def concat_plan(s):
    """{form: (capacity, whole)} for lzs_decompress_concat on the one stream ``s``: the capacity alone picks the form.  Whole where
    form_of allows a capacity that holds all of the output, cut otherwise."""
    n = len(s.data)
    total = steps_of(s.data, BIG, True)[0]
    plan = {"plain": (max(total, 4 * n), True)}
    lo, hi = 10 * n // 9 + 1, 4 * n - 1                                 # the capacities of TWO
    plan["two"] = (max(total, lo), True) if total <= hi else (hi, False)
    top = 10 * n // 9                                                   # the largest capacity of WIDE
    plan["wide"] = (top, total <= top)
    for form, (cap, whole) in plan.items():
        assert form_of(n, cap) == form and whole == (cap >= total), (s.name, form, cap)
    return plan


# ---------------------------------------------------------------------------------------------------------------- the composer
NOISE = np.random.default_rng(99).integers(0, 256, 1 << 15, dtype=np.uint8).tobytes()
ROW_MAX = len(NOISE)
TAILS = ("ff", "random", "rest")
TAIL_BYTES = 12


def marker_row(length):
    """A row of ``length`` bytes that begins with an end marker: it decodes to nothing and is never read past the marker."""
    assert 2 <= length <= ROW_MAX
    return b"\xC0\x00" + NOISE[:length - 2]


def _split(extra, k):
    """``extra`` bytes over at most ``k`` marker rows (two bytes a row at least), the other rows empty; None if they do not fit."""
    if extra == 0:
        return [0] * k
    rows = min(k, extra // 2)
    if rows == 0 or (extra + rows - 1) // rows > ROW_MAX:
        return None
    lens = [extra // rows + (1 if r < extra % rows else 0) for r in range(rows)]
    return lens + [0] * (k - rows)


def _extra_for(form, total, full):
    """Compressed bytes to add to ``total`` so that it has ``form`` against ``full``; None where adding cannot."""
    a, b, c = FORM_FACTORS
    if form == "plain":
        extra = 0
    elif form == "two":
        extra = max(0, full // a + 1 - total)
    else:
        extra = max(0, (c * full + b - 1) // b - total)
    if extra == 1:
        extra = 2
    return extra if form_of(total + extra, full) == form else None


def tune_strided(total, packets, cap, form, kmin, kmax=None):
    """Companion rows for a strided call -- full = rows x cap -- whose streams under test have ``total`` bytes in ``packets``
    rows: the lengths of kmin .. kmax companions (0: an empty row), or None where no such set gives ``form``.  ``kmax`` None: as
    many as form_of needs -- empty rows until ``total`` alone is at most a quarter of the room (plain) or below nine tenths of it
    (TWO); with no capacity the room is 0 whatever the rows, and every wavefront is WIDE."""
    a, b, c = FORM_FACTORS
    if kmax is None:
        if cap:
            need = {"plain": -(-a * total // cap), "two": b * total // (c * cap) + 1, "wide": 0}[form] - packets
            kmin = max(kmin, need)
        kmax = kmin + 64                                               # (more rows only where the bytes to add need them)
    for k in range(kmin, kmax + 1):
        extra = _extra_for(form, total, (packets + k) * cap)
        if extra is not None:
            lens = _split(extra, k)
            if lens is not None:
                return lens
    return None


def tune_packed(total, rooms, form, k):
    """Companions for a packed call -- full = the sum of the rooms --: (lengths of k rows, their rooms).  The last companion is an
    empty row whose room lowers the ratio; every form is within reach."""
    a, b, c = FORM_FACTORS
    extra, room = 0, 0
    if form == "plain":
        room = max(0, a * total - rooms)
    elif form == "wide":
        extra = _extra_for("wide", total, rooms)
    else:
        extra = max(0, rooms // a + 1 - total)
        extra = 2 if extra == 1 else extra
        if b * (total + extra) >= c * rooms:
            room = 2 * (total + extra) - rooms
    assert form_of(total + extra, rooms + room) == form, (total, rooms, form)
    lens = _split(extra, k - 1)
    assert lens is not None
    return lens + [0], [0] * (k - 1) + [room]


@dataclass
class Wave:
    """One composed wavefront: eight rows, the stream under test at ``pos``."""
    stream: Stream
    cap: int
    whole: bool
    form: str
    pos: int
    rows: list                  # eight byte strings
    rooms: list = None          # packed: the room of each row
    tail: str = "random"

    @property
    def total(self):
        return sum(len(r) for r in self.rows)


def compose(s, cap, form, pos, packed=False, whole=False, tail="random"):
    """The eight rows of one wavefront with ``s`` at group position ``pos`` and room ``cap``, in ``form``; None where form_of puts
    the form out of reach (strided calls only: eight rows share one capacity)."""
    n = len(s.data)
    if packed:
        lens, rooms = tune_packed(n, cap, form, LANES - 1)
    else:
        lens, rooms = tune_strided(n, 1, cap, form, LANES - 1, LANES - 1), None
        if lens is None:
            return None
    others = [marker_row(k) if k else b"" for k in lens]
    rows = others[:pos] + [s.data] + others[pos:]
    if packed:
        rooms = rooms[:pos] + [cap] + rooms[pos:]
        assert form_of(sum(len(r) for r in rows), sum(rooms)) == form
    else:
        assert form_of(sum(len(r) for r in rows), LANES * cap) == form
    return Wave(s, cap, whole, form, pos, rows, rooms, tail)


def left_out(packed=False, families=FAMILIES):
    """[(stream, capacity, form)]: the cut capacities no composed wavefront of eight rows reaches in that form."""
    out = []
    for s in by_family(*families):
        for cap, whole, _ in capacities(s):
            for form in FORMS:
                if packed:
                    continue
                if tune_strided(len(s.data), 1, cap, form, LANES - 1, LANES - 1) is None:
                    assert not whole, (s.name, cap, form)
                    out.append((s.name, cap, form))
    return out


@functools.lru_cache(maxsize=None)
def waves(packed, families=FAMILIES):
    """Every stream of the families, whole and at each cut capacity, in every form within reach; the streams sit at the eight
    group positions in turn, family G's whole decodes at four of them in a row (the four input alignments), and family F's rows
    end in each kind of tail."""
    out, turn = [], 0
    for s in by_family(*families):
        for cap, whole, _ in capacities(s):
            for form in FORMS:
                times = 4 if s.family == "G" and whole else (3 if s.family == "F" and whole else 1)
                for t in range(times):
                    w = compose(s, cap, form, turn % LANES, packed, whole, TAILS[(turn if times != 3 else t) % 3])
                    if w is not None:
                        out.append(w)
                    turn += 1
    return tuple(out)


def _tail_of(w, r):
    if r != w.pos or w.tail == "random":
        return NOISE[100 + r:100 + r + TAIL_BYTES]
    if w.tail == "ff":
        return b"\xFF" * TAIL_BYTES
    rest = (w.stream.uncut or b"")[len(w.stream.data):] + NOISE[:TAIL_BYTES]
    return rest[:TAIL_BYTES]


@dataclass
class Placed:
    """Rows in one flat buffer.  Strided: row r begins at ``base`` + r * ``stride`` behind an aligned address, and ``stride`` is 1
    modulo 4, so that consecutive rows have the four alignments in turn.  Packed: row r begins at ``offsets[r]``."""
    flat: np.ndarray
    lens: np.ndarray
    base: int = 0
    stride: int = 0
    offsets: np.ndarray = None
    FRONT = 64

    def skew(self, r):
        at = self.FRONT + (self.base + r * self.stride if self.offsets is None else int(self.offsets[r]))
        return at % 4


def place_strided(rows, tails, base=1):
    stride = (max(len(r) for r in rows) + TAIL_BYTES + 3) // 4 * 4 + 1
    blob = b"".join(r + t + bytes(stride - len(r) - len(t)) for r, t in zip(rows, tails))
    flat = np.zeros(Placed.FRONT + base + len(blob) + 128, dtype=np.uint8)
    flat[Placed.FRONT + base:Placed.FRONT + base + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    return Placed(flat, np.array([len(r) for r in rows], dtype=np.int32), base, stride)


def place_packed(rows, tails):
    """Row r at the next offset that is r modulo 4, its tail behind it."""
    parts, offsets, at = [], [], 0
    for r, (row, tail) in enumerate(zip(rows, tails)):
        gap = (r - at) % 4
        parts.append(bytes(gap) + row + tail)
        offsets.append(at + gap)
        at += gap + len(row) + len(tail)
    blob = b"".join(parts)
    flat = np.zeros(Placed.FRONT + len(blob) + 128, dtype=np.uint8)
    flat[Placed.FRONT:Placed.FRONT + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    return Placed(flat, np.array([len(r) for r in rows], dtype=np.int32), offsets=np.array(offsets, dtype=np.int64))


def rows_and_tails(ws):
    rows = [r for w in ws for r in w.rows]
    tails = [_tail_of(w, r) for w in ws for r in range(len(w.rows))]
    return rows, tails


def strided_batches(families=FAMILIES):
    """{capacity: waves}: the strided calls take one capacity a launch."""
    groups = {}
    for w in waves(False, families):
        groups.setdefault(w.cap, []).append(w)
    return groups


def companion_result(row, cap):
    """(status) of a companion row: an end marker first (END), or nothing at all (STARVED; FULL where there is no room)."""
    return 0x04 if row else (0x08 if cap == 0 else 0x03)


# ---------------------------------------------------------------------------------------------------------------- runs (bursts)
def _filler_packet():
    p = Program(12)
    for _ in range(12):
        p.filler_lit()
    p.short(5, 4)
    p.marker()
    return p.bytes()


FILLER = _filler_packet()
FILLER_OUT = 16


@dataclass
class RunCall:
    """One burst call of at most eight runs, so one wavefront: run i, on channel i, is [FILLER, stream, stream] for the i-th
    stream under test; the last run is the companions'.  ``packets`` and ``ids`` are in call order (the runs' packets in turn)."""
    streams: list
    cap: int
    form: str
    packets: list
    ids: list
    rooms: list = None          # packed
    under_test: list = None     # per stream: the indices of its three packets
    caps: list = None           # packed: each stream's room


def compose_runs(group, form, packed, cap=None):
    """A RunCall for the streams of ``group`` -- [(stream, capacity)], at most seven, strided: all at one capacity -- or None."""
    runs, rooms = [], []
    for s, c in group:
        runs.append([FILLER, s.data, s.data])
        rooms.append([FILLER_OUT, c, c])
    total = sum(len(pk) for run in runs for pk in run)
    if packed:
        lens, crooms = tune_packed(total, sum(sum(r) for r in rooms), form, LANES - 1)
    else:
        lens = tune_strided(total, 3 * len(runs), cap, form, 1)
        if lens is None:
            return None
        crooms = [0] * len(lens)
    runs.append([marker_row(k) if k else b"" for k in lens])
    rooms.append(crooms)
    packets, ids, prooms, where = [], [], [], [[] for _ in runs]
    for j in range(max(len(run) for run in runs)):
        for c, run in enumerate(runs):
            if j < len(run):
                where[c].append(len(packets))
                packets.append(run[j])
                ids.append(c)
                prooms.append(rooms[c][j])
    npk = len(packets)
    full = sum(prooms) if packed else npk * cap
    assert form_of(sum(len(pk) for pk in packets), full) == form and len(runs) <= LANES
    return RunCall([s for s, _ in group], cap, form, packets, ids, prooms if packed else None, where[:-1], [c for _, c in group])


def run_reachable(s, cap, form):
    return tune_strided(len(FILLER) + 2 * len(s.data), 3, cap, form, 1) is not None


@functools.lru_cache(maxsize=None)
def run_calls(packed, families=FAMILIES):
    """Every (stream, capacity, form) within reach as burst calls of up to seven runs under test each; strided calls group the
    streams that share a capacity.  The companions' run holds as many empty packets as the form needs, so a strided call leaves
    out only plain and TWO at capacity 0, where form_of knows WIDE alone.  Returns (calls, the triples left out)."""
    todo, out, missing = {}, [], []
    for s in by_family(*families):
        for cap, whole, _ in capacities(s):
            for form in FORMS:
                if packed or run_reachable(s, cap, form):
                    todo.setdefault((form,) if packed else (form, cap), []).append((s, cap))
                else:
                    assert not whole
                    missing.append((s.name, cap, form))
    for key, items in todo.items():
        form = key[0]
        i = 0
        while i < len(items):
            m = min(LANES - 1, len(items) - i)
            while True:
                call = compose_runs(items[i:i + m], form, packed, None if packed else key[1])
                if call is not None:
                    break
                m = max(1, m // 2)
                assert m >= 1
            out.append(call)
            i += m
    return tuple(out), tuple(missing)
