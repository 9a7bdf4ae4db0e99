"""No device: the streams of tests/block_decoder_programs.py are what their builders say -- read from the oracle's traces, not from
the builders --, the composer puts every one of them into every form the kernels' inequalities allow, the file rule's replay is
the model's, and the constants all of this stands on are the source's.  tests/test_gpu_block_decoder_forms.py then decodes the
same wavefronts on the device.
"""
import os
import re

import numpy as np

import oracle
import block_decoder_programs as P
from block_decoder_programs import K
from stream_border_programs import FIRSTS, SECONDS

O = oracle.oracle()
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lzs_compression_amd", "csrc")
NAME = {i: name for name, i in K.items()}


def _steps(s, file_rule=False):
    return P.steps_of(s.data, P.BIG, file_rule)[1]


def _chain(steps, i):
    """Bytes of the copy whose token is step i, with its nibbles."""
    n, j = int(steps[i, 3]), i + 1
    while j < len(steps) and steps[j, 1] in P.NIBBLES:
        n += int(steps[j, 3])
        j += 1
    return n


# ------------------------------------------------------------------------------------------------ the models agree
def test_the_two_decoder_models_agree_on_every_stream_and_capacity():
    count = 0
    for s in P.streams():
        for cap, _, _ in P.capacities(s):
            out, status, hist = O.decompress_channel(b"", s.data, cap)
            assert out == O.decompress(s.data, cap), (s.name, cap)
            assert hist == out[-2047:]
            count += 1
    assert count > 4000


def test_the_replay_is_the_decoder_where_there_is_one_marker_and_the_models_length_everywhere():
    single = 0
    for s in P.streams():
        steps = _steps(s, True)
        markers = np.flatnonzero(steps[:, 1] == K["marker"])
        caps = {cap for cap, _, _ in P.capacities(s)} | {cap for cap, _ in P.concat_plan(s).values()}
        for cap in sorted(caps):
            got = P.replay(s.data, cap)
            assert len(got) == O.scan_segments(s.data, 256, cap, file_rule=True)[0], (s.name, cap)
            if len(markers) == 0 or markers[0] == len(steps) - 1:
                assert got == O.decompress(s.data, cap), (s.name, cap)
                single += 1
    assert single > 3000
    # several markers: the first stream's bytes are the one-shot decoder's, and the rest go on from there
    for s in P.by_family("I"):
        whole = P.replay(s.data, P.BIG)
        first = O.decompress(s.data, P.BIG)
        assert whole[:len(first)] == first and len(whole) > len(first) + 300


def test_companion_rows_decode_to_nothing():
    for length in (2, 3, 17, 4000, P.ROW_MAX):
        for cap in (0, 1, 50):
            assert O.decompress_channel(b"", P.marker_row(length), cap)[:2] == (b"", P.companion_result(b"x", cap))
            assert O.decompress_channel(b"abc", P.marker_row(length), cap)[2] == b"abc"
            _, stop = O.decompress_channel(b"", P.marker_row(length), cap, trace=True)[3:]
            assert stop == 0                                           # it stops at bit 0: nothing behind the marker is read
    for cap in (0, 1, 50):
        assert O.decompress_channel(b"", b"", cap)[:2] == (b"", P.companion_result(b"", cap))


# ------------------------------------------------------------------------------------------------ reach
def test_family_a_every_run_length_at_every_phase_with_every_follower():
    seen = set()
    for s in P.by_family("A"):
        steps = _steps(s)
        kinds, n = steps[:, 1], len(steps)
        for i in range(1, n):
            if kinds[i - 1] in P.CLOSING and kinds[i] == K["lit"]:
                j = i
                while j < n and kinds[j] == K["lit"]:
                    j += 1
                follower = "end" if j == n else {"short2": "short", "long4": "long"}.get(NAME[int(kinds[j])], NAME[int(kinds[j])])
                seen.add((j - i, int(steps[i, 0]) % 8, follower))
    want = {(r, phase, f) for r in range(1, 17) for phase in range(8) for f in P.A_FOLLOWERS}
    assert not want - seen, sorted(want - seen)[:10]


def test_family_b_every_offset_with_every_length_and_nibble():
    nibbles, lengths, forms, close0 = set(), set(), set(), 0
    for s in P.by_family("B"):
        steps = _steps(s)
        for i, (bit, kind, off, n, pos) in enumerate(steps.tolist()):
            if kind in P.NIBBLES:
                nibbles.add((off, n))
                close0 += kind == K["close0"]
            elif kind in P.COPY_TOKENS:
                lengths.add((off, n))
                forms.add((off, NAME[kind][:-1], _chain(steps, i)))
    assert not {(o, e) for o in range(1, 17) for e in range(1, 16)} - nibbles          # both byte slots' replication tables
    assert not {(o, n) for o in range(1, 18) for n in range(2, 9)} - lengths
    want = {(o, "long" if lf else "short", n) for o, lf in P.B_OFFSETS for n in P.B_LENGTHS}
    assert not want - forms, sorted(want - forms)[:10]
    assert close0 >= 3 * len(P.B_OFFSETS)                                             # lengths 8, 23 and 38 close on nibble 0


def test_family_b_reads_every_entry_of_the_replication_tables_a_token_can_reach():
    """A step's first token is 15 bytes at the most (a nibble of fifteen), so bytes 0 .. 14 of offsets 1 .. 15 are all of the
    tables (mod_lo, mod_hi) that is ever read for replication: the streams read every one of them, and byte 15 -- lane 7's
    second slot -- belongs to no first token (in TWO it is the second's, which does not replicate).  So `off_now < 16u` and
    `< 15u` in the second slot's lookup are the same decoder.  More than that: the second slot reads the window after the first
    slot has written bytes 0 .. 7 of the step, and without the table byte idx comes from byte idx - off of the same step, which
    for off >= 7 and idx <= 14 is one of those eight and holds the replicated value already.  Builds with 15 and with 14 in that
    line ran the whole GPU suite and these tests without a difference; 6 is the first bound that changes a byte (offset 6, byte
    14 reads byte 8, not written yet), and that build fails these tests."""
    read = set()
    for s in P.by_family("B"):
        for bit, kind, off, n, pos in _steps(s).tolist():
            if kind in P.NIBBLES or kind in P.COPY_TOKENS:
                assert n <= 15
                read |= {(off, idx) for idx in range(n)}
    assert not {(off, idx) for off in range(1, 16) for idx in range(15)} - read
    longest = max(int(n) for s in P.streams() for n in _steps(s)[:, 3])
    assert longest == 15


def test_family_c_first_copies_from_in_front_of_the_output():
    seen = {}
    for s in P.by_family("C"):
        steps = _steps(s)
        i = next(i for i in range(len(steps)) if steps[i, 1] in P.COPY_TOKENS)
        assert (steps[:i, 1] == K["lit"]).all()
        pos, off, length = int(steps[i, 4]), int(steps[i, 2]), _chain(steps, i)
        assert off > pos                                               # its source begins in the zeros
        seen.setdefault(pos, set()).add((off, length))
    assert sorted(seen) == list(range(17))
    for q, got in seen.items():
        assert got == set(P.c_copies(q))
        assert any(off < length and off < q + length for off, length in got)          # replicates, and lies partly in the zeros
        assert any(off == 2047 for off, _ in got)


def test_family_d_every_crossing_with_its_token_kind():
    seen = set()
    for s in P.by_family("D"):
        steps = _steps(s)
        kind, d = s.notes["kind"], s.notes["d"]
        at = {int(steps[i, 4]): i for i in range(len(steps)) if steps[i, 3]}          # the step that produces each position's byte
        pairs = {j for _, _, j in P.pairs_in(steps)}
        for point in P.D_POINTS:
            i = at[point - d]
            k, off = int(steps[i, 1]), int(steps[i, 2])
            if kind == "lits7":
                ok = (steps[i:i + 7, 1] == K["lit"]).all() and steps[i + 7, 1] != K["lit"] and steps[i - 1, 1] == K["close0"]
            elif kind == "nib15-offset1":
                ok = k == K["nib15"] and off == 1
            elif kind == "copy2047":
                ok = k == K["long4"] and off == 2047 and steps[i, 3] == 7
            elif kind == "copy2047-extended":
                ok = k == K["long8"] and off == 2047 and _chain(steps, i) == 8 + 15 * 6
            else:
                ok = k == K["short8"] and any(i < j <= i + 7 for j in pairs)
            assert ok, (s.name, point)
            seen.add((kind, point, d))
        assert P.total_of(s) > 2 * P.RING                             # past ring position 2304 twice
    assert seen == {(kind, point, d) for kind in P.D_KINDS for point in P.D_POINTS for d in range(16)}


def _pairs_seen(steps):
    """(first, second) of every two steps that a decoder taking two tokens a trip could take together (adapted from
    tests/test_stream_border_model.py: no segment borders here)."""
    return {(first, second) for first, second, _ in P.pairs_in(steps)}


def test_family_e_every_first_token_with_every_second():
    seen = set()
    for s in P.by_family("E"):
        if s.uncut is None:
            seen |= _pairs_seen(_steps(s))
            assert _steps(s)[-1, 1] == K["marker"]
    want = {(f, sec) for f in FIRSTS for sec in SECONDS}
    assert not want - seen, sorted(want - seen)
    # a second token whose last field the end of the input cuts off: all steps but that one, so the first token's bytes come out
    cut = [s for s in P.by_family("E") if s.uncut is not None]
    assert len(cut) == len(FIRSTS)
    for s in cut:
        whole, part = P.steps_of(s.uncut)[1], _steps(s)
        assert part.tolist() == whole[:-1].tolist() and whole[-1, 1] in P.SHORT_MATCHES, s.name
        assert P.total_of(s) == P.steps_of(s.uncut)[0] - s.notes["second_len"]
        first = part[-1]
        assert first[1] in P.SHORT_MATCHES or first[1] == K["lit"]


def test_family_f_every_last_token_at_every_phase_cut_one_and_two_bytes_short():
    seen = set()
    for s in P.by_family("F"):
        whole, part = P.steps_of(s.uncut)[1], _steps(s)
        kind, phase, short_by = s.notes["kind"], s.notes["phase"], s.notes["short_by"]
        i = int(np.flatnonzero(whole[:, 0] == s.notes["last_token"])[0])
        assert NAME[int(whole[i, 1])] == ("short8" if kind == "nibbles" else kind) and int(whole[i, 0]) % 8 == phase, s.name
        assert len(whole) - i == {"nibbles": 4, "short8": 2, "long8": 2}.get(kind, 1)          # it is the last token
        assert len(s.data) == len(s.uncut) - short_by
        assert len(part) < len(whole) and part[:, 0].tolist() == whole[:len(part), 0].tolist(), s.name
        seen.add((kind, phase, short_by))
    assert seen == {(k, ph, c) for k in P.F_KINDS for ph in range(8) for c in (1, 2)}


def _skews_and_sides(waves, placed):
    got = set()
    for wi, w in enumerate(waves):
        if w.stream.family == "G" and w.whole:
            skew, n = placed.skew(P.LANES * wi + w.pos), len(w.stream.data)
            for border in (P.CHUNK, 2 * P.CHUNK):
                if abs(n - border) <= 12:
                    got.add((border, skew, skew + n > border))
    return got


def test_family_g_the_feed_at_every_skew_on_both_sides_of_a_chunk_border():
    assert tuple(len(s.data) for s in P.by_family("G")) == P.G_LENGTHS
    for s in P.by_family("G"):
        steps = _steps(s)
        i = int(np.flatnonzero(steps[:, 1] != K["lit"])[0])
        assert steps[i, 1] in (K["short8"], K["long8"]) and _chain(steps, i) == P.G_COPY and steps[-1, 1] == K["marker"]
        assert i > 90                                                  # all literals in front: the feed is what the loop waits for
    want = {(border, skew, side) for border in (P.CHUNK, 2 * P.CHUNK) for skew in range(4) for side in (False, True)}
    for cap, ws in P.strided_batches("G").items():
        rows, tails = P.rows_and_tails(ws)
        want -= _skews_and_sides(ws, P.place_strided(rows, tails))
    assert not want, sorted(want)
    ws = P.waves(True, "G")
    rows, tails = P.rows_and_tails(ws)
    assert len(_skews_and_sides(ws, P.place_packed(rows, tails))) == 16


def test_family_h_long_extensions():
    seen = set()
    for s in P.by_family("H"):
        steps = _steps(s)
        for i in range(len(steps)):
            if steps[i, 1] in P.COPY_TOKENS:
                seen.add((int(steps[i, 2]), _chain(steps, i)))
    assert seen == {(off, n) for off in (1, 3, 2047) for n in (P.H_COPY, P.H_COPY // 2)}


def test_family_i_streams_back_to_back_under_the_file_rule():
    pads, firsts = set(), set()
    for s, (kind, nstreams), (lo, hi) in zip(P.by_family("I"), P.I_PROGRAMS, ((1.0, 1.125), (0.5, 0.65), (0.07, 0.13))):
        total, steps = P.steps_of(s.data, P.BIG, True)
        assert lo <= len(s.data) / total <= hi, (s.name, len(s.data) / total)
        markers = np.flatnonzero(steps[:, 1] == K["marker"])
        assert len(markers) == nstreams and markers[-1] == len(steps) - 1
        starts = [0] + [int(steps[m, 4]) for m in markers[:-1]]        # output position of each stream's first byte
        reach_back = 0
        for m, nxt in zip(markers, list(markers[1:]) + [None]):
            end = int(steps[m, 0]) + 9
            pads.add((int(steps[m + 1, 0]) if nxt is not None else 8 * len(s.data)) - end)
        for k in range(1, nstreams):
            lo_step, hi_step = int(markers[k - 1]) + 1, int(markers[k])
            reach_back += any(steps[i, 1] in P.COPY_TOKENS and int(steps[i, 4]) - int(steps[i, 2]) < starts[k]
                              and int(steps[i, 4]) - int(steps[i, 2]) >= 0 for i in range(lo_step, hi_step))
        assert reach_back == nstreams - 1, s.name                       # every later stream copies from an earlier one
        firsts |= {first for first, second, _ in P.pairs_in(steps) if second == "marker"}
    assert pads == set(range(8)), pads
    assert firsts == set(FIRSTS)


# ------------------------------------------------------------------------------------------------ the composer
def test_the_composer_yields_every_form_the_inequalities_allow():
    assert [P.form_of(t, f) for t, f in ((25, 100), (26, 100), (89, 100), (90, 100), (0, 0), (1, 0), (0, 1))] == \
        ["plain", "two", "two", "wide", "wide", "wide", "plain"]
    for packed in (False, True):
        ran, missing = {}, set(P.left_out(packed))
        positions, skews = set(), set()
        for w in P.waves(packed):
            full = sum(w.rooms) if packed else P.LANES * w.cap
            assert len(w.rows) == P.LANES and w.rows[w.pos] is w.stream.data
            assert P.form_of(w.total, full) == w.form, (w.stream.name, w.cap, w.form)
            assert all(r == b"" or r[:2] == b"\xC0\x00" for i, r in enumerate(w.rows) if i != w.pos)
            if packed:
                assert w.rooms[w.pos] == w.cap
            ran.setdefault((w.stream.name, w.cap), set()).add(w.form)
            positions.add(w.pos)
        assert positions == set(range(P.LANES))
        for s in P.streams():
            forms_cut = set()
            for cap, whole, _ in P.capacities(s):
                got = ran.get((s.name, cap), set())
                gone = {form for form in P.FORMS if (s.name, cap, form) in missing}
                assert got | gone == set(P.FORMS) and not got & gone, (s.name, cap)
                if whole:
                    assert not gone, (s.name, cap)                     # whole decodes leave out nothing
                else:
                    forms_cut |= got
            assert forms_cut == set(P.FORMS), (s.name, forms_cut)      # still a cut capacity in every form
        if packed:
            assert not missing                                         # the rooms reach everything
        else:
            # what eight rows at one capacity cannot reach: plain below n / 2, TWO from 7.2 times the capacity on
            for name, cap, form in missing:
                n = len(P.by_name(name).data)
                assert (form == "plain" and n > 2 * cap) or (form == "two" and 10 * n >= 72 * cap), (name, cap, form)
    # the placements: rows at all four alignments, under the streams under test too
    for place, ws in ((P.place_strided, P.strided_batches("A")[P.WHOLE_CLASSES[1]]), (P.place_packed, P.waves(True, "C"))):
        rows, tails = P.rows_and_tails(ws)
        placed = place(rows, tails)
        assert {placed.skew(P.LANES * wi + w.pos) for wi, w in enumerate(ws)} == {0, 1, 2, 3}
        for r, row in enumerate(rows):
            at = P.Placed.FRONT + (placed.base + r * placed.stride if placed.offsets is None else int(placed.offsets[r]))
            assert placed.flat[at:at + len(row)].tobytes() == row and placed.lens[r] == len(row)


def test_the_burst_calls_are_one_wavefront_in_the_wanted_form():
    for packed in (False, True):
        calls, missing = P.run_calls(packed)
        assert not (packed and missing)
        ran = set()
        for c in calls:
            assert len(set(c.ids)) <= P.LANES and 1 <= len(c.streams) <= P.LANES - 1
            total = sum(len(pk) for pk in c.packets)
            full = sum(c.rooms) if packed else len(c.packets) * c.cap
            assert P.form_of(total, full) == c.form
            for s, where, cap in zip(c.streams, c.under_test, c.caps):
                assert [c.packets[i] for i in where] == [P.FILLER, s.data, s.data] and len({c.ids[i] for i in where}) == 1
                ran.add((s.name, cap, c.form))
        want = {(s.name, cap, form) for s in P.streams() for cap, _, _ in P.capacities(s) for form in P.FORMS}
        assert ran | set(missing) == want and not ran & set(missing)
        # the companions' run takes as many empty packets as the form needs: only a capacity of 0 -- no room whatever the rows,
        # so form_of knows WIDE alone -- puts plain and TWO out of a strided call's reach, and no stream here has such a cut
        assert all(cap == 0 and form != "wide" for _, cap, form in missing)
        assert not missing
        assert all(not whole or (s.name, cap, form) in ran for s in P.streams() for cap, whole, _ in P.capacities(s) for form in P.FORMS)
    assert len(O.decompress(P.FILLER, 100)) == P.FILLER_OUT


def test_the_cut_capacities_are_the_places_they_name():
    places = set()
    for s in P.streams():
        total, steps = P.steps_of(s.data)
        for cap, whole, where in P.capacities(s):
            assert whole == (cap > total)
            places |= set(where)
            cut = P.steps_of(s.data, cap)[1]
            last = cut[-1] if len(cut) else None
            if "inside a literal run" in where:
                assert last[1] == K["lit"] and steps[len(cut), 1] == K["lit"]
            if "inside a first copy" in where:
                assert last[1] in P.COPY_TOKENS and last[3] == 1 and not (steps[:len(cut) - 1, 2] > 0).any()
            if "inside a nibble run" in where:
                assert last[1] == K["nib15"] and last[3] == 7
            if "exactly at the size" in where:
                assert cap == total
    assert places == set(P.CUT_PLACES) | {"whole"}
    # every pair of family E has its three capacities -- the end of its second token - 1, + 0, + 1, up to the size -- and each is
    # where the trace says that token ends
    got = set()
    for s in P.by_family("E"):
        if s.uncut is not None:
            continue
        total, steps = P.steps_of(s.data)
        caps = dict(P.cut_capacities(s.name))
        first_of = {}
        for first, second, j in P.pairs_in(steps):
            first_of.setdefault((first, second), j)
        for (first, second), j in first_of.items():
            assert steps[j - 1, 1] == K["lit"] or steps[j - 1, 1] in P.SHORT_MATCHES
            end = int(steps[j, 4]) + int(steps[j, 3])
            for d in (-1, 0, 1):
                if end + d <= total:
                    assert "second token of a pair %+d" % d in caps[end + d], (s.name, first, second, d)
                    cut_total, cut = P.steps_of(s.data, end + d)
                    assert cut_total == end + d
                    if steps[j, 3] and d == -1:                        # the second token is the one the room cuts
                        assert cut[-1, 0] == steps[j, 0] and cut[-1, 3] == steps[j, 3] - 1
                    if steps[j, 3] and d == 0:                         # it fits exactly: all of it is the last that produces bytes
                        last = cut[np.flatnonzero(cut[:, 3])[-1]]
                        assert last[0] == steps[j, 0] and last[3] == steps[j, 3]
            got.add((first, second))
    assert got >= {(f, sec) for f in FIRSTS for sec in SECONDS}


# ------------------------------------------------------------------------------------------------ constants
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_constants_are_the_sources():
    blocks, packed, common = _source("kernels/decompress_blocks.inc"), _source("kernels/decompress_packed.inc"), _source("kernels/common.inc")
    two = re.findall(r"\(\((\d+)ull \* total > full && (\d+)ull \* total < (\d+)ull \* full\)", blocks + packed)
    wide = re.findall(r"uniform\((\d+)ull \* total >= (\d+)ull \* full \?", blocks + packed)
    assert len(two) == 5 and len(wide) == 5                            # blocks, channels, runs; packed, packed runs
    assert set(two) == {tuple(str(v) for v in P.FORM_FACTORS)} and set(wide) == {tuple(str(v) for v in P.FORM_FACTORS[1:])}
    assert int(re.search(r"^constexpr uint32_t kDecLanes\s*=\s*(\d+);", blocks, re.M).group(1)) == P.LANES
    assert int(re.search(r"^#define LZS_DEC_DRAIN (\d+)$", blocks, re.M).group(1)) == P.DRAIN
    assert int(re.search(r"^#define LZS_DEC_TWO_MAX (\d+)$", blocks, re.M).group(1)) == P.TWO_MAX
    window = int(re.search(r"^constexpr uint32_t kWindow\s*=\s*(\d+);", common, re.M).group(1))
    assert "kDecRing   = (kWindow + kDecDrain + 15u + kDecPiece - 1u) / kDecPiece * kDecPiece;" in blocks
    assert "kDecPiece  = 16u * kDecLanes;" in blocks and "kChunk = 16u * kDecLanes;" in blocks
    piece = 16 * P.LANES
    assert (window + P.DRAIN + 15 + piece - 1) // piece * piece == P.RING and piece == P.CHUNK
    assert P.D_POINTS == (128, 256, 2304, 2432, 4608)
