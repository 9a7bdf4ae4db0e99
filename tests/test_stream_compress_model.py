"""oracle.compress_segments -- the plain model of what a segment border of the segmented stream compressor is --
held to itself, to the one-shot compressors on the CPU, and to the directed inputs of tests/stream_compress_programs.py: the model's
counters prove here that those inputs reach every case they were built for.  tests/test_gpu_stream_compress_model.py compresses the
same inputs on the device; it asserts no coverage of its own.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from oracle import COMPRESS_NEVER as NEVER, LAST_KINDS, LAST_PAST
import lzs_compression_amd as lzs
from lzs_compression_amd import api
import stream_compress_programs as P

O = oracle.oracle()
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F = {name: i for i, name in enumerate(oracle.COMPRESS_SEGMENT_FIELDS)}
SEGS = (256, 512)
SHORT_PIECE, LONG_PIECE = 64, 10400                                     # family G: the low-memory block, and more than the full block collects


def inputs(*families):
    return [i for i in P.directed_inputs() if not families or i.family in families]


@functools.lru_cache(maxsize=None)
def walked(seg, families=None):
    """The directed inputs (of these families) through the model: (counters of them all, {name: (bits, records, rounds, tokens)})."""
    counters, each = oracle.CompressCounters(), {}
    for i in inputs(*(families or ())):
        each[i.name] = O.compress_segments(i.data, seg, counters=counters, trace=True)
    return counters, each


def rows(rec, *fields):
    return [[int(v) if v != NEVER else -1 for v in r[[F[f] for f in fields]]] for r in rec]


# ---------------------------------------------------------------- the model against itself and the one-shot oracle
@pytest.mark.parametrize("seg", SEGS)
def test_model_is_consistent_with_itself_and_the_one_shot_compressor(seg):
    """On every directed input: the segments' bits add up to the oracle's stream less its end marker and padding, bit_at is their
    prefix sum, the segments' tokens one behind the other are O.trace's, exits chain into entries, an empty segment has nothing, the
    simulated rounds arrive at the true exits, and the brute-force finder gives the same records on the inputs of 8 KiB and less."""
    _, each = walked(seg)
    for i in inputs():
        bits, rec, rounds, tokens = each[i.name]
        n, nseg = len(i.data), (len(i.data) + seg - 1) // seg
        stream = O.compress(i.data)
        assert rec.shape == (nseg, len(F))
        assert (bits + 9 + 7) // 8 == len(stream) and int(rec[:, F["bits"]].sum()) == bits, i.name
        assert (rec[:, F["bit_at"]] == np.concatenate(([0], np.cumsum(rec[:, F["bits"]])[:-1]))).all(), i.name
        # the tokens: the one-shot oracle's, each where the one before ended, their bits running on
        want = O.trace(i.data)
        assert (tokens[:, :3] == want).all() and len(tokens) == len(want) == int(rec[:, F["tokens"]].sum()), i.name
        assert tokens[0, 0] == 0 and (tokens[1:, 0] == tokens[:-1, 0] + tokens[:-1, 2]).all() and tokens[-1, 0] + tokens[-1, 2] == n
        assert (np.diff(tokens[:, 3].astype(np.int64)) >= 9).all()
        # a token belongs to the segment in which it starts
        owner = tokens[:, 0] // seg
        assert (np.bincount(owner, minlength=nseg) == rec[:, F["tokens"]]).all(), i.name
        # exits chain into entries; an empty segment has no token, no bit, and hands its predecessor's exit on
        at = 0
        for k in range(nseg):
            entry, exit_, empty = int(rec[k, F["entry"]]), int(rec[k, F["exit"]]), int(rec[k, F["empty"]])
            assert empty == (at >= min((k + 1) * seg, n)), (i.name, k)
            if empty:
                assert rec[k, F["entry"]] == NEVER and exit_ == at and rec[k, F["tokens"]] == 0 and rec[k, F["bits"]] == 0
            else:
                assert entry == at and k * seg <= entry < (k + 1) * seg and exit_ > entry, (i.name, k)
            at = exit_
        assert at == n
        assert (rec[:, F["oversized"]] == (rec[:, F["bits"]] > oracle.slot_bits(seg))).all()
        # the rounds: the last one leaves nothing to redo, every one before it something; they arrive at the true exits; a segment
        # redone r times is counted in r of the rounds
        assert rounds[-1] == 0 and all(rounds[:-1]) and len(rounds) <= nseg, (i.name, rounds)
        assert (rec[:, F["round_exit"]] == rec[:, F["exit"]]).all(), i.name
        assert int(rec[:, F["redone"]].sum()) == sum(rounds), i.name
        # the guessed walk of a border that is a token start is the true one
        at_start = rec[:, F["entry"]] == np.arange(nseg) * seg
        assert (rec[at_start, F["guess_merge"]] == 0).all() and (rec[at_start, F["guess_exit"]] == rec[at_start, F["exit"]]).all()
        if n <= 8192:
            brute = O.compress_segments(i.data, seg, brute=True, trace=True)
            assert brute[0] == bits and (brute[1] == rec).all() and brute[2] == rounds and (brute[3] == tokens).all(), i.name
            assert O.compress_brute(i.data) == stream


def test_model_on_three_inputs_followed_by_hand():
    """(1) A match over one border.  Bytes 0 .. 253 (no 2-gram twice: 254 literals), bytes 10 .. 15 again (a copy of six from 244
    back, the long form: 13 + 4 bits), then 255, 254, .. 216.  Segment 0 of 256: 254 * 9 + 17 = 2303 bits, its last token ends at
    260, four bytes past the border.  The walk from 256 finds 12 13 14 15 at the same offset: one token, and it stands on 260.  Round
    0 enters segment 1 at 256, segment 0 leaves at 260: one to redo, nothing after round 1.
    (2) An oversized segment.  Bytes 0 .. 254 and 478 more of 254: 255 literals (2295 bits) and, from the segment's last byte on, a
    match at offset 1 -- 9 + 4 bits for its first eight bytes, 31 nibbles of 15 and a closing 5 for the other 470: 2295 + 13 + 32 *
    4 = 2436 bits, four more than the slot's 8 * 304 = 2432.  (With 31 nibbles it is 2432: it fits.)  The match ends at 733:
    segment 1 is empty.  Then 100, 99, .. 81: twenty literals.  The walk from 256 is one token that ends at 733, behind its segment
    -- never in step inside it; the one from 512 is that token too, and stands on 733, inside segment 2 (the input ends at 753).
    Round 0 leaves 733, 733, 753; segments 1 and 2 were entered at 256 and 512: two to redo.
    (3) Walks that never merge: B(16, 3) twice, 8192 bytes.  No 3-gram repeats inside the window, so no match is longer than two;
    from 4783 on every token is a match of two (the literals are 2-grams not seen for 2047 bytes: the model's token list has the
    last of them at 4782, but for the last byte), and they start at odd positions.  A walk from an even border takes matches of two
    at even positions and stays one byte off to the end of its segment: segments 19 .. 31 are entered at their border + 1, and the
    walks from their borders never merge (the last one ends with the input, where every walk ends).  After round 0 three segments
    have a predecessor that left elsewhere: 1, 17 (their walks merge: after 1 and 9 tokens) and 19.  Each round after it corrects
    one more of 19 .. 31, whose own exit then moves by one: thirteen rounds behind round 0, fourteen in all."""
    head = bytes(range(254))
    d = head + head[10:16] + bytes(range(255, 215, -1))
    bits, rec, rounds, tokens = O.compress_segments(d, 256, trace=True)
    assert len(d) == 300 and bits == 2303 + 360 and rounds == [1, 0]
    assert rows(rec, "entry", "exit", "tokens", "bits", "bit_at", "empty", "oversized", "guess_merge", "guess_exit", "redone") == [
        [0, 260, 255, 2303, 0, 0, 0, 0, 260, 0],
        [260, 300, 40, 360, 2303, 0, 0, 1, 300, 1]]
    assert [int(v) for v in tokens[254]] == [254, 244, 6, 2286]

    d = bytes(range(255)) + bytes([254]) * 478 + bytes(range(100, 80, -1))
    bits, rec, rounds, tokens = O.compress_segments(d, 256, trace=True)
    assert len(d) == 753 and oracle.slot_bits(256) == 2432 and rounds == [2, 0]
    assert rows(rec, "entry", "exit", "tokens", "bits", "bit_at", "empty", "oversized", "guess_merge", "guess_exit", "redone") == [
        [0, 733, 256, 2436, 0, 0, 1, 0, 733, 0],
        [-1, 733, 0, 0, 2436, 1, 0, -1, 733, 1],
        [733, 753, 20, 180, 2436, 0, 0, 1, 753, 1]]
    assert [int(v) for v in tokens[255]] == [255, 1, 478, 2295]
    fits = bytes(range(255)) + bytes([254]) * 463 + bytes(range(100, 80, -1))       # 30 nibbles of 15 and a closing 5
    assert rows(O.compress_segments(fits, 256)[1], "bits", "oversized")[0] == [2432, 0]

    d = P.de_bruijn(16, 3) * 2
    bits, rec, rounds, tokens = O.compress_segments(d, 256, trace=True)
    assert len(d) == 8192 and rounds == [3] + [1] * 12 + [0]
    assert max(int(t[2]) for t in tokens) == 2
    assert max(int(t[0]) for t in tokens[:-1] if t[2] == 1) == 4782 and all(int(t[0]) % 2 for t in tokens if t[0] > 4782)
    assert [r[0] for r in rows(rec, "guess_merge")] == [0, 1] + [0] * 15 + [9, 0] + [-1] * 13
    assert [int(r[F["entry"]]) - 256 * k for k, r in enumerate(rec)] == [0, 1] + [0] * 15 + [1, 0] + [1] * 13
    assert [r[0] for r in rows(rec, "redone")] == [0, 1] + [0] * 15 + [1, 0] + [1] * 13
    # (the guessed walk of each of 19 .. 30 leaves one byte short of where the true one leaves)
    assert [int(r[F["guess_exit"]]) - int(r[F["exit"]]) for r in rec[19:31]] == [-1] * 12


# ---------------------------------------------------------------- coverage, family by family
def _longest(kind):
    return {"lit": 1, "short2-7": 7, "long2-7": 7, "ext0": 22, "ext1": 37, "ext2": 52, "ext3-39": 607}.get(kind, 1 << 30)


def _impossible_last(seg):
    """The cells of the last-token matrix that the format cannot have, each with its reason."""
    out = {}
    for kind in LAST_KINDS:
        longest, shortest = _longest(kind), 608 if kind == "ext40+" else 1
        for past in range(LAST_PAST):
            why = None
            if past <= 16 and longest < past + 1:
                why = f"ends {past} past the border and starts in front of it: {past + 1} bytes and more, it has {longest} at most"
            elif past <= 17 and shortest - seg > (16 if past <= 16 else seg - 1):
                why = f"{shortest} bytes and more, of which {seg} at most lie in its own segment: it ends {shortest - seg} and more past the border"
            elif past == 17 and longest < 18:
                why = "17 and more past the border: 18 bytes and more"
            elif past == 18 and longest < 2:
                why = "a literal ends on the border at the latest"
            elif past >= 19 and longest < (past - 18) * seg + 2:
                why = f"over {past - 18} whole segments and into one more: {(past - 18) * seg + 2} bytes and more"
            if why:
                out[(kind, past)] = why
    return out


@pytest.mark.parametrize("seg", SEGS)
def test_coverage_a_the_last_token_of_a_segment_against_its_border(seg):
    c, _ = walked(seg, ("A",))
    impossible = _impossible_last(seg)
    for k, kind in enumerate(LAST_KINDS):
        for past in range(LAST_PAST):
            if (kind, past) in impossible:
                assert c.last[k, past] == 0, (kind, past, impossible[(kind, past)])
            else:
                assert c.last[k, past] > 0, (kind, past)
    everything = walked(seg)[0]                                          # ... and in no other family either
    for (kind, past), why in impossible.items():
        assert everything.last[LAST_KINDS.index(kind), past] == 0, (kind, past, why)
    assert c.last_close[:3].all(), c.last_close                          # closing nibbles 0, 1, 14 of tokens that cross
    assert c.last_start[1:].all(), c.last_start                          # starting 1 .. 8 bytes before the border
    assert c.one_token_last_byte[0] >= 1                                 # an entry at the last byte of its segment: one token
    assert c.entry_mod64.all(), c.entry_mod64                            # entries at every c0 & 63


@pytest.mark.parametrize("seg", SEGS)
def test_coverage_b_the_first_token_and_the_window(seg):
    c, _ = walked(seg, ("B",))
    assert c.first_off.all(), c.first_off                                # offsets 2047 2046 2040 1, warm-up at 0, first beyond, far
    assert c.first_straddle[0] >= 4
    assert c.first_far_len.all(), c.first_far_len                        # a source of two and of three bytes at the far edge
    assert np.count_nonzero(c.entry_mod64) >= 3                          # entries at 0, 1 and 63 past a multiple of 64


@pytest.mark.parametrize("seg", SEGS)
def test_coverage_c_rounds(seg):
    c, each = walked(seg, ("C",))
    assert each["C-every-border-a-token-start"][2] == [0] and c.one_round[0] >= 1
    assert c.merge[[1, 2, 4, 5]].all(), c.merge                          # guesses that merge after 1, 2, >= 5 tokens, and never
    assert c.fix_changes_exit[0] >= 1 and c.fix_keeps_exit[0] >= 1
    # the run of walks that never merge: eight segments and more at 256, and as many rounds; half of that at 512
    run = {256: 8, 512: 4}[seg]
    assert c.never_run_max[0] >= run and c.rounds_max[0] >= run + 1, (c.never_run_max, c.rounds_max)
    assert (c.long_match >= 10).all(), c.long_match                      # one byte, a period of 2, of 300: over ten segments and more
    for name in ("one-byte", "period-2", "period-300"):
        bits, rec, rounds, _ = each[f"C-long-match-{name}"]
        assert int(rec[:, F["empty"]].sum()) >= 10 and len(rounds) == 2, (name, rounds)


@pytest.mark.parametrize("seg", SEGS)
def test_coverage_d_stitch(seg):
    c, _ = walked(seg, ("D",))
    assert c.bit_at_mod32.all() and c.nbits_mod32.all(), (c.bit_at_mod32, c.nbits_mod32)
    assert c.under_32[0] >= 8 and c.word_share_max[0] >= 3
    assert c.empty_between_sharers[0] >= 1
    assert c.total_mod32.all(), c.total_mod32
    assert c.marker_behind_empty[0] >= 1
    # impossible: the marker right behind an oversized segment.  The last segment's tokens end with the input, 9 bits a byte at most:
    # less than a slot.  The marker behind an oversized segment has empty ones between: family E.
    assert all(not rec[-1, F["oversized"]] for _, rec, _, _ in walked(seg)[1].values())


@pytest.mark.parametrize("seg", SEGS)
def test_coverage_e_oversized_segments(seg):
    c, each = walked(seg, ("E",))
    if seg == 256:
        assert c.margin.all(), c.margin                                  # the slot's bits - 8 .. + 8, and far more
        for delta in range(-8, 9):
            rec = each[f"E-256-slot{delta:+d}"][1]
            assert int(rec[8, F["bits"]]) == oracle.slot_bits(256) + delta and int(rec[8, F["oversized"]]) == (delta > 0)
    else:
        assert c.margin[[7, 8, 9, 17]].all(), c.margin                   # (one either side, the limit itself, and far more)
    assert c.over_bit_at[[0, 1, 3]].all(), c.over_bit_at                 # bit_at % 2048: 0, 1 .. 31, >= 2017
    for name, phase in (("5", 5), ("31", 31), ("2047", 2047)):
        rec = each[f"E-{seg}-first-bit-at-{name}"][1]
        assert [int(r[F["bit_at"]]) % 2048 for r in rec if r[F["oversized"]]] == [phase], name
    assert c.over_seg0[0] >= 1 and c.over_two[0] >= 1 and c.over_empties_one_token[0] >= 1
    assert c.marker_behind_oversized[0] >= 1                             # (empty segments between it and the marker)


@pytest.mark.parametrize("seg", SEGS)
def test_coverage_f_lengths(seg):
    c, each = walked(seg, ("F",))
    assert c.len_mod.all(), c.len_mod                                    # n % seg: 1 (a last segment of one byte), 63, 64, 255, 0
    assert {len(i.data) for i in inputs("F")} >= {6144, 6145}
    assert c.end_close.all() and c.end_one_short[0] >= 1
    rec = each["F-last-segment-of-one-byte"][1]
    assert int(rec[-1, F["tokens"]]) == 1 and int(rec[-1, F["entry"]]) == len(rec) * seg - seg


def _describe(tokens, cut):
    """What a piece that ends at ``cut`` leaves: ("open", residue) inside a match that started more than 15 bytes before, else
    ("bit0", the bit at which the next piece begins, the bytes from there to the cut: they wait for their look-ahead)."""
    starts = tokens[:, 0].astype(np.int64)
    decided = int(np.searchsorted(starts, cut - 15))                     # tokens that start before cut - 15
    if decided and starts[decided - 1] + tokens[decided - 1, 2] > cut:
        return ("open", (cut - int(starts[decided - 1]) - 8) % 15)
    return ("bit0", int(tokens[decided, 3]) % 8, cut - int(starts[decided]))


def test_coverage_g_piece_cuts():
    _, each = walked(256, ("G",))
    for name, least in (("G-short-pieces", SHORT_PIECE), ("G-long-pieces", LONG_PIECE)):
        tokens = each[name][3]
        n = int(tokens[-1, 0] + tokens[-1, 2])
        cuts = P.piece_cuts(tokens, n, least)
        residues, bit0s, past = set(), set(), set()
        for label, at in cuts.items():
            assert all(b - a >= least for a, b in zip([0] + at, at + [n])), (name, label)
            what = [_describe(tokens, x) for x in at]
            residues |= {w[1] for w in what if w[0] == "open"}
            bit0s |= {w[1] for w in what if w[0] == "bit0"}
            past |= {w[2] for w in what if w[0] == "bit0" and label.startswith("past-")}
        assert residues == set(range(15)) and bit0s == set(range(8)) and past >= set(range(1, 16)), (name, residues, bit0s, past)
        # one match open across three pieces: the middle one is nothing but nibbles
        assert [w[0] for w in (_describe(tokens, x) for x in cuts["open-across-three"])] == ["open"] * 3


# ---------------------------------------------------------------- the host codec, the reference, the sanitizers
def feed(data, cuts, simple, marker_separately=False):
    """``data`` through the incremental compressor in pieces cut at ``cuts``, room for everything in every call."""
    c, out, status = lzs.IncrementalCompressor(simple), bytearray(), 0
    room = api.compressed_max(len(data)) + 64
    pieces = [data[a:b] for a, b in zip([0] + list(cuts), list(cuts) + [len(data)])]
    for i, piece in enumerate(pieces):
        got, used, status = c.step(piece, room, i == len(pieces) - 1 and not marker_separately)
        assert used == len(piece)
        out += got
    for _ in range(2):
        if not status & api.STATUS_END_MARKER:
            got, _, status = c.step(b"", room, True)
            out += got
    assert status & api.STATUS_END_MARKER
    return bytes(out)


def test_host_codec_on_every_directed_input(monkeypatch):
    """lzs_compress() and the incremental compressors on the calling thread's own codec (LZS_ROUTE=host, csrc/lzs_hostcodec.c, whose
    hostcodec_compress_piece takes the contract of stream_compress_piece) get the same inputs for free."""
    monkeypatch.setenv("LZS_ROUTE", "host")
    _, each = walked(256)
    for i in inputs():
        want = O.compress(i.data)
        assert lzs.compress(i.data) == want, i.name
        for cap in (len(want) - 1, len(want) // 2):
            assert lzs.compress(i.data, cap) == want[:cap], (i.name, cap)
    for name, least, simple in (("G-short-pieces", SHORT_PIECE, True), ("G-long-pieces", LONG_PIECE, False)):
        data = next(i.data for i in inputs("G") if i.name == name)
        want = O.compress(data)
        for label, at in P.piece_cuts(each[name][3], len(data), least).items():
            assert feed(data, at, simple) == want, (name, label)
        assert feed(data, [], simple, marker_separately=True) == want, name


@pytest.mark.skipif(not oracle.have_ref(), reason="oracle/_ref/liblzs_ref.so was not built (needs the reference's sources)")
def test_oracle_compressor_is_the_reference_on_every_directed_input():
    ref = oracle.ref()
    for i in inputs():
        want = O.compress(i.data)
        assert ref.compress(i.data) == want, i.name
        for cap in sorted({1, len(want) // 3, len(want) - 2, len(want) - 1}):
            assert ref.compress(i.data, cap) == O.compress(i.data, cap) == want[:cap], (i.name, cap)


def test_the_standalone_sanitizer_program(tmp_path):
    """oracle/compress_segments_san.c: the model under AddressSanitizer and UndefinedBehaviorSanitizer in a program of its own (no
    runtime is preloaded into anything) on every directed input, at both segment sizes."""
    exe, blob = tmp_path / "compress_segments_san", tmp_path / "inputs.bin"
    with open(blob, "wb") as f:
        for i in inputs():
            f.write(len(i.data).to_bytes(4, "little") + i.data)
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "san-program", f"SAN_COMPRESS_PROGRAM={exe}",
                    f"SAN_PROGRAM={tmp_path / 'channel_encode_san'}", f"SAN_SCAN_PROGRAM={tmp_path / 'scan_segments_san'}"],
                   check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "0 failure(s)" in r.stdout and f"{len(inputs())} input(s)" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
