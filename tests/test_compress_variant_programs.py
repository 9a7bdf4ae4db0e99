"""No device: the contents of tests/compress_variant_programs.py are what their builders say, for every table shape of the
compress kernel -- the oracle's parse takes the named token at the named position, the chain model finds the answer where the
builder put it (last inside the window, behind enough candidates of other grams), the shapes' constants are the source's, and the
default shape's contents are those of tests/test_gpu_search_hop_end.py byte for byte.  tests/test_gpu_compress_variants.py then
runs these contents through each variant on the device.
"""
import os
import re

import numpy as np
import pytest

import oracle
import compress_variant_programs as P

O = oracle.oracle()
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lzs_compression_amd", "csrc")
LONGEST_CLOSED_TOKEN = 67              # 8 bytes + kExtMax: a longer token was an open match, which thins the chains behind it


def _trace(data: bytes):
    return [(int(p), int(off), int(ln)) for p, off, ln in O.trace(data)]


def _token_at(trace, pos):
    """(offset, length) of the token that STARTS at pos (offset 0: a literal); None if the parse steps over pos."""
    for p, off, ln in trace:
        if p == pos:
            return off, ln
        if p > pos:
            break
    return None


@pytest.mark.parametrize("shape", list(P.SHAPES))
def test_the_builders_build_what_they_say(shape):
    """Expected tokens (the oracle's trace) and reach (the chain model), for every content of the shape."""
    S = P.SHAPES[shape]
    for name, built in P.contents(shape).items():
        trace = _trace(built.data)
        for at in built.at:
            assert _token_at(trace, at.p) == at.token, (shape, name, at)
            longest = max((ln for p, _, ln in trace if p < at.p), default=0)
            assert longest <= LONGEST_CLOSED_TOKEN, (shape, name, at.p, longest)
            if at.which is None:
                continue
            ch = P.chain(built.data, at.p, S, at.which)
            mine = built.data[at.p:at.p + at.which]
            if at.answer:
                assert at.p - at.answer in ch, (shape, name, at)
                assert built.data[at.p - at.answer:at.p - at.answer + at.which] == mine
            if at.last:
                assert ch[-1] == at.p - at.answer, (shape, name, at, ch[-1])
            behind = at.p - at.answer if at.answer else -1          # (no answer on this chain: all of it is walked)
            others = [q for q in ch if q > behind and built.data[q:q + at.which] != mine]
            assert len(others) >= at.others, (shape, name, at, len(others))
    # the hops of a pass run out before the farthest candidate: a full step lands on a collision
    for name in ("3-gram at 2047", "3-gram at 2048", "12 bytes at 2047", "12 bytes at 2048"):
        at = P.contents(shape)[name].at[0]
        assert at.which == P.walked(S) and at.others >= S.hops_last + 2, (shape, name)
    assert (2047, 3) == P.contents(shape)["3-gram at 2047"].at[0].token
    assert P.contents(shape)["3-gram at 2048"].at[0].token[0] != 2048
    assert ("rejectable chain, 2-gram" in P.contents(shape)) == (not S.no3)


@pytest.mark.parametrize("shape", list(P.SHAPES))
def test_the_ladder_stands_on_the_chain_the_shape_walks(shape):
    """Nearest first: the candidates of 2 .. 12 bytes (from 3 with a 3-byte chain), then the twelfth, as long as the eleventh."""
    S = P.SHAPES[shape]
    data, p = P.contents(shape)["ladder"].data, P.LADDER_P
    which = P.walked(S)
    mine = data[p:p + which]
    same = [q for q in P.chain(data, p, S, which) if data[q:q + which] == mine]
    want = [p - 100 - P.LADDER_STEP * k for k in range(12)][which - 2:]
    assert same == want
    lcp = [next(i for i in range(14) if data[q + i] != data[p + i]) for q in want]
    assert lcp == list(range(which, 13)) + [12]


@pytest.mark.parametrize("shape", list(P.SHAPES))
def test_the_pool_border_walkers_stand_on_the_chain_the_shape_walks(shape):
    S = P.SHAPES[shape]
    data = P.contents(shape)["pool border"].data
    which = P.walked(S)
    for j, p in enumerate(P.BORDER_WALKERS):
        mine = data[p:p + which]
        same = [q for q in P.chain(data, p, S, which) if data[q:q + which] == mine]
        assert same == [1500 - 140 * k - 20 * j for k in range(10)], (shape, p)


@pytest.mark.parametrize("shape", list(P.SHAPES))
def test_the_lone_grams_are_alone_on_their_chains(shape):
    """The first link of the walk is the reach itself at 2047 (and the chains are empty inside the window at 2048); a lone 2-gram
    under a shape with a 3-byte chain finds that chain empty."""
    S = P.SHAPES[shape]
    for n in (3, 2):
        for dist in (2047, 2048):
            data = P.contents(shape)[f"lone {n}-gram at {dist}"].data
            assert P.lone_chains(S, data, 1 + dist) == P.lone_chains_wanted(S, dist, n), (shape, n, dist)


def test_the_collisions_are_collisions():
    for S in P.SHAPES.values():
        for h in P.grams_in_bucket2(S, P.G, 8):
            assert S.bucket2(h) == S.bucket2(P.G) and h != P.G[:2]
        if not S.no3:
            for h in P.grams_in_bucket3(S, P.G, 3, True) + P.grams_in_bucket3(S, P.G, 7, False):
                assert S.bucket3(h) == S.bucket3(P.G) and h != P.G


def test_the_seeds_are_seeds():
    """At the token start the byte before and the run - 1 bytes from p are one value: len1 = run - 1, capped at 12."""
    for name, run in (("seed 2 at a token start", 3), ("seed 5 at a token start", 6), ("seed 11 at a token start", 12),
                      ("seed capped at a token start", 20)):
        d, p = P.contents("text")[name].data, P.SEED_P
        assert len(set(d[p - 1:p + run - 1])) == 1 and d[p + run - 1] != d[p]


# ------------------------------------------------------------------------------------------------ constants
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^#define %s\s+(0[xX][0-9A-Fa-f]+|\d+)u?\b" % re.escape(name), text, re.M)
    return int(m.group(1), 0) if m else None


def _namespace(text, name):
    m = re.search(r"^namespace %s \{.*?^\}" % re.escape(name), text, re.M | re.S)
    assert m, name
    return m.group(0)


def test_the_shapes_are_the_sources():
    """A retune of a variant's tables or pass shape fails HERE instead of silently emptying the builders."""
    wg, hip, text_shape = _source("kernels/compress_wg.inc"), _source("lzs_kernels.hip"), _source("kernels/wgv_text_shape.inc")
    default = {k: _define(wg, "LZS_" + k) for k in ("HASH3_MUL", "HASH2_MUL", "WG_HEAD3", "WG_HEAD2", "HOPS", "SUBSTEPS")}
    assert None not in default.values(), default
    assert "kWgHead2 == 4096 ? 4 : kWgHead2 == 2048 ? 5 : kWgHead2 == 1024 ? 6 : kWgHead2 == 512 ? 7 : 8" in wg
    for S in P.SHAPES.values():
        ns = _namespace(hip, "wgv_" + S.name)
        own = ns + (text_shape if "wgv_text_shape.inc" in ns else "")
        own = own.replace("LZS_EXP_TEXT_HEAD3", str(_define(text_shape, "LZS_EXP_TEXT_HEAD3")))
        own = own.replace("LZS_EXP_TEXT_HEAD2", str(_define(text_shape, "LZS_EXP_TEXT_HEAD2")))

        def value(wgv, fallback):
            v = _define(own, "LZS_WGV_" + wgv)
            return default[fallback] if v is None else v

        assert S.no3 == (_define(own, "LZS_WGV_NO3") == 1), S.name
        if not S.no3:
            assert (S.hash3_mul, S.head3) == (value("HASH3_MUL", "HASH3_MUL"), value("HEAD3", "WG_HEAD3")), S.name
        assert (S.hash2_mul, S.head2) == (value("HASH2_MUL", "HASH2_MUL"), value("HEAD2", "WG_HEAD2")), S.name
        assert S.head2_shift == P.head2_shift(S.head2), S.name
        hops = value("HOPS", "HOPS")
        hops_last = _define(own, "LZS_WGV_HOPS_LAST")
        assert (S.hops, S.substeps) == (hops, value("SUBSTEPS", "SUBSTEPS")), S.name
        assert S.hops_last == (hops if hops_last is None else hops_last), S.name
        assert (hops_last is not None) <= (_define(own, "LZS_WGV_HOP_END") == 1), S.name
        assert (S.name == "safe") == (_define(own, "LZS_WGV_CHAIN_SAFE") == 1)
    aux = _source("kernels/compress_aux.inc")
    assert "kClassFewMax = %d, kClassManyMin = %d;" % (P.CLASS_FEW_MAX, P.CLASS_MANY_MIN) in aux
    assert "* 40503u) >> 4) & 4095u" in aux and "if (n >= 2049u)" in aux


def test_the_default_shape_gives_the_contents_of_the_hop_end_test():
    import test_gpu_search_hop_end as H
    assert (H.HASH3_MUL, H.HEAD3, H.HASH2_MUL, H.HEAD2, H.HEAD2_SHIFT) == P.DEFAULT[1:6]
    mine = P.contents(P.DEFAULT.name)
    both = [name for name in H.CONTENTS if name in mine]
    assert both == list(H.CONTENTS)
    for name in both:
        assert mine[name].data == H.CONTENTS[name](), name


# ------------------------------------------------------------------------------------------------ class changes
@pytest.mark.parametrize("name", list(P.CLASS_CHANGES))
def test_class_change_blocks(name):
    """The first 2100 bytes give the class they were built for (at every length the device test cuts to that the classifier looks
    at), the block is at most 40 KiB, holds an open match (a token longer than 4080 bytes), and ends in 600 literals in a row."""
    cls, _, first = P.CLASS_CHANGES[name]
    data = P.class_change(name)
    assert len(data) <= 40 * 1024
    for n in (len(data),) + P.CLASS_CHANGE_LENGTHS:
        assert P.classify(data[:n]) == (cls if n >= 2049 else 1), (name, n)
    trace = _trace(data)
    assert max(ln for _, _, ln in trace) > 4080
    at = P.literals_at(name)
    tail = [t for t in trace if t[0] >= at]
    assert tail == [(at + i, 0, 1) for i in range(P.LITERALS)], name
    # what follows the horizon is of another class than what leads
    follow = data[P.HORIZON:P.HORIZON + 2100]
    assert P.classify(follow) == {"text": 1, "run": 2, "random": 3}[first] != cls


def test_six_ordered_pairs_of_leading_class_and_first_follow_up():
    kind = {"text": 1, "run": 2, "random": 3}
    pairs = {(cls, kind[first]) for cls, _, first in P.CLASS_CHANGES.values()}
    assert pairs == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3) if a != b}
