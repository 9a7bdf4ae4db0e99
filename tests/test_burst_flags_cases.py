"""The generated queues of flagged packets (tests/burst_flags_cases.py) on the CPU: the rule's loop against the header's
rank-by-rank definition, written a second time with M.run_model and plain calls of the compressor model; and conditions on the
inputs of tests/test_gpu_burst_flags_queues.py -- what the queues reach, by the run borders and the models alone -- so that a later
change to the generator cannot silently empty a case."""
import numpy as np
import pytest

from lzs_compression_amd import api as A

import burst_flags_cases as C
import test_channel_model as M
from test_channel_model import O

QUEUES = [(p, d) for p in C.PATTERNS for d in C.DENSITIES]


def _ranks(ids):
    """[the entries of rank k, ascending], rank k being the k-th packet of every channel."""
    seen, ranks = {}, []
    for b, c in enumerate(ids):
        k = seen.get(c, 0)
        seen[c] = k + 1
        if k == len(ranks):
            ranks.append([])
        ranks[k].append(b)
    return ranks


def _reset_rank(rank, form, nch, hists):
    """Before the call of a rank: hist_len = 0 for every packet of it that is flagged, in range and a block."""
    for b in rank:
        if form.flags[b] & 1 and 0 <= form.ids[b] < nch and b not in form.skip:
            hists[form.ids[b]] = b""
    return [b for b in rank if 0 <= form.ids[b] < nch and b not in form.skip]


def _decode_by_ranks(form, nch, hists, cap):
    hists = list(hists)
    outs, status, touched = [b""] * form.n, np.full(form.n, A.STATUS_ERROR, dtype=np.uint8), set()
    for rank in _ranks(form.ids):
        call = _reset_rank(rank, form, nch, hists)
        m = M.run_model([form.coded[b] for b in call], [form.ids[b] for b in call], hists, cap)
        hists = m.hists
        for k, b in enumerate(call):
            outs[b], status[b] = m.outs[k], m.status[k]
            if m.before[k] is not None:
                touched.add(form.ids[b])
    return outs, status, hists, touched


def _compress_by_ranks(form, nch, hists, cap):
    hists = list(hists)
    outs, status, touched = [b""] * form.n, np.full(form.n, A.STATUS_ERROR, dtype=np.uint8), set()
    for rank in _ranks(form.ids):
        for b in _reset_rank(rank, form, nch, hists):
            c = form.ids[b]
            if hists[c] is None:
                continue
            outs[b], _, status[b], hists[c] = O.compress_channel(hists[c], form.plain[b], min(cap, A.compressed_max(len(form.plain[b]))))
            touched.add(c)
    return outs, status, hists, touched


@pytest.mark.parametrize("pattern,density", QUEUES)
def test_the_rule_equals_its_rank_by_rank_definition(pattern, density):
    """Every output, status and final history, of the decoder at a roomy capacity and at one that cuts, and of the compressor."""
    q = C.queue(pattern, density)
    for form in q.forms():
        for cap in (1 << 20, 20):
            got = C._apply_rule(C.decode_step(form.coded, [cap] * form.n), form.ids, form.flags, q.hists, form.skip)
            want = _decode_by_ranks(form, q.nch, q.hists, cap)
            assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2] and got[3] == want[3], (form.packed, cap)
            rooms = [min(cap, A.compressed_max(len(p))) for p in form.plain]
            got = C._apply_rule(C.compress_step(form.plain, rooms), form.ids, form.flags, q.hists, form.skip)
            want = _compress_by_ranks(form, q.nch, q.hists, cap)
            assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2] and got[3] == want[3], (form.packed, cap)


def test_the_queues_reach_every_edge():
    """Conditions on the inputs of the GPU tests.  `pairs` has 300 and more channels whose last run is staged and uses the last or
    the last but one of its n // 2 staging slots with n odd; n = 2 and n = 3 use theirs; every count of the report is reached
    somewhere; and in every queue with a flag behind a channel's first packet the compressor model tells at least half of those
    flags from none -- the decoder model half of those whose packet begins with a copy from in front of itself."""
    total = {}
    for pattern, density in QUEUES:
        q = C.queue(pattern, density)
        for form in q.forms():
            r = C.reach(q, form)
            print(q.name, "packed" if form.packed else "strided", r)
            for k, v in r.items():
                total[k] = max(total.get(k, 0), v)
            assert 2 * r["told_compress"] >= r["flagged_later"], (q.name, r)
            assert 2 * r["told_decode"] >= r["reach_back_later"], (q.name, r)
            assert r["top_slot"] < r["n"] // 2, (q.name, r)
            flag_bytes = set(form.flags)
            if form.n > 3:
                assert any(f & 1 and f >> 1 for f in flag_bytes), "no flagged byte with upper bits"
                assert density in ("all",) or any(not f & 1 and f >> 1 for f in flag_bytes), "no unflagged byte with upper bits"
        assert pattern != "tiny" or max(len(p) for p in q.plain) <= 40
    assert all(v > 0 for v in total.values()), total
    best = {}
    for density in C.DENSITIES:
        q = C.queue("pairs", density)
        r = C.reach(q, q.strided)
        assert r["n"] % 2 == 1 and r["runs1"] + r["runs2"] + r["runs3+"] >= 400, r
        for k, v in r.items():
            best[k] = max(best.get(k, 0), v)
        if r["top_slot"] in (r["n"] // 2 - 1, r["n"] // 2 - 2):
            best["last_slot"] = True
    assert best["staged"] >= 300 and best.get("last_slot"), best
    two, three = C.queue("two", "sparse"), C.queue("three", "all")
    assert two.strided.n == 2 and C.reach(two, two.strided)["top_slot"] == 0 and two.flags[1] & 1
    assert three.strided.n == 3 and C.reach(three, three.strided)["top_slot"] == 0


def test_a_window_of_tiny_packets_would_reach_across_a_reset():
    """In a `tiny` queue: a flagged packet and, further on in the run it starts, a packet with fewer than 2047 bytes between them and
    dozens of packets: its window would reach across the reset.  The model shows it: with that one flag cleared the later packet is
    coded differently."""
    q = C.queue("tiny", "sparse")
    form = q.strided
    rooms = [A.compressed_max(len(p)) for p in form.plain]
    outs = C._apply_rule(C.compress_step(form.plain, rooms), form.ids, form.flags, q.hists)[0]
    shown = 0
    for run in form.runs(q.nch):
        if not run.fresh or run.key >= q.nch or len(run.packets) < 8:
            continue
        first, far = run.packets[0], run.packets[7:]                 # (seven packets and more behind the reset)
        between = sum(len(form.plain[b]) for b in run.packets[:-1])
        if between >= M.WINDOW or first == min(b for b in range(form.n) if form.ids[b] == run.key):
            continue
        cleared = list(form.flags)
        cleared[first] &= 0xFE
        other = C._apply_rule(C.compress_step(form.plain, rooms), form.ids, cleared, q.hists)[0]
        changed = [b for b in far if other[b] != outs[b]]
        print("channel", run.key, "reset at", first, "packets behind it", len(run.packets) - 1, "coded differently without it", len(changed))
        shown += bool(changed)
    assert shown >= 4, shown
    # and one window spans 50 packets and more
    spans = []
    for c in range(q.nch):
        lens = [len(form.plain[b]) for b in range(form.n) if form.ids[b] == c]
        k, s = 0, 0
        while k < len(lens) and s + lens[-1 - k] <= M.WINDOW:
            s += lens[-1 - k]
            k += 1
        spans.append(k)
    assert max(spans) >= 50, spans
