"""Every form of the eight-streams-per-wavefront decoder (lzs_decompress_blocks_grp: TWO, WIDE, plain) on
every directed stream of tests/block_decoder_programs.py, through every entry that instantiates the template: each stream is put
into each form by the rows composed around it, decoded whole and at each of its cut capacities, and its length and bytes -- for the
channel entries its status and final slot too -- must be the plain CPU model's.  Outputs are prefilled with 0xA5: the strided block
call may write nothing past the capacity, every other call nothing past the length.  What the streams reach and that the composer
yields the forms is proven without a device in tests/test_block_decoder_programs.py; every test here ends by asserting that the
(family, form) pairs it ran are the full product.  A failure names the entry, the family, the form, the stream and the capacity.
"""
import functools
import time

import numpy as np
import pytest

import lzs_compression_amd as lzs
import block_decoder_programs as P

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_channel_model as M  # noqa: E402
from test_channel_model import O  # noqa: E402
import test_gpu_channel_model as G  # noqa: E402

FILL, GUARD = G.FILL, G.GUARD
PACKED_WAVES_A_LAUNCH = 2048
SLOTS7 = M.start_slots(np.random.default_rng(43), len(M.HIST_LENS))     # histories of 0, 1, 5, 127, 128, 2046 and 2047 bytes
SLOT_ROWS7 = G._slot_rows(SLOTS7)


@functools.lru_cache(maxsize=None)
def _block(name, cap):
    return O.decompress(P.by_name(name).data, cap)


@functools.lru_cache(maxsize=None)
def _packet(name, cap, h):
    """(bytes, status, new history) of the stream as a packet on history SLOTS7[h]."""
    return O.decompress_channel(SLOTS7[h], P.by_name(name).data, cap)


@functools.lru_cache(maxsize=None)
def _run(name, cap, h, packed):
    """[FILLER, stream, stream] as a run on history SLOTS7[h]: ([bytes], [status], final history).  The filler's room is its size
    in a packed call and the call's one capacity in a strided one."""
    return _run_model([P.FILLER, P.by_name(name).data, P.by_name(name).data], [P.FILLER_OUT if packed else cap, cap, cap], SLOTS7[h])


def _run_model(packets, caps, hist):
    m_outs, m_status = [], []
    for pk, cap in zip(packets, caps):
        m = M.run_model([pk], [0], [hist], cap)
        m_outs.append(m.outs[0])
        m_status.append(int(m.status[0]))
        hist = m.hists[0]
    return m_outs, m_status, hist


def _tag(entry, s, form, cap):
    return f"{entry}: family {s.family}, form {form}, stream {s.name} ({'; '.join(s.cases[:3])}), capacity {cap}"


def _diff(got, want):
    k = min(len(got), len(want))
    at = next((i for i in range(k) if got[i] != want[i]), k)
    return f"first differing byte {at}: {bytes(got[at:at + 8]).hex()} (model {bytes(want[at:at + 8]).hex()})"


def _report(entry, t0, launches, ran, families):
    print(f"{entry}: {launches} launches, {time.perf_counter() - t0:.2f} s")
    want = {(f, form) for f in families for form in P.FORMS}
    assert ran == want, sorted(want - ran)


def _upload_strided(placed, nrows):
    dev = torch.from_numpy(placed.flat).cuda()
    assert dev.data_ptr() % 64 == 0
    at = P.Placed.FRONT + placed.base
    return dev[at:at + nrows * placed.stride].view(nrows, placed.stride), torch.from_numpy(placed.lens).cuda()


def _slots(nch):
    return SLOT_ROWS7[np.arange(nch) % len(SLOTS7)].copy()


def _check_slots(tag_of, states, want_s):
    s = states.cpu().numpy()
    rows = np.nonzero((s != want_s).any(axis=1))[0]
    if rows.size:
        c = int(rows[0])
        i = int(np.nonzero(s[c] != want_s[c])[0][0])
        raise AssertionError(f"{tag_of(c)}: {rows.size} slots differ, first channel {c} at slot byte {i}: "
                             f"{s[c, i:i + 8].tobytes().hex()} (model {want_s[c, i:i + 8].tobytes().hex()})")


# ------------------------------------------------------------------------------------------------ the strided calls of eight rows
def _strided(entry):
    t0, ran, launches = time.perf_counter(), set(), 0
    for k, (cap, ws) in enumerate(sorted(P.strided_batches().items())):
        rows, tails = P.rows_and_tails(ws)
        nrows = len(rows)
        x, xl = _upload_strided(P.place_strided(rows, tails, base=k % 4), nrows)
        out = torch.full((nrows, (max(cap, 1) + 15) // 16 * 16 + GUARD), FILL, dtype=torch.uint8, device="cuda")
        states = st = None
        if entry == "R1":
            _, n = lzs.decompress_blocks(x, xl, cap, out=out)
        elif entry == "R3":
            before = _slots(nrows)
            states = torch.from_numpy(before).cuda()
            ids = None if k % 2 else torch.arange(nrows, dtype=torch.int32, device="cuda")
            _, n, st = lzs.decompress_channels(x, xl, ids, states, cap, out=out)
        else:
            n, st = lzs.decompressed_sizes(x, xl, limit=cap)
        torch.cuda.synchronize()
        launches += 1
        o, n = out.cpu().numpy(), n.cpu().numpy()
        want_n = np.zeros(nrows, dtype=np.int64)
        want_st = np.array([P.companion_result(r, cap) for r in rows], dtype=np.uint8)
        want = np.full(o.shape, FILL, dtype=np.uint8)
        if entry == "R1":
            want[:, :cap] = o[:, :cap]                                 # (below the capacity only the stream's bytes are asked for)
        want_s = None if states is None else before
        for wi, w in enumerate(ws):
            r = P.LANES * wi + w.pos
            if entry == "R3":
                e, want_st[r], hist = _packet(w.stream.name, cap, r % len(SLOTS7))
                want_s[r] = G._slot_rows([hist])[0]
            else:
                e, want_st[r], _ = _packet(w.stream.name, cap, 0)
                assert entry != "R1" or e == _block(w.stream.name, cap)
            want_n[r] = len(e)
            if entry != "sizes":
                want[r, :len(e)] = np.frombuffer(e, dtype=np.uint8)
                want[r, len(e):cap] = o[r, len(e):cap] if entry == "R1" else FILL
        wrong = (n != want_n) | (o != want).any(axis=1)
        if st is not None:
            wrong |= st.cpu().numpy() != want_st
        bad = np.nonzero(wrong)[0]
        if bad.size:
            r = int(bad[0])
            w = ws[r // P.LANES]
            who = "the stream under test" if r % P.LANES == w.pos else f"companion row {r % P.LANES} ({len(rows[r])} bytes)"
            past = np.nonzero(o[r, max(cap if entry == "R1" else int(want_n[r]), 0):] != FILL)[0]
            raise AssertionError(f"{_tag(entry, w.stream, w.form, cap)}, group position {w.pos}, {who} ({bad.size} rows differ): length "
                                 f"{int(n[r])} (model {int(want_n[r])})" + (f", status {int(st[r]):#x} (model {int(want_st[r]):#x})" if st is not None else "")
                                 + ", " + _diff(o[r, :int(want_n[r])], want[r, :int(want_n[r])])
                                 + (f"; a byte past the {'capacity' if entry == 'R1' else 'length'} was written" if past.size else ""))
        if states is not None:
            _check_slots(lambda c: _tag(entry, ws[c // P.LANES].stream, ws[c // P.LANES].form, cap), states, want_s)
        ran |= {(w.stream.family, w.form) for w in ws}
    _report(entry, t0, launches, ran, P.FAMILIES)


def test_r1_decompress_blocks():
    """lzs.decompress_blocks, the device-pointer call: lzs_decompress_blocks_grp_kernel<false>, the three plain-entry forms."""
    _strided("R1")


def test_r3_decompress_channels():
    """lzs.decompress_channels: the CHAN forms; every stream on histories of 0 .. 2047 bytes in turn, status and final slot too."""
    _strided("R3")


def test_decoded_sizes_on_the_same_rows():
    """lzs.decompressed_sizes(limit=capacity) on the rows of R1: size and status are the model's on an empty history."""
    _strided("sizes")


# ------------------------------------------------------------------------------------------------ the packed calls of eight rows
def _packed(entry):
    t0, ran, launches = time.perf_counter(), set(), 0
    every = P.waves(True)
    for k in range(0, len(every), PACKED_WAVES_A_LAUNCH):
        ws = every[k:k + PACKED_WAVES_A_LAUNCH]
        rows, tails = P.rows_and_tails(ws)
        nrows = len(rows)
        placed = P.place_packed(rows, tails)
        data = torch.from_numpy(placed.flat).cuda()
        in_off = torch.from_numpy(placed.offsets + P.Placed.FRONT).cuda()
        in_len = torch.from_numpy(placed.lens).cuda()
        rooms = np.array([room for w in ws for room in w.rooms], dtype=np.int64)
        off = np.concatenate(([0], np.cumsum(rooms))) + 3              # (the first output byte off every boundary)
        out = torch.full((int(off[-1]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        out_off = torch.from_numpy(off).cuda()
        states = st = None
        if entry == "R2":
            _, n = lzs.decompress_packed(data, in_off, out, out_off, in_len=in_len)
        else:
            before = _slots(nrows)
            states = torch.from_numpy(before).cuda()
            ids = None if (k // PACKED_WAVES_A_LAUNCH) % 2 else torch.arange(nrows, dtype=torch.int32, device="cuda")
            _, n, st = lzs.decompress_channels_packed(data, in_off, ids, states, out, out_off, in_len=in_len)
        torch.cuda.synchronize()
        launches += 1
        o, n = out.cpu().numpy(), n.cpu().numpy()
        want_n = np.zeros(nrows, dtype=np.int64)
        want_st = np.array([P.companion_result(r, room) for r, room in zip(rows, rooms)], dtype=np.uint8)
        want = np.full(o.shape, FILL, dtype=np.uint8)
        want_s = None if states is None else before
        for wi, w in enumerate(ws):
            r = P.LANES * wi + w.pos
            if entry == "R4":
                e, want_st[r], hist = _packet(w.stream.name, w.cap, r % len(SLOTS7))
                want_s[r] = G._slot_rows([hist])[0]
            else:
                e = _block(w.stream.name, w.cap)
            want_n[r] = len(e)
            want[off[r]:off[r] + len(e)] = np.frombuffer(e, dtype=np.uint8)
        wrong = n != want_n
        if st is not None:
            wrong |= st.cpu().numpy() != want_st
        if (o != want).any():
            first = int(np.nonzero(o != want)[0][0])
            wrong[max(int(np.searchsorted(off, first, side="right")) - 1, 0)] = True
        bad = np.nonzero(wrong)[0]
        if bad.size:
            r = int(bad[0])
            w = ws[r // P.LANES]
            who = "the stream under test" if r % P.LANES == w.pos else f"companion row {r % P.LANES} ({len(rows[r])} bytes, room {rooms[r]})"
            lo, end = int(off[r]), int(off[r]) + int(want_n[r])
            past = np.nonzero(o[end:int(off[r + 1])] != FILL)[0]
            raise AssertionError(f"{_tag(entry, w.stream, w.form, w.cap)}, group position {w.pos}, {who} ({bad.size} rows differ): length "
                                 f"{int(n[r])} (model {int(want_n[r])})" + (f", status {int(st[r]):#x} (model {int(want_st[r]):#x})" if st is not None else "")
                                 + ", " + _diff(o[lo:end], want[lo:end]) + ("; a byte past the length was written" if past.size else ""))
        if states is not None:
            _check_slots(lambda c: _tag(entry, ws[c // P.LANES].stream, ws[c // P.LANES].form, ws[c // P.LANES].cap), states, want_s)
        ran |= {(w.stream.family, w.form) for w in ws}
    _report(entry, t0, launches, ran, P.FAMILIES)


def test_r2_decompress_packed():
    """lzs.decompress_packed: the PACKED forms, each stream's room its capacity, the companions' rooms from the composer."""
    _packed("R2")


def test_r4_decompress_channels_packed():
    """lzs.decompress_channels_packed: the PACKED + CHAN forms."""
    _packed("R4")


# ------------------------------------------------------------------------------------------------ the burst calls: runs
def _bursts(entry):
    packed = entry == "R6"
    t0, ran, launches = time.perf_counter(), set(), 0
    calls, _ = P.run_calls(packed)
    most = max(len(c.packets) for c in calls)
    work_all = torch.full((lzs.channels_burst_work_bytes(most, P.LANES),), FILL, dtype=torch.uint8, device="cuda")
    for k, c in enumerate(calls):
        npk, nch = len(c.packets), max(c.ids) + 1
        tails = [P.NOISE[7 + b % 50:7 + b % 50 + P.TAIL_BYTES] for b in range(npk)]
        ids = torch.tensor(c.ids, dtype=torch.int32, device="cuda")
        before = _slots(nch)
        states = torch.from_numpy(before).cuda()
        work = work_all[:lzs.channels_burst_work_bytes(npk, nch)]      # (the run decoder's size: no split)
        if packed:
            placed = P.place_packed(c.packets, tails)
            data = torch.from_numpy(placed.flat).cuda()
            in_off = torch.from_numpy(placed.offsets + P.Placed.FRONT).cuda()
            rooms = np.array(c.rooms, dtype=np.int64)
            off = np.concatenate(([0], np.cumsum(rooms))) + 5
            out = torch.full((int(off[-1]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            _, n, st = lzs.decompress_channels_burst_packed(data, in_off, ids, states, out, torch.from_numpy(off).cuda(),
                                                            in_len=torch.from_numpy(placed.lens).cuda(), work=work)
        else:
            rooms = np.full(npk, c.cap, dtype=np.int64)
            x, xl = _upload_strided(P.place_strided(c.packets, tails, base=k % 4), npk)
            width = (max(c.cap, 1) + 15) // 16 * 16 + GUARD
            off = np.arange(npk + 1, dtype=np.int64) * width
            out = torch.full((npk, width), FILL, dtype=torch.uint8, device="cuda")
            _, n, st = lzs.decompress_channels_burst(x, xl, ids, states, c.cap, out=out, work=work)
        torch.cuda.synchronize()
        launches += 1
        o, n, st = out.cpu().numpy().reshape(-1), n.cpu().numpy(), st.cpu().numpy()
        want = np.full(o.shape, FILL, dtype=np.uint8)
        want_n = np.zeros(npk, dtype=np.int64)
        want_st = np.array([P.companion_result(pk, room) for pk, room in zip(c.packets, rooms)], dtype=np.uint8)
        want_s = before
        for ch, (s, where, cap) in enumerate(zip(c.streams, c.under_test, c.caps)):
            outs, status, hist = _run(s.name, cap, ch % len(SLOTS7), packed)
            for b, e, code in zip(where, outs, status):
                want_n[b], want_st[b] = len(e), code
                want[off[b]:off[b] + len(e)] = np.frombuffer(e, dtype=np.uint8)
            want_s[ch] = G._slot_rows([hist])[0]
        wrong = (n != want_n) | (st != want_st)
        if (o != want).any():
            first = int(np.nonzero(o != want)[0][0])
            wrong[min(max(int(np.searchsorted(off, first, side="right")) - 1, 0), npk - 1)] = True
        bad = np.nonzero(wrong)[0]
        if bad.size:
            b = int(bad[0])
            ch = c.ids[b]
            lo, end = int(off[b]), int(off[b]) + int(want_n[b])
            if ch < len(c.streams):
                s, cap = c.streams[ch], c.caps[ch]
                which = ("the filler", "the stream, first time", "the stream, second time")[c.under_test[ch].index(b)]
                detail = (G._explain(_tag(entry, s, c.form, cap) + f", {which}", b, ch, c.packets[b], SLOTS7[ch % len(SLOTS7)], int(rooms[b]),
                                     o[lo:int(off[b + 1])], n[b], st[b]) if which == "the filler" else
                          _tag(entry, s, c.form, cap) + f", {which} (packet {b} of {npk}, {len(c.streams)} runs under test): length {int(n[b])} "
                          f"(model {int(want_n[b])}), status {int(st[b]):#x} (model {int(want_st[b]):#x}), " + _diff(o[lo:end], want[lo:end]))
            else:
                s = c.streams[0]
                detail = (_tag(entry, s, c.form, c.caps[0]) + f": companion packet {b} ({len(c.packets[b])} bytes): length {int(n[b])}, "
                          f"status {int(st[b]):#x} (model {int(want_st[b]):#x})")
            past = np.nonzero(o[end:int(off[b + 1])] != FILL)[0]
            raise AssertionError(detail + ("; a byte past the length was written" if past.size else ""))
        _check_slots(lambda ch: _tag(entry, c.streams[min(ch, len(c.streams) - 1)], c.form, c.caps[min(ch, len(c.streams) - 1)]), states, want_s)
        ran |= {(s.family, c.form) for s in c.streams}
    _report(entry, t0, launches, ran, P.FAMILIES)


def test_r5_decompress_channels_burst():
    """lzs.decompress_channels_burst with the run decoder's work area: the CHAN + RUN forms.  A call is at most eight runs, so one
    wavefront: up to seven runs [filler, stream, stream] under test -- the second copy of the stream reads the first's output as
    its history -- and the companions' run."""
    _bursts("R5")


def test_r6_decompress_channels_burst_packed():
    """lzs.decompress_channels_burst_packed: the RUN + PACKED forms, the same runs with rooms."""
    _bursts("R6")


# ------------------------------------------------------------------------------------------------ the file rule, one wavefront
R7_FAMILIES = "ABEI"


def test_r7_decompress_concat_one_wavefront(monkeypatch):
    """lzs.decompress_concat on one wavefront (LZS_ONE_WAVE=1): lzs_decompress_blocks_grp_kernel<true>, the CONCAT forms -- the
    reference that test_file_rule_against_one_wavefront compares the many-wavefront route to.  One stream a call, so the capacity
    alone picks the form: every stream of families I, A, B and E in every form, whole where that form has a capacity that holds
    all of the output, cut otherwise; the bytes are the replay of the model's trace under the file rule."""
    monkeypatch.setenv("LZS_ONE_WAVE", "1")
    monkeypatch.setenv("LZS_ROUTE", "device")
    t0, ran, launches, whole_runs = time.perf_counter(), set(), 0, 0
    for s in P.by_family(*R7_FAMILIES):
        for form, (cap, whole) in P.concat_plan(s).items():
            want = P.replay(s.data, cap)
            got = lzs.decompress_concat(s.data, cap)
            launches += 1
            whole_runs += whole
            assert len(got) == len(want) and got == want, \
                f"{_tag('R7', s, form, cap)} ({'whole' if whole else 'cut'}): length {len(got)} (model {len(want)}), {_diff(got, want)}"
            ran.add((s.family, form))
    assert whole_runs > launches // 2
    _report("R7", t0, launches, ran, R7_FAMILIES)
