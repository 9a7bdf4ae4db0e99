"""The size query for long streams on the device: SCAN, the host's sums and lzs_size_finish_kernel, through the
Python calls, against the bit-by-bit model of tests/test_decoded_size_host.py, against the lane-per-stream query
(lzs_decompressed_size_batch_device) and against the decoders themselves.

The streams are the directed ones of tests/stream_border_programs.py -- a designed case at every segment border, among them the
walks that never fall in step (zeros, the de Bruijn literals, the locked stream) and the phantom end markers, the shapes at which
the rounds and the rule "an end is believed only from a settled walk" can go wrong -- in segments of 256 and 512 bytes, at the
limits of tests/size_stream_cases.py; then workload blocks at the default segment size, and the callers that ask before they
decode."""
import os
import subprocess

import numpy as np
import pytest

import stream_border_programs as P
import size_stream_cases as C
import lzs_compression_amd as lzs

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
O = C.O
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NONE32 = 0xFFFFFFFF


@pytest.fixture
def device(monkeypatch):
    monkeypatch.setenv("LZS_ROUTE", "device")
    monkeypatch.setenv("LZS_FORCE_STREAM", "1")
    return monkeypatch


@pytest.fixture(params=C.SEGS)
def seg(request, device):
    device.setenv("LZS_DEC_SEG", str(request.param))
    return request.param


_lane, _answers = {}, {}


def lane_queries(seg):
    """(size, status) of the lane-per-stream query -- the parent's kernel, not code under test -- for every directed stream at
    every limit of this segment size.  The limits all streams share go as one batch each; the others are one lane a call, so
    those calls go out over four streams and are waited for once."""
    all_streams = P.directed_streams()
    todo = [(s.name, min(limit, NONE32)) for s in all_streams for limit in C.limits(s, seg)]
    todo = [(name, limit) for name, limit in dict.fromkeys(todo) if (name, limit) not in _lane]
    shared = [limit for limit in (0, 1, NONE32) if all((s.name, limit) in todo for s in all_streams)]
    if shared:
        arr, lens = C.rows([s.data for s in all_streams])
        x, d_lens = torch.from_numpy(arr).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
        for limit in shared:
            size, status = lzs.decompressed_sizes(x, d_lens, limit)
            size, status = size.cpu().numpy().view(np.uint32), status.cpu().numpy()
            for b, s in enumerate(all_streams):
                _lane[(s.name, limit)] = (int(size[b]), int(status[b]))
    todo = [(C.by_name(name), limit) for name, limit in todo if (name, limit) not in _lane]
    if todo:
        streams = [torch.cuda.Stream() for _ in range(4)]
        size = torch.empty(len(todo), dtype=torch.int32, device="cuda")
        status = torch.empty(len(todo), dtype=torch.uint8, device="cuda")
        rows = {s.name: torch.from_numpy(np.frombuffer(s.data, dtype=np.uint8).copy()).cuda().view(1, -1) for s, _ in todo}
        torch.cuda.synchronize()
        for k, (s, limit) in enumerate(todo):
            lzs.decompressed_sizes(rows[s.name], None, limit, size=size[k:k + 1], status=status[k:k + 1], stream=streams[k % 4])
        torch.cuda.synchronize()
        size, status = size.cpu().numpy().view(np.uint32), status.cpu().numpy()
        for k, (s, limit) in enumerate(todo):
            _lane[(s.name, limit)] = (int(size[k]), int(status[k]))
    return _lane


def device_answers(seg, file_rule):
    """decompressed_size_stream of every directed stream at every limit, the input at byte offsets 0 to 3 of a larger tensor in
    turn: {(name, limit): (size, status)} under the plain rule (remembered: two tests ask), and a list under the file rule."""
    if not file_rule and seg in _answers:
        return _answers[seg]
    most = max(len(s.data) for s in P.directed_streams())
    bufs = [torch.empty(most + 8, dtype=torch.uint8, device="cuda") for _ in range(4)]
    plain, concat = {}, []
    for i, s in enumerate(P.directed_streams()):
        n = len(s.data)
        host = torch.from_numpy(np.frombuffer(s.data, dtype=np.uint8).copy())
        views = []
        for at in range(4):
            views.append(bufs[at][at:at + n])
            views[at].copy_(host)
        assert [v.data_ptr() % 4 for v in views] == [0, 1, 2, 3]
        for j, limit in enumerate(C.limits(s, seg)):
            if not file_rule:
                plain[(s.name, limit)] = lzs.decompressed_size_stream(views[(i + j) % 4], limit)
            elif s.file_rule:
                concat.append((s, limit, lzs.decompressed_size_stream(views[(i + j + 1) % 4], limit, concat=True)))
    assert lzs.decompressed_size_stream(bufs[1][1:1], None) == (0, 3)
    if file_rule:
        return concat
    _answers[seg] = plain
    return plain


def test_one_stream_in_device_memory(seg):
    """decompressed_size_stream at byte offsets 0 to 3 of a larger tensor: the model's (size, status)."""
    got = device_answers(seg, False)
    for s in P.directed_streams():
        for limit in C.limits(s, seg):
            assert got[(s.name, limit)] == C.expected(s, limit), (s.name, seg, limit, got[(s.name, limit)])


def test_one_stream_in_device_memory_under_the_file_rule(seg):
    """... and with concat the model's total cut at the limit, full or starved."""
    for s, limit, got in device_answers(seg, True):
        assert got == C.expected_file_rule(s, seg, limit), (s.name, seg, limit, got)


def test_one_stream_gives_what_the_lane_query_gives(seg):
    """(size, status) identical to lzs_decompressed_size_batch_device for the same bytes and limit."""
    got = device_answers(seg, False)
    lane = lane_queries(seg)
    for s in P.directed_streams():
        for limit in C.limits(s, seg):
            assert got[(s.name, limit)] == lane[(s.name, min(limit, NONE32))], (s.name, seg, limit, got[(s.name, limit)])


def test_one_stream_in_host_memory_and_the_decoders(seg):
    """decompressed_size: the model's (size, status), the length lzs_decompress gives at that capacity, and under the file rule
    the length lzs_decompress_concat gives."""
    for s in P.directed_streams():
        for limit in C.limits(s, seg):
            got = lzs.decompressed_size(s.data, limit)
            assert got == C.expected(s, limit), (s.name, seg, limit, got)
            assert len(lzs.decompress(s.data, min(limit, C.BIG))) == got[0], (s.name, seg, limit)
            if s.file_rule:
                got = lzs.decompressed_size(s.data, limit, concat=True)
                assert got == C.expected_file_rule(s, seg, limit), (s.name, seg, limit, got)
                assert len(lzs.decompress_concat(s.data, min(limit, C.BIG))) == got[0], (s.name, seg, limit)


@pytest.mark.parametrize("route", ["lanes", "segments"])
def test_all_streams_as_the_blocks_of_one_batch(seg, route, device, capfd):
    """decompressed_sizes_sync by either route: identical to the lane query and to the model, block by block."""
    datas = C.batch_blocks()
    arr, lens = C.rows(datas)
    x = torch.from_numpy(arr).cuda()
    d_lens = torch.from_numpy(lens.astype(np.int32)).cuda()
    device.setenv("LZS_SIZE_ROUTE", route)
    device.setenv("LZS_STREAM_DEBUG", "1")
    for limit in C.BATCH_LIMITS:
        capfd.readouterr()
        size, status = lzs.decompressed_sizes_sync(x, lens, limit)
        assert ("liblzs size query" in capfd.readouterr().err) == (route == "segments"), (route, limit)
        lane_size, lane_status = lzs.decompressed_sizes(x, d_lens, limit)
        lane_size = lane_size.cpu().numpy().view(np.uint32)
        lane_status = lane_status.cpu().numpy()
        for b, data in enumerate(datas):
            got = (int(size[b]), int(status[b]))
            assert got == (int(lane_size[b]), int(lane_status[b])), (seg, route, limit, b, got)
            assert got == C.model_of(data, limit), (seg, route, limit, b, got)


def _one_stream(cls, nbytes):
    x = lzs.workload.fill_device(cls, nbytes // 65536, 65536).view(-1)
    buf, n = lzs.compress_stream(x)
    return x, buf[:n]


@pytest.mark.parametrize("cls", ["text", "lowent", "random"])
def test_one_block_of_a_mebibyte_at_the_default_segment_size(cls):
    raw, stream = _one_stream(cls, 1 << 20)
    assert lzs.decompressed_size_stream(stream) == (1 << 20, lzs.STATUS_END_MARKER)
    assert lzs.decompressed_size_stream(stream, concat=True) == (1 << 20, 3)
    assert lzs.decompressed_size_stream(stream, 1 << 20) == (1 << 20, lzs.STATUS_END_MARKER)
    assert lzs.decompressed_size_stream(stream, (1 << 20) - 1) == ((1 << 20) - 1, lzs.STATUS_NO_OUTPUT_BUFFER_SPACE)
    half = stream[:stream.numel() // 2]
    want = len(O.decompress(half.cpu().numpy().tobytes(), 1 << 21))
    assert 0 < want < 1 << 20
    assert lzs.decompressed_size_stream(half) == (want, 3)
    assert lzs.decompressed_size(half.cpu().numpy().tobytes()) == (want, 3)


def test_a_batch_of_long_blocks_at_the_default_segment_size():
    """64 blocks of 256 KiB of text: long enough for the route by segments without forcing it."""
    x = lzs.workload.fill_device("text", 64, 262144)
    slots, lens = lzs.compress_blocks(x)
    h_lens = lens.cpu().numpy().astype(np.uint32)
    assert int(h_lens.sum()) // 64 >= 10167                            # lzs_plan_size_route's threshold
    lane_size, lane_status = lzs.decompressed_sizes(slots, lens)
    for limit in (None, 262144, 262143, 100_000):
        size, status = lzs.decompressed_sizes_sync(slots, h_lens, limit)
        lane_size, lane_status = lzs.decompressed_sizes(slots, lens, limit)
        assert (size == lane_size.cpu().numpy().view(np.uint32)).all() and (status == lane_status.cpu().numpy()).all(), limit
    size, status = lzs.decompressed_sizes_sync(slots, h_lens)
    assert (size == 262144).all() and (status == lzs.STATUS_END_MARKER).all()


def test_decoders_that_ask_first():
    """decompress_stream(x) and decompress(data) without a capacity return the input of a round trip."""
    raw, stream = _one_stream("text", 1 << 20)
    out, n = lzs.decompress_stream(stream)
    assert n == 1 << 20 and out.numel() == 1 << 20 and torch.equal(out, raw)
    data = stream.cpu().numpy().tobytes()
    want = raw.cpu().numpy().tobytes()
    assert lzs.decompress(data) == want
    assert lzs.decompress_concat(data + data) == want + want
    small = lzs.compress(b"hello hello hello hello")
    assert lzs.decompress(small) == b"hello hello hello hello"


def test_the_file_tool_decodes_once(tmp_path):
    """bin/lzs-decompress without an index on a low-entropy file (ratio 0.04: the guess 4 n + 4096 was too small twice): the
    file comes back, and LZS_STREAM_DEBUG shows one decode behind the size query."""
    raw = lzs.workload.fill("lowent", 16, 65536).tobytes()
    packed = lzs.compress(raw)
    assert 4096 < len(packed) and 4 * (4 * len(packed) + 4096) < len(raw)
    (tmp_path / "in.lzs").write_bytes(packed)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LZS_")}
    env["LZS_STREAM_DEBUG"] = "1"
    r = subprocess.run([os.path.join(ROOT, "lzs_compression_amd", "bin", "lzs-decompress"), str(tmp_path / "in.lzs"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "out.bin").read_bytes() == raw
    assert r.stderr.count("bytes decoded in") == 1 and "liblzs size query" in r.stderr, r.stderr[-3000:]
