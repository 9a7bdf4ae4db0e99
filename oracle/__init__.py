"""ctypes front-end for the CHECKERS under oracle/.

TEST INFRASTRUCTURE ONLY.  Importable from tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg; the product package (lzs_compression_amd) never
imports this module.

Two checkers, same four-argument signature as the reference's one-shot calls
(c/src/liblzs/lzs.h:218,229):

* ``oracle``  -- oracle/liblzs_oracle.so, our CPU restatement (lzs_oracle.c).
* ``ref``     -- oracle/_ref/liblzs_ref.so, the REAL reference compiled from
                 /root/reference by oracle/Makefile (present only if it was built
                 in the container and travelled with the snapshot).
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (LZS_ORACLE_SO: another build of the restatement -- tests/test_sanitizers.py points it at oracle/_build/liblzs_oracle_asan.so)
_ORACLE_SO = os.environ.get("LZS_ORACLE_SO") or os.path.join(_HERE, "liblzs_oracle.so")
_REF_SO = os.path.join(_HERE, "_ref", "liblzs_ref.so")

_SIG = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]


def build(quiet: bool = True) -> None:
    """Compile the restatement (always) and the reference (when its sources exist)."""
    subprocess.run(["make", "-C", _HERE, "all"], check=True,
                   stdout=subprocess.DEVNULL if quiet else None)


def compressed_max(n: int) -> int:
    """LZS_COMPRESSED_MAX (c/src/liblzs/lzs.h:77)."""
    return n + (n + 7) // 8 + 3


class _Codec:
    def __init__(self, path: str, compress: str, decompress: str, extra: Sequence[str] = ()):
        self.path = path
        self.lib = ctypes.CDLL(path)
        self._c = getattr(self.lib, compress)
        self._d = getattr(self.lib, decompress)
        for f in (self._c, self._d):
            f.restype = ctypes.c_size_t
            f.argtypes = _SIG
        for name in extra:
            f = getattr(self.lib, name)
            f.restype = ctypes.c_size_t
            f.argtypes = _SIG
            setattr(self, "_" + name, f)

    @staticmethod
    def _call(fn, data: bytes, cap: int) -> bytes:
        # +1 spare input byte: the reference reads in[len] once (lzs-compression.c:437).
        src = ctypes.create_string_buffer(bytes(data) + b"\0", len(data) + 1)
        dst = ctypes.create_string_buffer(max(cap, 1))
        n = fn(ctypes.addressof(dst), cap, ctypes.addressof(src), len(data))
        assert n <= cap
        return dst.raw[:n]

    def compress(self, data: bytes, cap: Optional[int] = None) -> bytes:
        return self._call(self._c, data, compressed_max(len(data)) if cap is None else cap)

    def decompress(self, data: bytes, cap: int) -> bytes:
        return self._call(self._d, data, cap)

    # function addresses, for the threaded block runner
    @property
    def compress_addr(self) -> int:
        return ctypes.cast(self._c, ctypes.c_void_p).value

    @property
    def decompress_addr(self) -> int:
        return ctypes.cast(self._d, ctypes.c_void_p).value


# what lzs_oracle_decompress_channel counts (the enum beside it), in order
CHANNEL_COUNTERS = ("zero_bytes", "crossing", "overlap", "long_small", "long_zero", "cut", "nibble0_marker", "nibble0_full")

# what lzs_oracle_compress_channel counts (the enum before compress_core), in order
CHANNEL_ENCODE_COUNTERS = ("src_in_history", "src_straddles", "offset_2047", "reaches_view_0", "short_form_127", "long_form_128",
                           "nibble_15", "ext_ends_at_packet_end", "search_cut_by_end", "last_byte_literal", "first_token_offset_1",
                           "cut")


# ---- lzs_oracle_scan_segments (oracle/lzs_oracle.c: the enums beside it)
SEGMENT_FIELDS = ("entry_bit", "entry_ext", "entry_off", "bytes", "out_start", "stop", "merge", "phantoms")
SEGMENT_NEVER = 0xFFFFFFFF                      # entry_bit: the walk never got here; merge: not inside the segment
STOP_MARKER, STOP_INPUT, STOP_FULL = 1, 2, 3    # stop
STEP_KINDS = ("lit", "short2", "long2", "short4", "long4", "short8", "long8", "first_nibble", "nib15", "close0", "close1",
              "close14", "close_other", "marker", "long_zero")
STEP_WIDTH = {"lit": 9, "short2": 11, "long2": 15, "short4": 13, "long4": 17, "short8": 13, "long8": 17, "first_nibble": 4,
              "nib15": 4, "close0": 4, "close1": 4, "close14": 4, "close_other": 4, "marker": 9, "long_zero": 13}
OFFSET_CLASSES = ("1", "2", "127 short form", "127 long form", "128", "1024", "2047", "other")
OFFSET_EDGES = (1023, 1024, 1025, 2046, 2047)
_SCAN_B = 24


class ScanCounters:
    """What lzs_oracle_scan_segments counts, as named views of one uint64 array (``raw``) that its calls add to."""
    _LAYOUT = (("straddle", (len(STEP_KINDS), _SCAN_B)),      # [kind][b]: steps with b of their bits in front of a border
               ("ext_entry", (8, 16)),                       # [offset class][closing nibble, 15 = never closed]
               ("close_at", (16,)),                          # [d + 8]: closing nibbles that start d bits behind a border
               ("ones_seg", (2, 4)),                         # [next three bits set][entry bit & 3]: whole 0xFF segments in an extension
               ("ones_run", (5,)),                           # [0 1 2 3 >=4] whole 0xFF segments under one extension that crosses a border
               ("short_all_ones", (1,)),                     # borders crossed by the extension of a short token 11 1111111 1111
               ("phantom", (5,)),                            # [0 1 2 3 >=4] end markers the guessed walk read before it merged
               ("never", (1,)), ("never_run_max", (1,)),
               ("src_own", (1,)), ("src_other", (1,)), ("src_straddle", (1,)), ("src_before_out0", (1,)),
               ("before_out0_seg", (16,)),                   # [segment, 15 = later]
               ("off_edge", (5,)), ("off_edge_first", (5,)), # [1023 1024 1025 2046 2047]; ... producing a segment's first byte
               ("chain_max", (1,)), ("small_segs", (1,)))

    def __init__(self):
        size = sum(int(np.prod(shape)) for _, shape in self._LAYOUT)
        self.raw = np.zeros(size, dtype=np.uint64)
        at = 0
        for name, shape in self._LAYOUT:
            k = int(np.prod(shape))
            setattr(self, name, self.raw[at:at + k].reshape(shape))
            at += k


# ---- lzs_oracle_compress_segments (oracle/lzs_oracle.c: the enums beside it)
COMPRESS_SEGMENT_FIELDS = ("entry", "exit", "tokens", "bits", "bit_at", "empty", "oversized", "guess_merge", "guess_exit", "redone",
                           "round_exit")
COMPRESS_NEVER = 0xFFFFFFFFFFFFFFFF             # entry: a match ran over all of the segment; guess_merge: not inside the segment
LAST_KINDS = ("lit", "short2-7", "long2-7", "ext0", "ext1", "ext2", "ext3-39", "ext40+")   # ext: length 8 and more, by its nibbles of 15
LAST_PAST = 21                                  # 0 .. 16 bytes past the border; 17: farther, in the next segment; 18 19 20: past 1, 2, >= 3 whole segments
FIRST_OFFSETS = (2047, 2046, 2040, 1)
WARM_UPS = ("at 0", "first beyond", "far")
MERGE_CLASSES = ("0", "1", "2", "3-4", ">=5", "never")


def slot_bits(seg: int) -> int:
    """The bits of a segment's slot, the host's figure: 8 * align16(LZS_COMPRESSED_MAX(seg))."""
    return 8 * ((compressed_max(seg) + 15) & ~15)


class CompressCounters:
    """What lzs_oracle_compress_segments counts, as named views of one uint64 array (``raw``) that its calls add to."""
    _LAYOUT = (("last", (len(LAST_KINDS), LAST_PAST)),       # [kind][past]: the last token of a segment with a border behind it
               ("last_close", (4,)),                         # [0 1 14 other]: closing nibbles of last tokens that end past their border
               ("last_start", (9,)),                         # [s]: last tokens that are matches, s = 1 .. 8 bytes before the border (0: farther)
               ("one_token_last_byte", (1,)),
               ("entry_mod64", (64,)),
               ("first_off", (4, 3)),                        # [2047 2046 2040 1][warm-up at 0, first beyond, far]
               ("first_straddle", (1,)), ("first_far_len", (2,)),
               ("merge", (6,)),                              # [0 1 2 3-4 >=5 never]
               ("one_round", (1,)), ("rounds_max", (1,)), ("fix_changes_exit", (1,)), ("fix_keeps_exit", (1,)),
               ("never_run_max", (1,)),
               ("long_match", (3,)),                         # [offset 1, 2, 300]: the most segments under one token
               ("bit_at_mod32", (32,)), ("nbits_mod32", (32,)), ("under_32", (1,)), ("word_share_max", (1,)),
               ("empty_between_sharers", (1,)), ("total_mod32", (32,)), ("marker_behind_empty", (1,)),
               ("marker_behind_oversized", (1,)),
               ("margin", (18,)),                            # [d + 8], d = -8 .. 8; [17]: more than 4096 bits over
               ("over_bit_at", (4,)),                        # [0, 1-31, 32-2016, >= 2017]: oversized segments by bit_at % 2048
               ("over_seg0", (1,)), ("over_two", (1,)), ("over_empties_one_token", (1,)),
               ("len_mod", (5,)),                            # [n % seg: 1 63 64 255 0]
               ("end_close", (2,)),                          # [0 14]
               ("end_one_short", (1,)))

    def __init__(self):
        size = sum(int(np.prod(shape)) for _, shape in self._LAYOUT)
        self.raw = np.zeros(size, dtype=np.uint64)
        at = 0
        for name, shape in self._LAYOUT:
            k = int(np.prod(shape))
            setattr(self, name, self.raw[at:at + k].reshape(shape))
            at += k


class _Oracle(_Codec):
    def __init__(self):
        if not os.path.exists(_ORACLE_SO):
            build()
        super().__init__(_ORACLE_SO, "lzs_oracle_compress", "lzs_oracle_decompress",
                         extra=("lzs_oracle_compress_brute",))
        self.lib.lzs_cpu_run_blocks.restype = ctypes.c_double
        self.lib.lzs_cpu_run_blocks.argtypes = [
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
            ctypes.c_int]
        self.lib.lzs_oracle_trace.restype = ctypes.c_size_t
        self.lib.lzs_oracle_trace.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                              ctypes.c_size_t]
        self.lib.lzs_oracle_decompress_channel.restype = ctypes.c_size_t
        self.lib.lzs_oracle_decompress_channel.argtypes = [
            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
            ctypes.c_void_p, ctypes.c_void_p]
        self.lib.lzs_oracle_compress_channel.restype = ctypes.c_size_t
        self.lib.lzs_oracle_compress_channel.argtypes = [
            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
            ctypes.c_void_p]
        self.lib.lzs_oracle_scan_segments.restype = ctypes.c_size_t
        self.lib.lzs_oracle_scan_segments.argtypes = [
            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        self.lib.lzs_oracle_compress_segments.restype = ctypes.c_size_t
        self.lib.lzs_oracle_compress_segments.argtypes = [
            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
            ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        sizes = (ctypes.c_uint32 * 4)()
        self.lib.lzs_oracle_compress_segments_layout(sizes)
        assert list(sizes) == [CompressCounters().raw.size, len(COMPRESS_SEGMENT_FIELDS), len(LAST_KINDS), LAST_PAST], list(sizes)
        sizes = (ctypes.c_uint32 * 4)()
        self.lib.lzs_oracle_scan_layout(sizes)
        assert list(sizes) == [ScanCounters().raw.size, len(SEGMENT_FIELDS), len(STEP_KINDS), _SCAN_B], list(sizes)

    def scan_segments(self, data: bytes, seg: int, cap: int, file_rule: bool = False, counters: Optional[ScanCounters] = None,
                      trace: bool = False):
        """The plain model of a segment border (lzs_oracle_scan_segments): ``data`` cut every ``seg`` bytes, walked once from
        bit 0 under the one-shot rule (or the file rule of lzs_decompress_concat) up to ``cap`` bytes of output, and every
        segment walked once more from its border bit in the normal state.  Returns (bytes produced, records [nseg,
        len(SEGMENT_FIELDS)] uint32) -- and, with ``trace``, the steps of the true walk [(bit, kind, offset, bytes, output
        position)], one a token and one a length nibble.  ``counters``: a ScanCounters that the call adds to."""
        nseg = (len(data) + seg - 1) // seg
        src = ctypes.create_string_buffer(bytes(data), len(data) + 1)
        rec = np.zeros((max(nseg, 1), len(SEGMENT_FIELDS)), dtype=np.uint32)
        max_tok = 2 * len(data) + 1 if trace else 0   # no step is shorter than four bits
        steps = np.zeros((max_tok, 5), dtype=np.uint32) if trace else None
        ntok = ctypes.c_size_t(0)
        n = self.lib.lzs_oracle_scan_segments(
            ctypes.addressof(src), len(data), seg, int(file_rule), cap, rec.ctypes.data, nseg,
            None if counters is None else counters.raw.ctypes.data, None if steps is None else steps.ctypes.data, max_tok,
            ctypes.addressof(ntok))
        if n == ctypes.c_size_t(-1).value:
            raise MemoryError("lzs_oracle_scan_segments")
        got = (int(n), rec[:nseg])
        return got + (steps[:ntok.value],) if trace else got

    def compress_segments(self, data: bytes, seg: int, counters: Optional[CompressCounters] = None, trace: bool = False,
                          brute: bool = False):
        """The plain model of a segment border of the segmented stream compressor (lzs_oracle_compress_segments): ``data`` cut
        every ``seg`` bytes and parsed once; every segment behind the first walked once more from its own border; the host's
        rounds simulated on those walks.  Returns (bits of all tokens, records [nseg, len(COMPRESS_SEGMENT_FIELDS)] uint64,
        the segments to redo after each round -- its length is the number of rounds) -- and, with ``trace``, the tokens
        [(position, offset or 0, bytes covered, bit position)].  ``counters``: a CompressCounters that the call adds to;
        ``brute``: the written search rule instead of the chained finder."""
        nseg = max((len(data) + seg - 1) // seg, 1)
        src = ctypes.create_string_buffer(bytes(data), len(data) + 1)
        rec = np.zeros((nseg, len(COMPRESS_SEGMENT_FIELDS)), dtype=np.uint64)
        rounds = np.zeros(nseg + 1, dtype=np.uint32)          # a round settles at least one segment more
        max_tok = len(data) if trace else 0                   # no token covers less than a byte
        toks = np.zeros((max_tok, 4), dtype=np.uint32) if trace else None
        ntok, nrounds = ctypes.c_size_t(0), ctypes.c_size_t(0)
        bits = self.lib.lzs_oracle_compress_segments(
            ctypes.addressof(src), len(data), seg, int(brute), rec.ctypes.data, nseg, rounds.ctypes.data, rounds.size,
            ctypes.addressof(nrounds), None if counters is None else counters.raw.ctypes.data,
            None if toks is None else toks.ctypes.data, max_tok, ctypes.addressof(ntok))
        if bits == ctypes.c_size_t(-1).value:
            raise MemoryError("lzs_oracle_compress_segments")
        assert nrounds.value <= rounds.size
        got = (int(bits), rec, [int(v) for v in rounds[:nrounds.value]])
        return got + (toks[:ntok.value],) if trace else got

    def compress_brute(self, data: bytes, cap: Optional[int] = None) -> bytes:
        return self._call(self._lzs_oracle_compress_brute, data,
                          compressed_max(len(data)) if cap is None else cap)

    def trace(self, data: bytes, max_tok: int = 1 << 20) -> np.ndarray:
        """Token list [(pos, off, total_len)], off 0 = literal (debug aid)."""
        src = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
        rec = np.zeros((max_tok, 3), dtype=np.uint32)
        n = self.lib.lzs_oracle_trace(ctypes.addressof(src), len(data), rec.ctypes.data, max_tok)
        return rec[:min(n, max_tok)]

    def decompress_channel(self, hist: bytes, data: bytes, cap: int, counters: Optional[np.ndarray] = None,
                           trace: bool = False):
        """One packet of a channel through the plain model of include/lzs/lzs_channels.h (lzs_oracle_decompress_channel):
        ``hist`` is the channel's history (at most 2047 bytes), ``cap`` the output capacity.  Returns (output bytes, status
        byte, new history) -- and, with ``trace``, the token list [(output position, offset or 0, bytes produced, bit
        position)] and the bit at which the packet stopped (its marker's first bit, if it stopped at one).  ``counters``: a
        uint64 array of len(CHANNEL_COUNTERS) that the call adds to."""
        assert len(hist) <= 2047
        room = min(cap, 30 * len(data) + 16)          # a nibble gives at most 15 bytes: no packet decodes to more
        src = ctypes.create_string_buffer(bytes(data), len(data) + 1)
        old = ctypes.create_string_buffer(bytes(hist), len(hist) + 1)
        dst = ctypes.create_string_buffer(room + 1)
        new = ctypes.create_string_buffer(2048)
        new_h, ntok, status, stop = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint8(0), ctypes.c_uint64(0)
        if counters is not None:
            assert counters.dtype == np.uint64 and counters.size == len(CHANNEL_COUNTERS) and counters.flags.c_contiguous
        max_tok = 2 * len(data) + 1 if trace else 0   # no token is shorter than four bits
        rec = np.zeros((max_tok, 4), dtype=np.uint32) if trace else None
        n = self.lib.lzs_oracle_decompress_channel(
            ctypes.addressof(dst), cap, ctypes.addressof(src), len(data), ctypes.addressof(old), len(hist),
            ctypes.addressof(new), ctypes.addressof(new_h), ctypes.addressof(status),
            None if counters is None else counters.ctypes.data, None if rec is None else rec.ctypes.data, max_tok,
            ctypes.addressof(ntok), ctypes.addressof(stop))
        assert n <= room
        got = (dst.raw[:n], int(status.value), new.raw[:new_h.value])
        return got + (rec[:ntok.value], int(stop.value)) if trace else got

    def compress_channel(self, hist: bytes, data: bytes, cap: Optional[int] = None, brute: bool = False,
                         counters: Optional[np.ndarray] = None, trace: bool = False):
        """One packet of a channel through the plain model of include/lzs/lzs_channels.h compression
        (lzs_oracle_compress_channel): ``hist`` is the channel's history (at most 2047 bytes), ``cap`` the output capacity
        (default: compressed_max(len(data)), room for all of it).  Returns (the stream cut at ``cap``, the uncut length, the
        status byte, the new history) -- and, with ``trace``, the token list [(position in the packet, offset or 0, bytes
        covered, bit position)].  ``brute``: the written search rule instead of the chained finder.  ``counters``: a uint64
        array of len(CHANNEL_ENCODE_COUNTERS) that the call adds to."""
        assert len(hist) <= 2047
        if cap is None:
            cap = compressed_max(len(data))
        src = ctypes.create_string_buffer(bytes(data), len(data) + 1)
        old = ctypes.create_string_buffer(bytes(hist), len(hist) + 1)
        dst = ctypes.create_string_buffer(cap + 1)
        new = ctypes.create_string_buffer(2048)
        new_h, ntok, total, status = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint8(0)
        if counters is not None:
            assert counters.dtype == np.uint64 and counters.size == len(CHANNEL_ENCODE_COUNTERS) and counters.flags.c_contiguous
        max_tok = len(data) if trace else 0           # no token covers less than a byte
        rec = np.zeros((max_tok, 4), dtype=np.uint32) if trace else None
        n = self.lib.lzs_oracle_compress_channel(
            ctypes.addressof(dst), cap, ctypes.addressof(src), len(data), ctypes.addressof(old), len(hist), int(brute),
            ctypes.addressof(total), ctypes.addressof(new), ctypes.addressof(new_h), ctypes.addressof(status),
            None if counters is None else counters.ctypes.data, None if rec is None else rec.ctypes.data, max_tok,
            ctypes.addressof(ntok))
        if n == ctypes.c_size_t(-1).value:
            raise MemoryError("lzs_oracle_compress_channel")
        assert n == min(total.value, cap) and dst.raw[cap:] == b"\0"
        got = (dst.raw[:n], int(total.value), int(status.value), new.raw[:new_h.value])
        return got + (rec[:ntok.value],) if trace else got


_oracle: Optional[_Oracle] = None
_ref: Optional[_Codec] = None


def oracle() -> _Oracle:
    global _oracle
    if _oracle is None:
        _oracle = _Oracle()
    return _oracle


def have_ref() -> bool:
    return os.path.exists(_REF_SO)


def ref() -> _Codec:
    """The compiled reference; raises FileNotFoundError where it did not travel."""
    global _ref
    if _ref is None:
        if not have_ref():
            raise FileNotFoundError(_REF_SO)
        _ref = _Codec(_REF_SO, "lzs_compress", "lzs_decompress", extra=("lzs_simple_compress",))
    return _ref


def run_blocks(codec: _Codec, blocks: np.ndarray, *, decompress: bool = False,
               in_len: Optional[np.ndarray] = None, out_cap: Optional[int] = None,
               threads: int = 1):
    """Run a CPU one-shot codec over independent blocks, one block per task.

    blocks: uint8 array [nblocks, stride].  Returns (out[nblocks, out_cap], out_len[nblocks],
    seconds).  Used by tests as a many-block checker and by bench.py's cpu_baseline."""
    assert blocks.dtype == np.uint8 and blocks.ndim == 2
    nb, stride = blocks.shape
    # one spare byte after the last block for the reference's 1-byte over-read
    flat = np.zeros(nb * stride + 16, dtype=np.uint8)
    flat[:nb * stride] = blocks.reshape(-1)
    if out_cap is None:
        out_cap = stride if decompress else compressed_max(stride)
    out = np.empty((nb, out_cap), dtype=np.uint8)
    out.fill(0)                      # touch the pages now, not inside the timed threads
    out_len = np.zeros(nb, dtype=np.uint32)
    if in_len is not None:
        in_len = np.ascontiguousarray(in_len, dtype=np.uint32)
    fn = codec.decompress_addr if decompress else codec.compress_addr
    secs = oracle().lib.lzs_cpu_run_blocks(
        fn, out.ctypes.data, out_cap, out_cap, out_len.ctypes.data,
        flat.ctypes.data, stride, None if in_len is None else in_len.ctypes.data,
        stride, nb, threads)
    if secs < 0:
        raise RuntimeError("lzs_cpu_run_blocks failed")
    return out, out_len, secs
