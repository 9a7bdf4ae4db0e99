"""What the tests of the size query for long streams share: the limits a stream is asked at, what the bit-by-bit
model of tests/test_decoded_size_host.py expects there, and the extra blocks of the batch tests.  Helper module, not a conftest:
nothing here is a test."""
import functools

import numpy as np

import oracle
import stream_border_programs as P
from test_decoded_size_host import model

O = oracle.oracle()
F = {name: i for i, name in enumerate(oracle.SEGMENT_FIELDS)}
BIG = 1 << 22
MAX64 = (1 << 64) - 1
SEGS = (256, 512)                                  # LZS_DEC_SEG: the directed streams are built for borders every 256 bytes
BATCH_LIMITS = (300_000, 20_001, 999, 0, 0xFFFFFFFF)
EXTRA_BLOCKS = (b"", b"\x20", b"\xC0\x00", bytes(np.random.default_rng(7).integers(0, 256, 5000, dtype=np.uint8)))


def by_name(name):
    return next(s for s in P.directed_streams() if s.name == name)


@functools.lru_cache(maxsize=None)
def model_of(data, limit):
    """tests/test_decoded_size_host.py: model(), remembered (a walk over a directed stream is 30 ms)."""
    return model(data, limit)


def _expected(name, limit):
    return model_of(by_name(name).data, limit)


def expected(s, limit):
    """(size, status) of the plain rule at ``limit``."""
    return _expected(s.name, limit)


@functools.lru_cache(maxsize=None)
def _limits(name, seg):
    s = by_name(name)
    true = _expected(name, MAX64)[0]
    limits = {MAX64, true, max(true - 1, 0), 0, 1}
    _, rec = O.scan_segments(s.data, seg, BIG)
    reached = np.flatnonzero(rec[:, F["entry_bit"]] != oracle.SEGMENT_NEVER)
    for k in (int(reached[len(reached) // 2]), int(reached[-1])):
        for d in (-1, 0, 1):
            limits.add(max(int(rec[k, F["out_start"]]) + d, 0))
    return tuple(sorted(limits))


def limits(s, seg):
    """The maximum, the true size and one below, 0, 1, and the output start of a middle and of the last segment the stream
    reaches (the model's: oracle.scan_segments) - 1, + 0, + 1."""
    return _limits(s.name, seg)


@functools.lru_cache(maxsize=None)
def _file_total(name, seg):
    return O.scan_segments(by_name(name).data, seg, BIG, file_rule=True)[0]


def expected_file_rule(s, seg, limit):
    """(size, status) under the file rule: the model's total cut at the limit; full, or starved -- never an end marker."""
    size = min(_file_total(s.name, seg), limit)
    return size, (8 if size == limit else 3)


def batch_blocks():
    """All directed streams, an empty block, a block of one byte, a marker alone, garbage."""
    return [s.data for s in P.directed_streams()] + list(EXTRA_BLOCKS)


def rows(datas):
    stride = (max(len(d) for d in datas) + 63) // 64 * 64
    arr = np.zeros((len(datas), stride), dtype=np.uint8)
    for i, d in enumerate(datas):
        arr[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    return arr, np.array([len(d) for d in datas], dtype=np.uint32)
