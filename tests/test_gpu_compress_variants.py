"""Every variant of the compress kernel against the oracle on contents BUILT for its tables.

kernels/compress_wg.inc is compiled four times for the block and packed entries: wgv_text, wgv_few, wgv_lit, wgv_safe.  Which one a
process runs is decided by switches the library reads once (LZS_VARIANT, LZS_CHAIN_FALLBACK), so each case is a child process --
tests/helpers/compress_variant_worker.py -- started one after the other, never in parallel.  The child first proves which variant
it runs (lzs_hip_forced_variant(), the "order-independent fallback" of backend_info()), then compares with the oracle, length and
bytes: every content of its table shape (tests/compress_variant_programs.py; tests/test_compress_variant_programs.py proves on the
CPU what they reach) cut to every length of test_gpu_search_hop_end.LENGTHS, the class-change blocks at full length and cut just
behind the classifier's horizon, through one strided and one packed launch; four contents at rooms of 0, 1, 2, 255, 256, 257,
full - 1 and full bytes into outputs prefilled with 0xA5.  `by-class` (no switch) begins with the first compress launch of its
process -- all three variants run -- over 66 blocks whose classes the classifier must name as they were built.

Time: one clean child on an MI355X took 2.3 - 2.5 s, start of the process and imports included (the child prints its own figure,
1.8 - 2.1 s from its first line on); the limit, CHILD_LIMIT, is about ten times that, rounded up: 30 s.  After a child that ends
by a signal, an abort or the limit the remaining cases fail at once without starting a process: nothing more is started on a
device that may have faulted.
"""
import json
import os
import subprocess
import sys

import pytest

import compress_variant_programs as P
import test_gpu_search_hop_end as H

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
WORKER = os.path.join(ROOT, "tests", "helpers", "compress_variant_worker.py")
CHILD_LIMIT = 30                       # seconds: ten times a clean child
CASES = {"text": {"LZS_VARIANT": "text"}, "few": {"LZS_VARIANT": "few"}, "lit": {"LZS_VARIANT": "lit"},
         "safe": {"LZS_CHAIN_FALLBACK": "1"}, "by-class": {}}
_stopped = []                          # the latch: why no further child is started


@pytest.mark.parametrize("case", list(CASES))
def test_the_variant_gives_the_oracles_bytes_on_built_content(case):
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    env = {k: v for k, v in os.environ.items() if k not in ("LZS_VARIANT", "LZS_CHAIN_FALLBACK", "LZS_KERNEL", "LZS_VERIFY")}
    env.update(CASES[case], PYTHONPATH=ROOT)
    try:
        r = subprocess.run([sys.executable, WORKER, case], capture_output=True, text=True, env=env, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired as e:
        _stopped.append(f"the child of case {case} ran into its limit of {CHILD_LIMIT} s")
        pytest.fail(_stopped[0] + ": " + str(e.stderr)[-2000:])
    if r.returncode < 0 or r.returncode in (134, 139):
        _stopped.append(f"the child of case {case} ended by a signal or an abort (exit status {r.returncode})")
        pytest.fail(_stopped[0] + ": " + r.stderr[-2000:])
    assert r.returncode == 0, (case, r.stderr[-3000:])
    report = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, {k: v for k, v in report.items() if k != "failures"})
    # none left out: every content at every length and the class-change blocks at four, strided and packed; four contents at
    # eight rooms, packed and strided; by-class: 66 blocks twice before that
    cut = len(P.builders(P.SHAPES.get(case, P.DEFAULT))) * len(H.LENGTHS) + len(P.CLASS_CHANGES) * (1 + len(P.CLASS_CHANGE_LENGTHS))
    assert report["case"] == case and report["blocks"] == 2 * cut + 2 * 4 * 8 + (2 * 66 if case == "by-class" else 0), report
    assert report["failures"] == [], report["failures"]
