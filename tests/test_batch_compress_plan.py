"""How lzs_compress_batch_device_sync() decides, on the CPU: lzs_plan_batch_compress_route(),
lzs_plan_batch_compress_group() and lzs_plan_batch_compress_segments() of csrc/lzs_launch_plan.h held to the literal rows of
tests/cpu_shim/batch_compress/route_check.c -- every precondition one side and the other, both forced values of
LZS_BATCH_COMPRESS_ROUTE, the measured thresholds one below, at and one above, a batch whose strides sum beyond 32 bits; a block
above the groups' bound, a sum exactly at it, blocks without a byte; ragged lengths, multiples of the segment size and length 0
in the segment table -- in a program of its own built with -Wall -Wextra -Werror and the address and undefined-behaviour
sanitizers."""
import os
import subprocess

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_shim", "batch_compress")


def test_the_plan_gives_its_tables(tmp_path):
    program = tmp_path / "batch_compress_route_check"
    r = subprocess.run(["make", "-C", HERE, f"OUT={tmp_path}", str(program)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LZS_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(program)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "58 rows, 0 failure(s)" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
