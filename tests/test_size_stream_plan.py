"""Which route the size query of a batch with host lengths takes, on the CPU: lzs_plan_size_route() of
csrc/lzs_launch_plan.h held to the literal rows of tests/cpu_shim/size_stream/route_check.c -- the 32-bit extent at 0xFFFFFFFF and
0x100000000, the measured threshold one below, at and one above, both forced values of LZS_SIZE_ROUTE -- in a program of its own
built with -Wall -Wextra -Werror and the address and undefined-behaviour sanitizers."""
import os
import subprocess

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_shim", "size_stream")


def test_the_size_route_gives_its_table(tmp_path):
    program = tmp_path / "size_route_check"
    r = subprocess.run(["make", "-C", HERE, f"OUT={tmp_path}", str(program)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LZS_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(program)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "18 rows, 0 failure(s)" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
