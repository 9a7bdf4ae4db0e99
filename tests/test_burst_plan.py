"""The burst calls' host arithmetic on the CPU: csrc/lzs_burst_plan.h -- where the parts of the work area lie (aligned, in order, not
overlapping, the split decoder's tables inside the slots), the three work-area sizes with their clamps and overflow rules, the bits of
the channel sort, the grid of RESOLVE, whether a strided or a packed call splits, split_min -- held to the table of literal rows in
tests/cpu_shim/burst_plan_check.c, a program of its own built with -Wall -Wextra -Werror and the address and undefined-behaviour
sanitizers.  lzs_channels_burst.hip, lzs_channels.c and lzs_packed.c ask these functions; none keeps a copy of a rule."""
import os
import subprocess

SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_shim")


def test_the_burst_plan_gives_its_table():
    program = os.path.join(SHIM, "_build", "burst_plan_check")
    r = subprocess.run(["make", "-C", SHIM, program], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LZS_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and " 0 failure(s)" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
