"""What csrc/lzs_burst_plan.h adds for history resets inside a burst on the CPU: the decoder's staging slots and the
start marks lie inside the parts of the work area they borrow at n = 1, 2, 3, 255, 256, 257, 65 536 and LZS_BURST_PACKETS_MAX, every
field and size the header had before is where it was, RESOLVE's grid with flags and a run's staging slot -- held to the table of
literal rows in tests/cpu_shim/burst_flags_plan_check.c, a program of its own built with -Wall -Wextra -Werror and the address and
undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SHIM = os.path.join(ROOT, "tests", "cpu_shim")
CSRC = os.path.join(ROOT, "lzs_compression_amd", "csrc")


def test_the_flags_plan_gives_its_table(tmp_path):
    program = tmp_path / "burst_flags_plan_check"
    r = subprocess.run([os.environ.get("CC", "gcc"), "-O1", "-g", "-fno-omit-frame-pointer", "-std=c11", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}",
                        os.path.join(SHIM, "burst_flags_plan_check.c"), "-o", str(program)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LZS_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(program)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and " 0 failure(s)" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
