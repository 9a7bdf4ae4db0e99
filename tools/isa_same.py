"""usage: tools/isa_same.py [--registers] PARENT.s NEW.s  -- two outputs of tools/isa.sh: does every kernel of the first have the same
instructions and the same metadata (registers, LDS, scratch, arguments) in the second?  Line tables, assembler comments and the
per-function numbers in local labels (.LBB12_3: the 12 moves when a kernel is added in front) are left out of the comparison.
Prints what differs, then a count and the kernels only NEW.s has; exit status 1 if anything differs or is missing.
--registers: a kernel whose instructions are the same, line for line, once register numbers are blanked, and whose metadata is
identical, is listed as such and not counted as a difference (another register assignment, nothing else); of the others it says
whether they are the same instructions in another order.

    git stash; tools/isa.sh /tmp/parent.s; git stash pop; tools/isa.sh /tmp/new.s; python tools/isa_same.py /tmp/parent.s /tmp/new.s
"""
import re
import sys


def kernels(path):
    s = open(path).read()
    code = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @", s, re.M):
        body = s[m.start():s.index(".Lfunc_end", m.start())]
        body = "\n".join(line for line in body.splitlines() if not re.match(r"\s*(\.loc|\.file|\.cfi|;)", line) and not line.startswith(".Ltmp"))
        body = re.sub(r"\s*;.*$", "", body, flags=re.M)
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        body = re.sub(r"\.L(func_begin|func_end|tmp|JTI|__unnamed_)\d+", r".L\1", body)
        code[m.group(1)] = body
    meta = {}
    for block in re.split(r"\n  - \.", s[s.index("amdhsa.kernels"):] if "amdhsa.kernels" in s else ""):
        m = re.search(r"\.name:\s+(\S+)", block)
        if m:
            meta[m.group(1)] = block.split("\namdhsa.")[0]
    return code, meta


def blank(body):
    """Register numbers out: v12, s[4:5], a3 -> v, s, a."""
    return re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1", body)


def main():
    args = [x for x in sys.argv[1:] if x != "--registers"]
    registers = len(args) != len(sys.argv) - 1
    (a, am), (b, bm) = kernels(args[0]), kernels(args[1])
    bad = 0
    for what, old, new in (("ISA", a, b), ("metadata", am, bm)):
        for k in old:
            if k not in new or old[k] != new[k]:
                if registers and what == "ISA" and k in new and am.get(k) == bm.get(k):
                    x, y = blank(old[k]).splitlines(), blank(new[k]).splitlines()
                    if x == y:
                        print(f"ISA the same but for register numbers: {k}")
                        continue
                    if sorted(x) == sorted(y):
                        print(f"ISA differs (the same instructions in another order): {k}")
                        bad += 1
                        continue
                print(f"{what} {'missing' if k not in new else 'differs'}: {k}")
                bad += 1
    print(f"{len(a)} kernels and {len(am)} metadata entries of {args[0]}: {bad} differences; only in {args[1]}: {[k for k in b if k not in a]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
