#!/usr/bin/env python3
"""Record inc_call_traces.json: the scenarios of tests/test_incremental_trace.py through the library named by LZS_LIBRARY --
a build of the commit whose per-call behaviour is to be kept, never the code under test.

    LZS_LIBRARY=path/to/that/liblzs.so python tests/golden/make_inc_call_traces.py host      (anywhere: no device needed)
    LZS_LIBRARY=path/to/that/liblzs.so python tests/golden/make_inc_call_traces.py device    (on the MI355X)

  inc_call_traces.json   {"host" | "device": {scenario: {"calls", "bytes", "digest"}}}: the number of calls, the bytes they
                         produced and the SHA-256 over one line a call (what it produced and consumed, the status byte and
                         every byte of reserved_ in the caller's block)

The named section is replaced, the other one kept.  Results only: the inputs are made again, from their seeds, by the tests.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    section = sys.argv[1] if len(sys.argv) > 1 else ""
    assert section in ("host", "device"), __doc__
    assert os.environ.get("LZS_LIBRARY"), "LZS_LIBRARY: the build to record (not this tree's)"
    os.environ["LZS_ROUTE"] = section
    os.environ["LZS_DEV_ENV"] = "1"
    import test_incremental_trace as T
    path = os.path.join(HERE, "inc_call_traces.json")
    record = {}
    if os.path.exists(path):
        with open(path) as f:
            record = json.load(f)
    record[section] = {}
    for name, run in T.SCENARIOS.items():
        record[section][name] = run().result()
        print(name, record[section][name])
    with open(path, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
