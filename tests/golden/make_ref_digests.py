"""Mints tests/golden/ref_digests.json: what the compiled reference (oracle/_ref/liblzs_ref.so, built by oracle/Makefile
where the reference's sources are) outputs for the inputs of two differential tests, as digests, so that those tests
compare with the reference wherever they run:
  * oracle_differential -- tests/test_oracle.py::test_live_differential_vs_reference, one digest per fuzz input over
    all the one-shot outputs compared for it;
  * incremental_decoder_on_malformed_streams -- tests/test_routes.py::test_incremental_decoder_on_malformed_streams_
    against_the_reference_itself, per stream the digest of the reference's incremental decoder's output and, where the
    stream holds a long offset of 0 inside the room, of the output up to that token.
Run from the repository root after build():  python tests/golden/make_ref_digests.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import oracle          # noqa: E402
import test_oracle     # noqa: E402
import test_routes     # noqa: E402

if not oracle.have_ref():
    raise SystemExit("oracle/_ref/liblzs_ref.so is not built: nothing to mint from")
R = oracle.ref()
doc = {
    "what": "digests of the compiled reference's outputs (tests/golden/make_ref_digests.py)",
    "oracle_differential": [test_oracle.outputs_digest(o) for o in test_oracle.differential_outputs(R)],
    "incremental_decoder_on_malformed_streams": [
        test_routes.malformed_digests(test_routes.ref_incremental_decode(s, room), test_routes._first_long_offset_zero(s), room)
        for s, room, _piece in test_routes.malformed_streams()],
}
with open(os.path.join(HERE, "ref_digests.json"), "w") as f:
    json.dump(doc, f, indent=0)
    f.write("\n")
print("wrote", os.path.join(HERE, "ref_digests.json"))
