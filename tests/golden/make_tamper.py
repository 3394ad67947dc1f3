#!/usr/bin/env python3
"""Golden verdicts for TAMPERED verifiers, from the REFERENCE verifiers.

tests/test_verdict_compare.py takes the width of every final compare from the oracle (pyoracle), whose widths were
read from the reference's source (pdf...c:184-189 `boundary`, msoffcrypto...c:168 and :184-188, odt...c:98-123).  This
records what the reference's own executables answer for the document's password on a subset of that module's streams
(golden_entries(): per family every fourth byte position of the tampered field, both ends of the compared width and the
first byte outside it; the Office hash_size gate streams; the ODF 2-byte and checksum-coverage streams; the R2 / R5
gate-only streams), so the oracle is pinned in the rejecting direction too.

Needs the reference verifiers built into oracle/_ref (`make -f oracle/ref.mk`, as for make_long.py):
    python tests/golden/make_tamper.py          -> tests/golden/tamper_verdicts.json
"""
import collections
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
import make_long as L  # noqa: E402
import test_verdict_compare as T  # noqa: E402


def main():
    out, codes = {}, collections.Counter()
    for name, stream, pw in T.golden_entries():
        code = L.ref_code(G.O.split_stream(stream), pw)
        assert code in (0, 1), (name, code)
        out[name] = dict(stream=stream, password=pw, code=code)
        codes[name.rsplit("-", 1)[0], code] += 1
    for name in out:
        if name.endswith("-base"):
            assert out[name]["code"] == 1, (name, "the reference must accept the untampered document's password")
    for k in sorted(codes):
        print(k, codes[k])
    json.dump(out, open(os.path.join(HERE, "tamper_verdicts.json"), "w"), indent=0)


if __name__ == "__main__":
    main()
