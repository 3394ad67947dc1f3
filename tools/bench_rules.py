#!/usr/bin/env python3
"""Rates of rule mode (dprf_search_rules: a word table times rules, k_spell_rules) against hybrid mode of the same
build over the bare word (dprf_search_hybrid with no mask position, k_spell_hybrid) -- on bench.py's test documents,
one device, stop_on_first off, no hit in any window.

  (a) hybrid   the bare word over 2^22 distinct 8-byte words
  (b) rules    the single rule ":" over the same table: the same candidates through the rule kernel
  (c) rules    64 rules of 1-3 functions, gather and per-unit functions mixed, over 2^16 words (also 2^22 candidates)
  (b64) rules  64 copies of ":" over the 2^16-word table, timed alternately with (c): (c)'s launches and table with
               no function work, which separates the interpreter's cost from the shape of the window

Each timed leg is `calls` library calls of `window` candidates (at most the keyspace of 2^22), the same for every leg
of a format, sized to about --seconds at the format's hybrid rate.  The sizing calls double as warm-up; (a) and (b)
are timed alternately --rounds times, then (b64) and (c), and the medians are reported with (a)'s run-to-run spread.
Writes profiles/bench_rules_<build>.json (or --out) and prints one JSON line per format.

Usage (on a machine with the GPU): python tools/bench_rules.py [--formats odt,office,...] [--seconds S]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

import bench  # noqa: E402
from dprf_amd import _lib, brute_force, rules  # noqa: E402

BIG, SMALL = 1 << 22, 1 << 16
SPACE = 1 << 22
RULES64 = [
    ":", "l", "u", "c", "C", "t", "r", "d", "f", "{", "}", "q", "k", "K", "[", "]", "E", "$1", "$!", "^1", "c $1",
    "c $1 $2", "$2 $0 $2", "sa@", "so0", "se3", "sa@ so0", "T0", "T1", "T2", "D0", "D1", "D2", "'4", "'5", "'6",
    "x03", "x14", "O12", "i1-", "i3.", "o0X", "o1_", "z1", "z2", "Z1", "Z2", "y2", "Y2", "p1", ".1", ",1", "*01",
    "*12", "@a", "@e", "r c", "u r", "d ]", "c $!", "l $1 $2", "^! $!", "t $7", "E $9"]


def words(n):
    """n < 2^24 distinct words of 8 bytes: letters and digits, mixed case."""
    return [b"W%c%06x" % (97 + k % 26, k) for k in range(n)]


def timed(fn, n, calls=1):
    t = time.perf_counter()
    for k in range(calls):
        st = fn(k, n)[2]
        assert st["candidates"] == n, (st, n)
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="odt,office,pdf_r34,pdf_r6,pdf_r2,pdf_r5")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build = _lib.build_id()
    S = bench.streams()
    big, small = words(BIG), words(SMALL)
    assert len(set(big)) == BIG
    one = rules.encode([rules.parse_rule(":")])
    many = rules.encode([rules.parse_rule(t) for t in RULES64])
    colons = rules.encode([rules.parse_rule(":")] * 64)
    assert len(RULES64) == 64 and all(1 <= len(rules.parse_rule(t)) <= 3 for t in RULES64)
    result = {"build": build, "words": BIG, "words_c": SMALL, "rules_c": RULES64, "seconds": a.seconds,
              "rounds": a.rounds, "formats": {}}
    for name in a.formats.split(","):
        with contextlib.redirect_stdout(io.StringIO()):
            fields = brute_force.parse_verification_data(S[bench.WORKLOADS[name][0]]["stream"])
        with _lib.Context(fields, device=0) as ctx:
            at = lambda k, n: (k * n) % (SPACE - n + 1)             # consecutive windows, wrapping in the keyspace
            hybrid = lambda k, n: ctx.search_hybrid([], 0, at(k, n), n)
            legs_big = {"a_hybrid": hybrid, "b_rules_colon": lambda k, n: ctx.search_rules(one, at(k, n), n)}
            legs_small = {"b64_rules_colons": lambda k, n: ctx.search_rules(colons, at(k, n), n),
                          "c_rules_64": lambda k, n: ctx.search_rules(many, at(k, n), n)}
            ctx.set_words(big)
            n = 1 << 14
            while True:                             # grow the window until a hybrid call runs 0.2 s or fills the keyspace
                dt = timed(hybrid, n)
                if dt >= 0.2 or n >= SPACE:
                    break
                n = min(SPACE, int(n * min(16.0, max(2.0, 0.3 / max(dt, 1e-4)))))
            n = max(1 << 12, min(SPACE, int(n * a.seconds / dt)))
            calls = max(1, int(round(a.seconds / max(timed(hybrid, n), 1e-4))))
            rates = {}
            for table, legs in ((None, legs_big), (small, legs_small)):
                if table is not None:
                    ctx.set_words(table)
                for fn in legs.values():
                    timed(fn, n, calls)             # warm-up at the timed size
                for leg in legs:
                    rates[leg] = []
                for _ in range(a.rounds):
                    for leg, fn in legs.items():    # alternating: drift of the machine hits both legs alike
                        rates[leg].append(n * calls / timed(fn, n, calls))
        rec = {"kernel": name, "window": n, "calls": calls}
        for leg in rates:
            rec[leg] = statistics.median(rates[leg])
            rec[leg + "_min_max"] = [min(rates[leg]), max(rates[leg])]
        rec["a_spread"] = (max(rates["a_hybrid"]) - min(rates["a_hybrid"])) / rec["a_hybrid"]
        rec["b_vs_a"] = rec["b_rules_colon"] / rec["a_hybrid"]
        rec["c_vs_a"] = rec["c_rules_64"] / rec["a_hybrid"]
        rec["c_vs_b64"] = rec["c_rules_64"] / rec["b64_rules_colons"]
        result["formats"][name] = rec
        print(json.dumps(rec), flush=True)
    out = a.out or os.path.join(REPO, "profiles", "bench_rules_%s.json" % build)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + out, file=sys.stderr)


if __name__ == "__main__":
    main()
