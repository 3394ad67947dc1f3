#!/usr/bin/env python3
"""Rates of hybrid mode (dprf_search_hybrid: a word table times a mask, k_spell_hybrid) against mask mode of the same
build (dprf_search_mask, k_spell_mask) over candidates of the same number and length -- on bench.py's test documents,
one device, stop_on_first off, no hit in either window.

  hybrid   "?w?d?d?d" over 2^16 generated 8-letter words (keyspace 65,536,000)
  mask     "?l?l?l?l?l?l?l?l?d?d?d": 11 bytes per candidate as well

Each timed leg is `calls` library calls of `window` candidates, the same for both legs of a format, sized to about
--seconds at the format's mask rate (the hybrid keyspace caps a call at 65,536,000 candidates, which the fastest
format verifies in milliseconds: hence several calls per leg).  The sizing calls double as warm-up; the two legs are
then timed alternately --rounds times and the medians reported with the spread.  Writes
profiles/hybrid_rate_<build>.json (or --out) and prints one JSON line per format.

Usage (on a machine with the GPU): python tools/bench_hybrid.py [--formats pdf_r34,pdf_r5,odt,office] [--seconds S]
"""
import argparse
import contextlib
import io
import json
import os
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

import bench  # noqa: E402
from dprf_amd import _lib, brute_force, hybrid, mask  # noqa: E402

NWORDS = 1 << 16
SEED = 0x4859
HYBRID_MASK = "?w?d?d?d"
MASK = "?l" * 8 + "?d?d?d"


def words():
    rng = random.Random(SEED)
    return [bytes(rng.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(8)) for _ in range(NWORDS)]


def timed(fn, n, calls=1):
    t = time.perf_counter()
    for k in range(calls):
        st = fn(k, n)[2]                            # a call returns after its last result copy
        assert st["candidates"] == n, (st, n)
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="pdf_r34,pdf_r5,odt,office")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build = _lib.build_id()
    S = bench.streams()
    table = words()
    hpos, hat = hybrid.parse_hybrid(HYBRID_MASK)
    mpos = mask.parse_mask(MASK)
    space = hybrid.space(NWORDS, hpos)
    result = {"build": build, "hybrid": HYBRID_MASK, "words": NWORDS, "mask": MASK, "seconds": a.seconds,
              "rounds": a.rounds, "formats": {}}
    for name in a.formats.split(","):
        with contextlib.redirect_stdout(io.StringIO()):
            fields = brute_force.parse_verification_data(S[bench.WORKLOADS[name][0]]["stream"])
        with _lib.Context(fields, device=0) as ctx:
            ctx.set_words(table)
            # consecutive calls take consecutive windows (wrapping inside the hybrid keyspace; the mask's is far larger)
            legs = {"hybrid": lambda k, n: ctx.search_hybrid(hpos, hat, (k * n) % (space - n + 1), n),
                    "mask": lambda k, n: ctx.search_mask(mpos, k * n, n)}
            n = 1 << 16
            while True:                             # grow the window until a mask call runs 0.2 s or fills the keyspace
                dt = timed(legs["mask"], n)
                if dt >= 0.2 or n >= space:
                    break
                n = min(space, int(n * min(16.0, max(2.0, 0.3 / max(dt, 1e-4)))))
            n = max(1 << 16, min(space, int(n * a.seconds / dt)))
            calls = max(1, int(round(a.seconds / max(timed(legs["mask"], n), 1e-4))))
            for fn in legs.values():
                timed(fn, n, calls)                 # warm-up at the timed size
            rates = {leg: [] for leg in legs}
            for _ in range(a.rounds):
                for leg, fn in legs.items():        # alternating: drift of the machine hits both legs alike
                    rates[leg].append(n * calls / timed(fn, n, calls))
        rec = {"kernel": name, "window": n, "calls": calls}
        for leg in legs:
            rec[leg] = statistics.median(rates[leg])
            rec[leg + "_min_max"] = [min(rates[leg]), max(rates[leg])]
        rec["hybrid_vs_mask"] = rec["hybrid"] / rec["mask"]
        result["formats"][name] = rec
        print(json.dumps(rec), flush=True)
    out = a.out or os.path.join(REPO, "profiles", "hybrid_rate_%s.json" % build)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + out, file=sys.stderr)


if __name__ == "__main__":
    main()
