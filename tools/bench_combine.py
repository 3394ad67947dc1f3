#!/usr/bin/env python3
"""Rates of combinator mode (dprf_search_combine: a left word table times a right one, k_spell_combine) against hybrid
mode of the same build (dprf_search_hybrid, k_spell_hybrid) over candidates of the same number and length -- on
bench.py's test documents, one device, stop_on_first off, no hit in either window.

  combine  2^13 x 2^13 generated words of 8 + 3 bytes (keyspace 67,108,864)
  hybrid   "?w?d?d?d" over 2^16 generated 8-letter words (keyspace 65,536,000): 11 bytes per candidate as well

Each timed leg is `calls` library calls of `window` candidates, the same for both legs of a format, sized to about
--seconds at the format's hybrid rate (the keyspaces cap a call at 65,536,000 candidates, which the fastest format
verifies in milliseconds: hence several calls per leg).  The sizing calls double as warm-up; the two legs are then timed
alternately --rounds times and the medians reported with the spread.  Per leg the record also holds
1 - kernel_ms / wall_ms of its calls: the part of a call that is not the verification kernels' event time -- the
spelling kernel, and the launch gaps with it, so an upper bound of the spelling kernel's share (the event times of
PDF R2-R4, whose launches alternate between two streams, overlap and are not comparable).  Writes
profiles/combine_rate_<build>.json (or --out) and prints one JSON line per format.

Usage (on a machine with the GPU): python tools/bench_combine.py [--formats pdf_r2,pdf_r34,pdf_r5,odt,office] [--seconds S]
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
from dprf_amd import _lib, brute_force, combine, hybrid  # noqa: E402

NSIDE = 1 << 13
NWORDS = 1 << 16
SEED = 0x434F
HYBRID_MASK = "?w?d?d?d"
UPPER = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"


def tables():
    """(left, right, hybrid words): 2^13 words of 8 letters, 2^13 of 3 digits-or-letters, 2^16 words of 8 letters."""
    rng = random.Random(SEED)
    word = lambda n, alpha: bytes(rng.choice(alpha) for _ in range(n))
    left = [word(8, UPPER) for _ in range(NSIDE)]
    right = [word(3, UPPER + b"0123456789") for _ in range(NSIDE)]
    return left, right, [word(8, UPPER) for _ in range(NWORDS)]


def timed(fn, n, calls=1):
    """(seconds, 1 - kernel_ms / wall_ms over the calls)"""
    t = time.perf_counter()
    kernel = wall = 0.0
    for k in range(calls):
        st = fn(k, n)[2]                            # a call returns after its last result copy
        assert st["candidates"] == n, (st, n)
        kernel += st["kernel_ms"]
        wall += st["wall_ms"]
    return time.perf_counter() - t, 1.0 - kernel / max(wall, 1e-9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="pdf_r2,pdf_r34,pdf_r5,odt,office")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build = _lib.build_id()
    S = bench.streams()
    left, right, words = tables()
    hpos, hat = hybrid.parse_hybrid(HYBRID_MASK)
    hspace = hybrid.space(NWORDS, hpos)
    cspace = combine.space(len(left), len(right))
    space = min(hspace, cspace)
    result = {"build": build, "combine": [len(left), len(right)], "hybrid": HYBRID_MASK, "words": NWORDS,
              "seconds": a.seconds, "rounds": a.rounds, "formats": {}}
    for name in a.formats.split(","):
        with contextlib.redirect_stdout(io.StringIO()):
            fields = brute_force.parse_verification_data(S[bench.WORKLOADS[name][0]]["stream"])
        # one context per leg: each holds its own left table
        with _lib.Context(fields, device=0) as hctx, _lib.Context(fields, device=0) as cctx:
            hctx.set_words(words)
            cctx.set_words(left)
            cctx.set_right_words(right)
            # consecutive calls take consecutive windows, wrapping inside the keyspace
            legs = {"combine": lambda k, n: cctx.search_combine((k * n) % (cspace - n + 1), n),
                    "hybrid": lambda k, n: hctx.search_hybrid(hpos, hat, (k * n) % (hspace - n + 1), n)}
            n = 1 << 16
            while True:                             # grow the window until a hybrid call runs 0.2 s or fills the keyspace
                dt = timed(legs["hybrid"], n)[0]
                if dt >= 0.2 or n >= space:
                    break
                n = min(space, int(n * min(16.0, max(2.0, 0.3 / max(dt, 1e-4)))))
            n = max(1 << 16, min(space, int(n * a.seconds / dt)))
            calls = max(1, int(round(a.seconds / max(timed(legs["hybrid"], n)[0], 1e-4))))
            for fn in legs.values():
                timed(fn, n, calls)                 # warm-up at the timed size
            rates = {leg: [] for leg in legs}
            other = {leg: [] for leg in legs}
            for _ in range(a.rounds):
                for leg, fn in legs.items():        # alternating: drift of the machine hits both legs alike
                    dt, share = timed(fn, n, calls)
                    rates[leg].append(n * calls / dt)
                    other[leg].append(share)
        rec = {"kernel": name, "window": n, "calls": calls}
        for leg in legs:
            rec[leg] = statistics.median(rates[leg])
            rec[leg + "_min_max"] = [min(rates[leg]), max(rates[leg])]
            rec[leg + "_not_verifying"] = statistics.median(other[leg])
        rec["combine_vs_hybrid"] = rec["combine"] / rec["hybrid"]
        result["formats"][name] = rec
        print(json.dumps(rec), flush=True)
    out = a.out or os.path.join(REPO, "profiles", "combine_rate_%s.json" % build)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + out, file=sys.stderr)


if __name__ == "__main__":
    main()
