#!/usr/bin/env python3
"""Rates of mask mode (dprf_search_mask, ABI 8) with a uniform lowercase mask against two calls of the same build over
the same keyspace: ASCII range mode (dprf_search_range) and the device-spelled symbol window (dprf_search_symbols) with
the same characters -- on bench.py's test documents, one device, stop_on_first off.  Each leg's window is sized to
about --seconds at that leg's own rate (the sizing calls double as warm-up of every kernel and buffer the timed calls
use, and one more call at the timed size follows them); the legs are then timed alternately --repeats times and the
median is reported with the spread.  Writes profiles/mask_rate_<build>.json (or --out) and prints one JSON line per
format.

Usage (on a machine with the GPU): python tools/bench_mask.py [--formats odt,office,...] [--seconds S] [--out PATH]
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
from dprf_amd import _lib, brute_force  # noqa: E402

LOWER = brute_force.LOWERCASE
PWLEN = 8                      # 26^8 = 2.1e11 candidates: more than a second of the fastest format
MAX_WINDOW = 1 << 36


def timed(fn, n):
    t = time.perf_counter()
    st = fn(n)[2]                                   # the call returns after its last result copy
    dt = time.perf_counter() - t
    assert st["candidates"] == n, (st, n)
    return dt


def window_for(fn, seconds):
    """Candidates that take about `seconds`: grow a trial window until it runs for 0.2 s, then scale."""
    n = 1 << 16
    while True:
        dt = timed(fn, n)
        if dt >= 0.2 or n >= MAX_WINDOW:
            break
        n = min(MAX_WINDOW, int(n * min(16.0, max(2.0, 0.3 / max(dt, 1e-4)))))
    return max(1 << 16, min(MAX_WINDOW, 26 ** PWLEN, int(n * seconds / dt)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="odt,office,pdf_r34,pdf_r5,pdf_r6")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build = _lib.build_id()
    S = bench.streams()
    result = {"build": build, "mask": "?l" * PWLEN, "seconds": a.seconds, "repeats": a.repeats, "formats": {}}
    for name in a.formats.split(","):
        stream_name = bench.WORKLOADS[name][0]
        with contextlib.redirect_stdout(io.StringIO()):
            fields = brute_force.parse_verification_data(S[stream_name]["stream"])
        with _lib.Context(fields, device=0) as ctx:
            legs = {"range": lambda k: ctx.search_range(LOWER, PWLEN, 0, k),
                    "symbols": lambda k: ctx.search_symbols(LOWER, PWLEN, 0, k),
                    "mask": lambda k: ctx.search_mask([LOWER] * PWLEN, 0, k)}
            n = {leg: window_for(fn, a.seconds) for leg, fn in legs.items()}
            for leg, fn in legs.items():
                timed(fn, n[leg])                   # warm-up at the timed size
            rates = {leg: [] for leg in legs}
            for _ in range(a.repeats):
                for leg, fn in legs.items():        # alternating: drift of the machine hits every leg alike
                    rates[leg].append(n[leg] / timed(fn, n[leg]))
        rec = {"kernel": name, "candidates": n}
        for leg in legs:
            rec[leg] = statistics.median(rates[leg])
            rec[leg + "_min_max"] = [min(rates[leg]), max(rates[leg])]
        rec["mask_vs_symbols"] = rec["mask"] / rec["symbols"]
        rec["mask_vs_range"] = rec["mask"] / rec["range"]
        result["formats"][name] = rec
        print(json.dumps(rec), flush=True)
    out = a.out or os.path.join(REPO, "profiles", "mask_rate_%s.json" % build)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + out, file=sys.stderr)


if __name__ == "__main__":
    main()
