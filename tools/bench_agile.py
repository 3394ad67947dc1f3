#!/usr/bin/env python3
"""Range-mode rates of the Office kernel families on one device: office_std (2007 Standard Encryption, bench.py's
document) beside office_agile_sha1 and office_agile_sha512 (Agile Encryption at spinCount 100000: the public example
streams of tests/golden/agile_vectors.json).

For each family a no-hit dprf_search_range window over lowercase^6 is timed, stop_on_first off.  The window is about
--seconds of work at the rate a first call measures, but never less than one first chunk of the family's policy
(dprf_plan_chunk: one resident generation of its KDF kernel -- a smaller launch leaves CUs idle and measures the
machine's fill, not the kernel) and a whole number of them.  Every family runs its window once as warm-up; the families
are then timed alternately for --rounds rounds and the median is reported with its spread, beside the expectation
(DESIGN.md "Office Agile"): the SHA-1 family runs office_std's loop twice as long, so half of office_std's rate on the
same build; the SHA-512 family ~6,800 issue slots per compression x 100,000, on the order of 100 k candidates/s.
Writes profiles/agile_rate_<build>.json (or --out) and prints one JSON line per family.

Usage (on a machine with the GPU): python tools/bench_agile.py [--seconds S] [--rounds N]
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

LOWER = "abcdefghijklmnopqrstuvwxyz"
PWLEN = 6
SHA512_EXPECTED = 100e3      # candidates/s, order of magnitude (6.8e8 issue slots per candidate)


def family_streams():
    agile = json.load(open(os.path.join(REPO, "tests", "golden", "agile_vectors.json")))
    return [("office_std", bench.streams()["office_testdoc"]["stream"]),
            ("office_agile_sha1", "v:" + agile["office_2010_hashcat"]["stream"]),
            ("office_agile_sha512", "v:" + agile["office_2013_hashcat"]["stream"])]


def timed(ctx, n):
    t = time.perf_counter()
    _, nhits, st = ctx.search_range(LOWER, PWLEN, 0, n)        # returns after the last result copy
    dt = time.perf_counter() - t
    assert nhits == 0 and st["candidates"] == n, (nhits, st, n)
    return dt, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="length of a timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build = _lib.build_id()
    ctxs, window, kernels = {}, {}, {}
    try:
        for name, stream in family_streams():
            with contextlib.redirect_stdout(io.StringIO()):
                fields = brute_force.parse_verification_data(stream)
            ctx = ctxs[name] = _lib.Context(fields, device=0)
            kernels[name] = ctx.kernel
            assert ctx.kernel == name, (ctx.kernel, name)
            chunk = _lib.plan_chunk(name, 0.0, 1 << 40, 1 << 40, 1)
            dt, _ = timed(ctx, chunk)                           # first call: the rate that sizes the window
            window[name] = chunk * max(1, round(a.seconds * (chunk / dt) / chunk))
            timed(ctx, window[name])                            # warm-up at the timed size
        rates = {n: [] for n in ctxs}
        last = {}
        for _ in range(a.rounds):
            for name, ctx in ctxs.items():                      # alternating: drift of the machine hits all alike
                dt, last[name] = timed(ctx, window[name])
                rates[name].append(window[name] / dt)
    finally:
        for ctx in ctxs.values():
            ctx.close()
    result = {"build": build, "seconds": a.seconds, "rounds": a.rounds, "charset": "lower", "pwlen": PWLEN,
              "spin_count": 100000, "families": {}}
    std = statistics.median(rates["office_std"])
    expected = {"office_std": None, "office_agile_sha1": std / 2, "office_agile_sha512": SHA512_EXPECTED}
    for name in ctxs:
        rate = statistics.median(rates[name])
        rec = {"family": name, "kernel": kernels[name], "candidates": window[name], "launches": last[name]["launches"],
               "rate": rate, "rate_min_max": [min(rates[name]), max(rates[name])],
               "kdf_fraction": last[name]["main_kernel_ms"] / max(last[name]["kernel_ms"], 1e-9),
               "expected": expected[name],
               "measured_over_expected": rate / expected[name] if expected[name] else None}
        result["families"][name] = rec
        print(json.dumps(rec), flush=True)
    out = a.out or os.path.join(REPO, "profiles", "agile_rate_%s.json" % build)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + out, file=sys.stderr)


if __name__ == "__main__":
    main()
