#!/usr/bin/env python3
"""Range-mode rates of the Office 97-2003 RC4 kernel families on one device: office_rc4_md5 (types 0 / 1) and
office_rc4_sha1 (types 3 / 4), on the public example streams of tests/golden/oldoffice_vectors.json with the last
bit of encryptedVerifierHash flipped (their password, "hashcat", lies in lowercase^7; with the stored hash changed no
candidate verifies, and every candidate still runs the whole check), beside pdf_r24 on bench.py's PDF R2 document --
the family whose workgroup shape and KSA k_oldoffice shares -- on the same build.

For each family a no-hit dprf_search_range window over lowercase^7 is timed, stop_on_first off.  The window is about
--seconds of work at the rate a first call measures, a whole number of first chunks of the family's policy
(dprf_plan_chunk).  Every family runs its window once as warm-up; the families are then timed alternately for --rounds
rounds and the median is reported with its spread and its ratio to the R2 rate (DESIGN.md 4e has the instruction-count
account of that ratio).
Writes profiles/oldoffice_rate_<build>.json (or --out) and prints one JSON line per family.

Usage (on a machine with the GPU): python tools/bench_oldoffice.py [--seconds S] [--rounds N]
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
PWLEN = 7
R2 = "pdf_r2"


def no_hit(stream):
    """The stream with the last bit of its last field (encryptedVerifierHash) flipped."""
    return stream[:-1] + "%x" % (int(stream[-1], 16) ^ 1)


def family_streams():
    old = json.load(open(os.path.join(REPO, "tests", "golden", "oldoffice_vectors.json")))
    return [(R2, "pdf_r24", bench.streams()["pdf_testdoc_r2"]["stream"]),
            ("office_rc4_md5", "office_rc4_md5", "v:" + no_hit(old["oldoffice_type1_hashcat"]["stream"])),
            ("office_rc4_sha1", "office_rc4_sha1", "v:" + no_hit(old["oldoffice_type3_hashcat"]["stream"]))]


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
    space = len(LOWER) ** PWLEN
    try:
        for name, family, stream in family_streams():
            with contextlib.redirect_stdout(io.StringIO()):
                fields = brute_force.parse_verification_data(stream)
            ctx = ctxs[name] = _lib.Context(fields, device=0)
            kernels[name] = ctx.kernel
            assert ctx.kernel == family, (ctx.kernel, family)
            chunk = _lib.plan_chunk(family, 0.0, 1 << 40, 1 << 40, 1)
            timed(ctx, chunk)                                   # first touch: module load, buffers
            dt, _ = timed(ctx, chunk)                           # the rate that sizes the window
            window[name] = min(space, chunk * max(1, round(a.seconds * (chunk / dt) / chunk)))
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
              "families": {}}
    r2 = statistics.median(rates[R2])
    for name in ctxs:
        rate = statistics.median(rates[name])
        rec = {"family": name, "kernel": kernels[name], "candidates": window[name], "launches": last[name]["launches"],
               "rate": rate, "rate_min_max": [min(rates[name]), max(rates[name])],
               "spread": (max(rates[name]) - min(rates[name])) / rate,
               "kernel_ms": last[name]["kernel_ms"], "wall_ms": last[name]["wall_ms"],
               "ratio_to_pdf_r2": rate / r2}
        result["families"][name] = rec
        print(json.dumps(rec), flush=True)
    out = a.out or os.path.join(REPO, "profiles", "oldoffice_rate_%s.json" % build)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + out, file=sys.stderr)


if __name__ == "__main__":
    main()
