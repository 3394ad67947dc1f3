#!/usr/bin/env python3
"""Owner-password search rates against user-password rates (dprf_ctx_set_pdf_password, ABI 9), per PDF kernel family.

For each family a no-hit dprf_search_range window over bench.py's document, charset and length is timed in owner mode
and in user mode on the SAME context, one device, stop_on_first off.  The window is grown until a call takes at least
--min-launches launches (or, with --max-seconds, until it runs that long: R6's launches take seconds each), both modes
run it once as warm-up, and the two modes are then timed alternately for --rounds rounds.  Reported per family: the
median rate of each mode with its spread, their ratio, the launches of a timed call, and the ratio the algorithms
predict (DESIGN.md "Owner password").  Writes profiles/owner_rates_<build>.json (or --out) and prints one JSON line
per family.

With --window mask the same keyspace is searched as a uniform mask spelled on the device (dprf_search_mask): the
list-mode instantiations of the same kernels, user and owner.

Usage (on a machine with the GPU): python tools/bench_owner.py [--families pdf_r34,pdf_r2,...] [--max-seconds S]
                                                                [--window mask]
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

# owner / user rate the algorithms predict (DESIGN.md "Owner password": KSA and PRGA steps, SHA-256 blocks, period bytes)
EXPECTED = {"pdf_r34": 0.47, "pdf_r3": 0.47, "pdf_r3_40": 0.47, "pdf_r2": 0.47, "pdf_r5": 0.5, "pdf_r6": 0.53}
MODES = ("owner", "user")


def timed(ctx, charset, pwlen, n, window="range"):
    """One timed call: a range window, or ("mask") the same keyspace as a device-spelled uniform mask, which the
    list-mode instantiation of the kernel verifies."""
    t = time.perf_counter()
    if window == "mask":
        _, nhits, st = ctx.search_mask([charset] * pwlen, 0, n)
    else:
        _, nhits, st = ctx.search_range(charset, pwlen, 0, n)  # returns after the last result copy
    dt = time.perf_counter() - t
    assert nhits == 0 and st["candidates"] == n, (nhits, st, n)
    return dt, st["launches"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", default="pdf_r34,pdf_r3_40,pdf_r2,pdf_r5,pdf_r6")
    ap.add_argument("--min-launches", type=int, default=20)
    ap.add_argument("--max-seconds", type=float, default=0.0,
                    help="stop growing the window once a call runs this long, whatever its launches (0: no cap)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", default="range", choices=["range", "mask"],
                    help="the call that is timed: a range window, or the same keyspace as a uniform mask (list-mode kernels)")
    a = ap.parse_args()
    build = _lib.build_id()
    S = bench.streams()
    result = {"build": build, "min_launches": a.min_launches, "max_seconds": a.max_seconds, "rounds": a.rounds,
              "window": a.window, "families": {}}
    for name in a.families.split(","):
        stream_name, charset, pwlen = bench.WORKLOADS[name][:3]
        with contextlib.redirect_stdout(io.StringIO()):
            fields = brute_force.parse_verification_data(S[stream_name]["stream"])
        space = len(charset) ** pwlen
        with _lib.Context(fields, device=0) as ctx:
            # the window: grown on the slower mode until a call has enough launches (or runs long enough)
            ctx.set_pdf_password("owner")
            n = 1 << 20
            while True:
                dt, launches = timed(ctx, charset, pwlen, n, a.window)
                if launches >= a.min_launches or n >= space or (a.max_seconds and dt >= a.max_seconds):
                    break
                grow = 2.0 if not a.max_seconds else min(2.0, max(1.1, a.max_seconds / max(dt, 1e-3)))
                n = min(space, int(n * grow))
            for mode in MODES:                                  # warm-up of both modes at the timed size
                ctx.set_pdf_password(mode)
                timed(ctx, charset, pwlen, n, a.window)
            rates = {m: [] for m in MODES}
            launches = {}
            kernels = {}
            for _ in range(a.rounds):
                for mode in MODES:                              # alternating: drift of the machine hits both alike
                    ctx.set_pdf_password(mode)
                    kernels[mode] = ctx.kernel
                    dt, launches[mode] = timed(ctx, charset, pwlen, n, a.window)
                    rates[mode].append(n / dt)
        rec = {"family": name, "stream": stream_name, "pwlen": pwlen, "candidates": n, "launches": launches,
               "kernels": kernels, "expected_ratio": EXPECTED.get(name)}
        for mode in MODES:
            rec[mode] = statistics.median(rates[mode])
            rec[mode + "_min_max"] = [min(rates[mode]), max(rates[mode])]
        rec["owner_vs_user"] = rec["owner"] / rec["user"]
        result["families"][name] = rec
        print(json.dumps(rec), flush=True)
    out = a.out or os.path.join(REPO, "profiles", "owner_rates_%s.json" % build)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + out, file=sys.stderr)


if __name__ == "__main__":
    main()
