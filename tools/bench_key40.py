#!/usr/bin/env python3
"""Rates of the 40-bit key search (dprf_search_key40) beside the password range search of the same document, on one
device and one build: PDF R2, PDF R3 with Length 40, Office 97-2003 types 0 / 1 (office_rc4_md5) and type 3
(office_rc4_sha1).

The documents are golden streams with their last hex digit changed, so that neither a key of the timed window nor a
password verifies and every candidate still runs the whole check.  Per family a no-hit dprf_search_key40 window and a
no-hit dprf_search_range window over lowercase^7 are sized for about --seconds of work each, at the rate a first call
measures, a whole number of first chunks of the family's policy (dprf_plan_chunk).  After one warm-up at the timed size
the key search and the password search alternate for --rounds rounds, family after family; medians, spread, the ratio
of the two and 2^40 / rate are reported.
Writes profiles/key40_rate_<build>.json (or --out) and prints one JSON line per family.

Usage (on a machine with the GPU): python tools/bench_key40.py [--seconds S] [--rounds N]
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

from dprf_amd import _lib, brute_force  # noqa: E402

LOWER = "abcdefghijklmnopqrstuvwxyz"
PWLEN = 7
KEY_START = 0x4000000000        # the timed key windows start here: no golden key lies near


def no_hit(stream):
    """The stream with the last bit of its last hex digit flipped."""
    return stream[:-1] + "%x" % (int(stream[-1], 16) ^ 1)


def no_hit_pdf(stream):
    """A PDF stream with one bit of U's first byte flipped (U is field 9; the last field is O, which a key search does
    not read)."""
    f = stream.split("*")
    f[9] = "%x" % (int(f[9][0], 16) ^ 1) + f[9][1:]
    return "*".join(f)


def family_streams():
    golden = os.path.join(REPO, "tests", "golden")
    pdf = json.load(open(os.path.join(golden, "streams.json")))
    old = json.load(open(os.path.join(golden, "oldoffice_vectors.json")))
    return [("pdf_r2", "pdf_r24", no_hit_pdf(pdf["pdf_testdoc_r2"]["stream"])),
            ("pdf_r3_40", "pdf_r24", no_hit_pdf(pdf["pdf_synth_r3_l40_cab"]["stream"])),
            ("office_rc4_md5", "office_rc4_md5", "v:" + no_hit(old["oldoffice_type1_hashcat"]["stream"])),
            ("office_rc4_sha1", "office_rc4_sha1", "v:" + no_hit(old["oldoffice_type3_hashcat"]["stream"]))]


def timed(ctx, mode, n):
    t = time.perf_counter()
    if mode == "key40":
        _, nhits, st = ctx.search_key40(KEY_START, n)
    else:
        _, nhits, st = ctx.search_range(LOWER, PWLEN, 0, n)    # returns after the last result copy
    dt = time.perf_counter() - t
    assert nhits == 0 and st["candidates"] == n, (mode, nhits, st, n)
    return dt, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="length of a timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build = _lib.build_id()
    modes = ("key40", "password")
    limit = {"key40": _lib.KEY40_SPACE - KEY_START, "password": len(LOWER) ** PWLEN}
    ctxs, window = {}, {}
    try:
        for name, family, stream in family_streams():
            with contextlib.redirect_stdout(io.StringIO()):
                fields = brute_force.parse_verification_data(stream)
            ctx = ctxs[name] = _lib.Context(fields, device=0)
            assert ctx.kernel == family, (ctx.kernel, family)
            for mode in modes:
                chunk = _lib.plan_chunk(family + ("_key40" if mode == "key40" else ""), 0.0, 1 << 40, 1 << 40, 1)
                timed(ctx, mode, chunk)                         # first touch: module load, buffers
                dt, _ = timed(ctx, mode, chunk)                 # the rate that sizes the window
                window[name, mode] = min(limit[mode], chunk * max(1, round(a.seconds * (chunk / dt) / chunk)))
                timed(ctx, mode, window[name, mode])            # warm-up at the timed size
        rates = {k: [] for k in window}
        last = {}
        for _ in range(a.rounds):
            for name, ctx in ctxs.items():
                for mode in modes:                              # alternating: drift of the machine hits both alike
                    dt, last[name, mode] = timed(ctx, mode, window[name, mode])
                    rates[name, mode].append(window[name, mode] / dt)
    finally:
        for ctx in ctxs.values():
            ctx.close()
    result = {"build": build, "seconds": a.seconds, "rounds": a.rounds, "charset": "lower", "pwlen": PWLEN,
              "families": {}}
    for name in ctxs:
        rec = {"family": name}
        for mode in modes:
            r = rates[name, mode]
            med = statistics.median(r)
            rec[mode] = {"candidates": window[name, mode], "launches": last[name, mode]["launches"], "rate": med,
                         "rate_min_max": [min(r), max(r)], "spread": (max(r) - min(r)) / med,
                         "kernel_ms": last[name, mode]["kernel_ms"], "wall_ms": last[name, mode]["wall_ms"]}
        rec["ratio_key40_to_password"] = rec["key40"]["rate"] / rec["password"]["rate"]
        rec["seconds_for_2_40"] = _lib.KEY40_SPACE / rec["key40"]["rate"]
        result["families"][name] = rec
        print(json.dumps(rec), flush=True)
    out = a.out or os.path.join(REPO, "profiles", "key40_rate_%s.json" % build)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + out, file=sys.stderr)


if __name__ == "__main__":
    main()
