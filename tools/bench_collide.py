#!/usr/bin/env python3
"""Rates of the password search for a known 40-bit key (dprf_ctx_set_key40) beside the password range search of the same
document, on one device and one build: PDF R2, PDF R3 with Length 40, Office 97-2003 types 0 / 1 (office_rc4_md5) and
type 3 (office_rc4_sha1).

The documents are bench_key40's: golden streams with one bit changed, so that no password of the timed window verifies
and every candidate runs the whole check.  The known key is that of a password outside the window, so the collider hits
nothing either.  Per family the collider and the password search run no-hit windows of lowercase^7 sized for about
--seconds of work each at the rate a first call measures; where the whole space lasts less, the space is searched
several times in a row.  After one warm-up at the timed size the two alternate for --rounds rounds, family after family;
medians, spread, the ratio of the two, the fraction of the spec bound (SURVEY.md 8(d)'s ops per compression at the
78.64 T lane-op peak of DESIGN.md 5) and 2^40 / rate are reported.  Mask mode (?l x 7, the spelled
path) is timed for PDF R2 with a key set, alternating in the same rounds.
Writes profiles/collide_rate_<build>.json (or --out) and prints one JSON line per family.

Usage (on a machine with the GPU): python tools/bench_collide.py [--seconds S] [--rounds N]
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
sys.path.insert(0, os.path.join(REPO, "tests"))

from bench_key40 import LOWER, PWLEN, family_streams  # noqa: E402
from dprf_amd import _lib, brute_force, mask  # noqa: E402
from dprf_amd.work import PEAK_SLOTS_PER_S  # noqa: E402
import key40_model  # noqa: E402

SPACE = len(LOWER) ** PWLEN
OUTSIDE = "Outside-the-window-9"      # its key is the known key: no candidate of lowercase^7 is expected to share it
MASK_FAMILY = "pdf_r2"
# spec-level ops per compression, and the compressions of a 7-character candidate's key derivation
SPEC_OPS = {"md5": 532, "sha1": 1001}
COMPRESSIONS = {"pdf_r2": ("md5", 2), "pdf_r3_40": ("md5", 52), "office_rc4_md5": ("md5", 7),
                "office_rc4_sha1": ("sha1", 2)}


def timed(ctx, mode, n, positions):
    """n candidates from index 0, wrapping to 0 at the end of the space: (seconds, stats of the last call)."""
    t = time.perf_counter()
    left, st = n, None
    while left:
        take = min(left, SPACE)
        if mode == "mask":
            _, nhits, st = ctx.search_mask(positions, 0, take)
        else:
            _, nhits, st = ctx.search_range(LOWER, PWLEN, 0, take)   # returns after the last result copy
        assert nhits == 0 and st["candidates"] == take, (mode, nhits, st, take)
        left -= take
    return time.perf_counter() - t, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="length of a timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build = _lib.build_id()
    positions = mask.parse_mask("?l" * PWLEN)
    ctxs, keys, window = {}, {}, {}

    def select(name, mode):
        ctxs[name].set_key40(None if mode == "password" else keys[name])

    try:
        for name, family, stream in family_streams():
            with contextlib.redirect_stdout(io.StringIO()):
                fields = list(brute_force.parse_verification_data(stream))
            ctx = ctxs[name] = _lib.Context(fields, device=0)
            assert ctx.kernel == family, (ctx.kernel, family)
            keys[name] = key40_model.key_of_password(fields, OUTSIDE)
            for mode in ("collide", "password") + (("mask",) if name == MASK_FAMILY else ()):
                select(name, mode)
                assert ctx.kernel == family + ("" if mode == "password" else "_collide"), ctx.kernel
                chunk = _lib.plan_chunk(ctx.kernel, 0.0, 1 << 40, 1 << 40, 1)
                timed(ctx, mode, chunk, positions)              # first touch: module load, buffers
                dt, _ = timed(ctx, mode, chunk, positions)      # the rate that sizes the window
                window[name, mode] = chunk * max(1, round(a.seconds * (chunk / dt) / chunk))
                timed(ctx, mode, window[name, mode], positions)  # warm-up at the timed size
        rates = {k: [] for k in window}
        last = {}
        for _ in range(a.rounds):
            for name in ctxs:
                for mode in [m for (n, m) in window if n == name]:   # alternating: drift hits both alike
                    select(name, mode)
                    dt, last[name, mode] = timed(ctxs[name], mode, window[name, mode], positions)
                    rates[name, mode].append(window[name, mode] / dt)
    finally:
        for ctx in ctxs.values():
            ctx.close()
    result = {"build": build, "seconds": a.seconds, "rounds": a.rounds, "charset": "lower", "pwlen": PWLEN,
              "space": SPACE, "families": {}}
    for name in ctxs:
        rec = {"family": name, "key": keys[name].hex()}
        for mode in [m for (n, m) in window if n == name]:
            r = rates[name, mode]
            med = statistics.median(r)
            rec[mode] = {"candidates": window[name, mode], "passes_of_the_space": window[name, mode] / SPACE,
                         "launches_last_call": last[name, mode]["launches"], "rate": med,
                         "rate_min_max": [min(r), max(r)], "spread": (max(r) - min(r)) / med}
        alg, ncomp = COMPRESSIONS[name]
        bound = PEAK_SLOTS_PER_S / (ncomp * SPEC_OPS[alg])
        rec["ratio_collide_to_password"] = rec["collide"]["rate"] / rec["password"]["rate"]
        rec["spec"] = {"compressions": "%d %s" % (ncomp, alg), "bound_rate": bound,
                       "fraction": rec["collide"]["rate"] / bound}
        rec["seconds_for_2_40"] = (1 << 40) / rec["collide"]["rate"]
        result["families"][name] = rec
        print(json.dumps(rec), flush=True)
    out = a.out or os.path.join(REPO, "profiles", "collide_rate_%s.json" % build)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + out, file=sys.stderr)


if __name__ == "__main__":
    main()
