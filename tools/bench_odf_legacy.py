#!/usr/bin/env python3
"""Range-mode rate of the ODF 1.0 / 1.1 family (odf_bf_sha1: Blowfish-CFB, SHA-1, iterations 1024) on one device,
beside the ODF 1.2 family (odf_aes256) on the same build.

Both streams are no-hit streams, so every candidate runs the whole check: the ODF 1.0 / 1.1 stream has salt, iv,
content and checksum drawn from SHA-256 (nothing decrypts to that checksum); the ODF 1.2 stream is bench.py's document
with the last bit of its checksum flipped.  For each family a dprf_search_range window over lowercase^7 is timed,
stop_on_first off.  The window is about --seconds of work at the rate a first call measures, a whole number of first
chunks of the family's policy (dprf_plan_chunk).  Every family runs its window once as warm-up; the families are then
timed alternately for --rounds rounds and the median is reported with its spread.  Per family the record also splits
the device time of the last window into its KDF kernel (main_kernel_ms) and its check kernel (the rest), per
candidate, and gives the ratios DESIGN.md 4f discusses: KDF time per candidate against k_odt_kdf's (the compression
counts give 2,050 / 4,098), the check kernel's own candidates per second, and the family rate against ODF 1.2's.
Writes profiles/odf_legacy_rate_<build>.json (or --out) and prints one JSON line per family.

Usage (on a machine with the GPU): python tools/bench_odf_legacy.py [--seconds S] [--rounds N]
"""
import argparse
import contextlib
import hashlib
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
ODT, ODF = "odf_aes256", "odf_bf_sha1"


def _draw(label, n):
    out, k = b"", 0
    while len(out) < n:
        out += hashlib.sha256(("bench_odf_legacy/%s/%d" % (label, k)).encode()).digest()
        k += 1
    return out[:n].hex()


def family_streams(iterations):
    odt = bench.streams()["odt_testdoc_std"]["stream"].split("*")
    odt[2] = odt[2][:-1] + "%x" % (int(odt[2][-1], 16) ^ 1)            # the checksum, last bit flipped
    odf = "v:$odf$*0*0*%d*16*%s*8*%s*16*%s*0*%s" % (iterations, _draw("checksum", 20), _draw("iv", 8),
                                                   _draw("salt", 16), _draw("content", 1024))
    return [(ODT, "*".join(odt)), (ODF, odf)]


def timed(ctx, n):
    t = time.perf_counter()
    _, nhits, st = ctx.search_range(LOWER, PWLEN, 0, n)        # returns after the last result copy
    dt = time.perf_counter() - t
    assert nhits == 0 and st["candidates"] == n, (nhits, st, n)
    return dt, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="length of a timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=1024, help="PBKDF2 count of the ODF 1.0 / 1.1 stream")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build = _lib.build_id()
    ctxs, window = {}, {}
    space = len(LOWER) ** PWLEN
    try:
        for family, stream in family_streams(a.iterations):
            with contextlib.redirect_stdout(io.StringIO()):
                fields = brute_force.parse_verification_data(stream)
            ctx = ctxs[family] = _lib.Context(fields, device=0)
            assert ctx.kernel == family, (ctx.kernel, family)
            chunk = _lib.plan_chunk(family, 0.0, 1 << 40, 1 << 40, 1)
            timed(ctx, chunk)                                   # first touch: module load, buffers
            dt, _ = timed(ctx, chunk)                           # the rate that sizes the window
            window[family] = min(space, chunk * max(1, round(a.seconds * (chunk / dt) / chunk)))
            timed(ctx, window[family])                          # warm-up at the timed size
        rates = {n: [] for n in ctxs}
        last = {}
        for _ in range(a.rounds):
            for family, ctx in ctxs.items():                    # alternating: drift of the machine hits all alike
                dt, last[family] = timed(ctx, window[family])
                rates[family].append(window[family] / dt)
    finally:
        for ctx in ctxs.values():
            ctx.close()
    result = {"build": build, "seconds": a.seconds, "rounds": a.rounds, "charset": "lower", "pwlen": PWLEN,
              "iterations": a.iterations, "families": {}}
    for family in ctxs:
        rate = statistics.median(rates[family])
        st, n = last[family], window[family]
        kdf_ms, check_ms = st["main_kernel_ms"], st["kernel_ms"] - st["main_kernel_ms"]
        result["families"][family] = {
            "family": family, "candidates": n, "launches": st["launches"], "rate": rate,
            "rate_min_max": [min(rates[family]), max(rates[family])],
            "spread": (max(rates[family]) - min(rates[family])) / rate,
            "kernel_ms": st["kernel_ms"], "wall_ms": st["wall_ms"],
            "kdf_ns_per_candidate": kdf_ms * 1e6 / n, "check_ns_per_candidate": check_ms * 1e6 / n,
            "check_rate": n / (check_ms / 1e3) if check_ms > 0 else None}
    f12, f11 = result["families"][ODT], result["families"][ODF]
    result["kdf_time_ratio_to_odf12"] = f11["kdf_ns_per_candidate"] / f12["kdf_ns_per_candidate"]
    result["rate_ratio_to_odf12"] = f11["rate"] / f12["rate"]
    for rec in result["families"].values():
        print(json.dumps(rec), flush=True)
    print(json.dumps({"kdf_time_ratio_to_odf12": result["kdf_time_ratio_to_odf12"],
                      "rate_ratio_to_odf12": result["rate_ratio_to_odf12"]}), flush=True)
    out = a.out or os.path.join(REPO, "profiles", "odf_legacy_rate_%s.json" % build)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + out, file=sys.stderr)


if __name__ == "__main__":
    main()
