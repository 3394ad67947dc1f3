#!/usr/bin/env python3
"""Range-mode rate of the ODF 1.2 family that takes the manifest's PBKDF2 count (odf_aes_sha256, the "$odf$*1*1*"
stream) on one device, beside the "$odt$" stream of the same document (odf_aes256, k_odt_kdf: the yardstick) on the
same build, then at --iterations (100000, what LibreOffice writes today).

The document is bench.py's ODF document with the last bit of its checksum flipped, so every candidate runs the whole
check; the "$odf$*1*1*" streams are that document's checksum, iv, salt and first 1024 encrypted bytes under a count.
For each stream a dprf_search_range window over lowercase^7 is timed, stop_on_first off.  The window is about --seconds
of work at the rate a first call measures, a whole number of the context's first chunks.  Every stream runs its window
once as warm-up; the two 1024-iteration streams are then timed alternately for --rounds rounds, and the --iterations
stream for --rounds rounds after them; medians are reported with their spread.  Per stream the record splits the device
time of the last window into its KDF kernel (main_kernel_ms) and the check kernel (the rest), and gives the SHA-1
compressions per second of the KDF (2 + 4c per candidate, dprf_amd/work.py odf_aes_counts).
Writes profiles/odf_aes_rate_<build>.json (or --out) and prints one JSON line per stream.

Usage (on a machine with the GPU): python tools/bench_odf_aes.py [--seconds S] [--rounds N] [--iterations C]
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
from dprf_amd import _lib, brute_force, work  # noqa: E402

LOWER = "abcdefghijklmnopqrstuvwxyz"
PWLEN = 7
ODT, ODF = "odf_aes256", "odf_aes_sha256"
GENERATION = 256 * 4 * 5 * 64       # the floor of a context's chunks (include/dprf.h): resident lanes of k_odf_aes_kdf


def streams(iterations):
    """(label, family, iterations, stream) of the three timed streams"""
    odt = bench.streams()["odt_testdoc_std"]["stream"].split("*")
    odt[2] = odt[2][:-1] + "%x" % (int(odt[2][-1], 16) ^ 1)            # the checksum, last bit flipped
    assert int(odt[6]) >= 1024
    odf = lambda c: "v:$odf$*1*1*%d*32*%s*16*%s*16*%s*0*%s" % (c, odt[2], odt[3], odt[4], odt[5][:2048])
    return [("odt_1024", ODT, 1024, "*".join(odt)), ("odf_1024", ODF, 1024, odf(1024)),
            ("odf_%d" % iterations, ODF, iterations, odf(iterations))]


def first_chunk(iterations):
    """The first chunk of a context at this count: the 1024-iteration row scaled, not under a generation"""
    row = _lib.plan_chunk(ODF, 0.0, 1 << 40, 1 << 40, 1)
    return row if iterations == 1024 else max(GENERATION, -(-row * 1024 // iterations))


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
    ap.add_argument("--iterations", type=int, default=100000, help="the count of the third stream")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build = _lib.build_id()
    ctxs, window, meta = {}, {}, {}
    space = len(LOWER) ** PWLEN
    try:
        for label, family, c, stream in streams(a.iterations):
            with contextlib.redirect_stdout(io.StringIO()):
                fields = brute_force.parse_verification_data(stream)
            ctx = ctxs[label] = _lib.Context(fields, device=0)
            assert ctx.kernel == family, (ctx.kernel, family)
            chunk = first_chunk(c)
            timed(ctx, chunk)                                   # first touch: module load, buffers
            dt, _ = timed(ctx, chunk)                           # the rate that sizes the window
            meta[label] = (family, c, chunk, dt)
            window[label] = min(space, chunk * max(1, round(a.seconds * (chunk / dt) / chunk)))
            timed(ctx, window[label])                           # warm-up at the timed size
        rates = {n: [] for n in ctxs}
        last = {}
        pair = [n for n in ctxs if meta[n][1] == 1024]
        for _ in range(a.rounds):
            for label in pair:                                  # alternating: drift of the machine hits both alike
                dt, last[label] = timed(ctxs[label], window[label])
                rates[label].append(window[label] / dt)
        for label in ctxs:
            if label not in pair:
                for _ in range(a.rounds):
                    dt, last[label] = timed(ctxs[label], window[label])
                    rates[label].append(window[label] / dt)
    finally:
        for ctx in ctxs.values():
            ctx.close()
    result = {"build": build, "seconds": a.seconds, "rounds": a.rounds, "charset": "lower", "pwlen": PWLEN, "streams": {}}
    for label in ctxs:
        family, c, chunk, chunk_s = meta[label]
        rate = statistics.median(rates[label])
        st, n = last[label], window[label]
        kdf_ms, check_ms = st["main_kernel_ms"], st["kernel_ms"] - st["main_kernel_ms"]
        sha1c = sum(v for k, v in work.odf_aes_counts(c)[1].items() if k.startswith("sha1c"))
        result["streams"][label] = {
            "stream": label, "family": family, "iterations": c, "first_chunk": chunk, "first_chunk_seconds": chunk_s,
            "candidates": n, "launches": st["launches"], "rate": rate,
            "rate_min_max": [min(rates[label]), max(rates[label])],
            "spread": (max(rates[label]) - min(rates[label])) / rate,
            "kernel_ms": st["kernel_ms"], "wall_ms": st["wall_ms"],
            "kdf_ns_per_candidate": kdf_ms * 1e6 / n, "check_ns_per_candidate": check_ms * 1e6 / n,
            "sha1_compressions_per_candidate": sha1c, "sha1_compressions_per_s": rate * sha1c}
    s = result["streams"]
    result["rate_ratio_to_odt_at_1024"] = s["odf_1024"]["rate"] / s["odt_1024"]["rate"]
    result["kdf_time_ratio_to_odt_at_1024"] = s["odf_1024"]["kdf_ns_per_candidate"] / s["odt_1024"]["kdf_ns_per_candidate"]
    for rec in s.values():
        print(json.dumps(rec), flush=True)
    print(json.dumps({"rate_ratio_to_odt_at_1024": result["rate_ratio_to_odt_at_1024"],
                      "kdf_time_ratio_to_odt_at_1024": result["kdf_time_ratio_to_odt_at_1024"]}), flush=True)
    out = a.out or os.path.join(REPO, "profiles", "odf_aes_rate_%s.json" % build)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote " + out, file=sys.stderr)


if __name__ == "__main__":
    main()
