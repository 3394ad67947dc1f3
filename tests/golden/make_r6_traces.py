#!/usr/bin/env python3
"""PDF R6 passwords chosen by the trace of their hardened hash, from the project's own ORACLE.

The R6 hash runs a data-dependent number of rounds: after n rounds it ends when n >= 64 and the round's last ciphertext
byte is at most n - 32.  A planted password exercises the exit rule at its equality edge only by luck (about 1 in 40),
so this scans a range-mode window with pyoracle.pdf_r6_trace_range and records one index per stratum:

  user (salt U[32:40])
    S1  64 rounds, final byte exactly 32                 the rule's equality edge at the first exit
    S2  64 rounds, final byte 0
    S3  65 rounds, the byte after 64 rounds exactly 33   misses the first exit by one
    S4  more than 64 rounds, final byte exactly rounds - 32
    S5  after some n >= 64 rounds (n > 64 where the scan has one) the byte is exactly n - 31: goes on by one
    S6  the three longest traces of the scan
  owner (salt O[32:40], udata U[0:48] of the same stream)
    S1, S4

The hash does not depend on the 32 bytes it is compared with, so tests/r6_plant.py makes any of these the password of
the base stream by writing its hash into U[0:32] (O[0:32] for the owner).  The base stream is tests/golden/docs.json's
pdf_r6.pdf, copied into the fixture in full; the charset and the scan sizes are recorded with the largest round count
seen.  Needs no reference build.

    python tests/golden/make_r6_traces.py [log2 of the user scan, default 17]   -> tests/golden/r6_traces.json

About 50 hashes a second and thread: 2^17 indices take some 40 minutes on one thread.

What the longest traces can and cannot show: the kernels keep a slot's round count in 14 bits of state[] (k_pdf_r6:
(st >> 16) & 0x3fff).  The count cannot pass 32 + 255 = 287 by the exit rule itself, so the field is wide enough by
construction; S6 only shows that counts well past 64 (109 in the committed scan, 1 candidate in 13,000 reaches 104) are
carried right.  128 rounds or more need a run of 64 bytes each above its own rising bound -- about 1e-8 per candidate,
out of reach of a scan a fixture can afford -- and no value beyond the recorded maximum is promised.
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import pyoracle as O  # noqa: E402

CHARSET = "abcdefghijklmnop"
PWLEN = 6
OWNER_SCAN = 1 << 12
CHUNK = 1 << 12


def scan(salt, udata, count, nthreads):
    rounds, final, edge = [], [], []
    t0 = time.time()
    for s in range(0, count, CHUNK):
        r, f, e = O.pdf_r6_trace_range(salt, CHARSET, PWLEN, s, min(CHUNK, count - s), udata, nthreads)
        rounds += r
        final += f
        edge += e
        print("  %7d / %d  %.0f s  max %d" % (len(rounds), count, time.time() - t0, max(rounds)), flush=True)
    return rounds, final, edge


def first(pred, n):
    for k in range(n):
        if pred(k):
            return k
    raise SystemExit("stratum not found in the scan: enlarge it")


def main():
    log2 = int(sys.argv[1]) if len(sys.argv) > 1 else 17
    assert log2 >= 17, "S6 needs a trace of 104 rounds or more: about one candidate in 20,000"
    nthreads = os.cpu_count() or 1
    stream = json.load(open(os.path.join(HERE, "docs.json")))["pdf_r6.pdf"]["streams"]["std"]["stream"]
    f = O.split_stream(stream)
    assert f[0] == "pdf" and f[2] == "6"
    U, Ob = bytes.fromhex(f[9]), bytes.fromhex(f[11])
    entries = []

    def add(mode, stratum, k, rounds, final, edge):
        entries.append(dict(name="%s-%s" % (mode, stratum), mode=mode, stratum=stratum, index=k,
                            password=O.index_to_password(k, CHARSET, PWLEN), rounds=rounds[k], final=final[k],
                            edge=edge[k]))

    n = 1 << log2
    r, fb, e = scan(U[32:40], b"", n, nthreads)
    add("user", "S1", first(lambda k: r[k] == 64 and fb[k] == 32, n), r, fb, e)
    add("user", "S2", first(lambda k: r[k] == 64 and fb[k] == 0, n), r, fb, e)
    add("user", "S3", first(lambda k: r[k] == 65 and e[k] == 64, n), r, fb, e)
    add("user", "S4", first(lambda k: r[k] > 64 and fb[k] == r[k] - 32, n), r, fb, e)
    late = [k for k in range(n) if e[k] > 64]
    add("user", "S5", late[0] if late else first(lambda k: e[k] >= 64, n), r, fb, e)
    longest = sorted(range(n), key=lambda k: (-r[k], k))[:3]
    for j, k in enumerate(longest):
        add("user", "S6%s" % "abc"[j], k, r, fb, e)
    assert r[longest[0]] >= 104, "the longest trace has %d rounds: enlarge the scan" % r[longest[0]]
    user_max = r[longest[0]]

    ro, fo, eo = scan(Ob[32:40], U[:48], OWNER_SCAN, nthreads)
    add("owner", "S1", first(lambda k: ro[k] == 64 and fo[k] == 32, OWNER_SCAN), ro, fo, eo)
    add("owner", "S4", first(lambda k: ro[k] > 64 and fo[k] == ro[k] - 32, OWNER_SCAN), ro, fo, eo)

    hist = {}
    for x in r:
        hist[x] = hist.get(x, 0) + 1
    out = dict(stream=stream, charset=CHARSET, pwlen=PWLEN,
               scan=dict(user=[0, n], owner=[0, OWNER_SCAN]),
               max_rounds=dict(user=user_max, owner=max(ro)),
               user_rounds_at_least={str(t): sum(c for x, c in hist.items() if x >= t) for t in (64, 65, 80, 88, 96, 104, 112)},
               user_rounds_exactly_64=hist.get(64, 0),
               entries=entries)
    json.dump(out, open(os.path.join(HERE, "r6_traces.json"), "w"), indent=1)
    for en in entries:
        print(en)
    print("max rounds: user %d, owner %d" % (user_max, max(ro)))


if __name__ == "__main__":
    main()
