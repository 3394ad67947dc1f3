"""Make any password the password of one PDF R6 stream (TEST INFRASTRUCTURE: a helper, not a test).

The R6 hardened hash of a candidate depends on the candidate, on the salt U[32:40] and, for the owner password, on
O[32:40] and U[0:48] -- not on the 32 bytes it is compared with.  Writing the hash of pw into U[0:32] (O[0:32] for the
owner) of a base stream therefore gives a document whose user (owner) password is pw, at the cost of one CPU hash
(pyoracle.pdf_r6_trace, pinned against Ctx.intermediates and owner_model.r6_hash in tests/test_r6_trace_model.py).
The base stream is the one tests/golden/r6_traces.json carries.
"""
import functools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import pyoracle as O  # noqa: E402

MAX_LEN = 176          # the longest R6 candidate the reference verifies (oracle.c verify_pdf)
OWNER_MAX_LEN = 64     # the longest owner candidate the library takes (include/dprf.h)


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(HERE, "golden", "r6_traces.json")) as f:
        return json.load(f)


def base_fields():
    return O.split_stream(fixture()["stream"])


def _as_bytes(pw):
    return pw.encode("utf-8") if isinstance(pw, str) else bytes(pw)


def trace(fields, pw, which="user"):
    """(hash32, [(bs, last byte) per round]) of pw on this stream's salts."""
    assert fields[0] == "pdf" and fields[2] == "6" and which in ("user", "owner")
    U, Ob = bytes.fromhex(fields[9]), bytes.fromhex(fields[11])
    assert len(U) >= 48 and len(Ob) >= 48
    if which == "user":
        return O.pdf_r6_trace(_as_bytes(pw), U[32:40])
    return O.pdf_r6_trace(_as_bytes(pw), Ob[32:40], U[:48])


def plant(base, pw, which="user", hash32=None):
    """The fields of `base` with U[0:32] (which="user") or O[0:32] ("owner") replaced by pw's hash: pw becomes that
    password of the stream.  hash32: the hash if the caller has it already (it must be trace(base, pw, which)[0])."""
    h = hash32 if hash32 is not None else trace(base, pw, which)[0]
    assert len(h) == 32
    out = list(base)
    k = 9 if which == "user" else 11
    out[k] = h.hex() + out[k][64:]
    return out


def length_word(L):
    """L printable ASCII bytes, a function of L alone; for L >= 1 the first byte differs from length_word(L + 1)'s, so
    no word is a prefix of the next."""
    return bytes(33 + (11 * L + 7 * k + k * k) % 94 for k in range(L))


@functools.lru_cache(maxsize=None)
def length_words(which="user"):
    """(words, hashes): length_word(L) for L = 0..176 (user) or 1..64 (owner) with their hashes on the base stream,
    computed once (about 20 ms each)."""
    lens = range(0, MAX_LEN + 1) if which == "user" else range(1, OWNER_MAX_LEN + 1)
    words = tuple(length_word(L) for L in lens)
    base = base_fields()
    return words, tuple(trace(base, w, which)[0] for w in words)
