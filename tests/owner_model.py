"""The owner-password check of a PDF stream, stated in Python (TEST INFRASTRUCTURE: a helper, not a test).

The reference has no owner verifier, so the library's owner mode (include/dprf.h "owner password") is pinned against
this restatement of ISO 32000-1 Algorithms 3 and 7 and ISO 32000-2 Algorithms 12 and 2.B.  It is built only from the
oracle's KAT-pinned primitives (pyoracle.md5 / rc4 / sha256 / sha384 / sha512 / aes_encrypt_block, tests/
test_oracle_kat.py); for R2-R4 the last step -- "the decrypted bytes pass the user check" -- is pyoracle.Ctx(...)
.verify(x), the reference-pinned verifier, called with the 32 raw bytes.

Cost: about 0.25 s per R6 candidate, under 0.3 ms per candidate for the other revisions.
"""
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import pyoracle as O  # noqa: E402

PAD = bytes.fromhex("28bf4e5e4e758a4164004e56fffa01082e2e00b6d0683e802f0ca9fe6453697a")


def fields_of(stream):
    return O.split_stream(stream) if isinstance(stream, str) else list(stream)


def parse(stream):
    """The PDF stream's fields: R, n (key bytes, R2-R4), O and U as bytes."""
    f = fields_of(stream)
    assert f[0] == "pdf" and len(f) == 12, f[:3]
    R, length = int(f[2]), int(f[3])
    return {"fields": f, "R": R, "n": 5 if R == 2 else length // 8, "U": bytes.fromhex(f[9]), "O": bytes.fromhex(f[11])}


@functools.lru_cache(maxsize=None)
def _ctx(fields):
    return O.Ctx(list(fields))


def _as_bytes(pw):
    return pw.encode("utf-8") if isinstance(pw, str) else bytes(pw)


def owner_key(d, pw):
    """Algorithm 3 a-d: MD5 of the padded password, for R >= 3 fifty more MD5s over all 16 bytes, the first n bytes."""
    h = O.md5((_as_bytes(pw)[:32] + PAD)[:32])
    if d["R"] >= 3:
        for _ in range(50):
            h = O.md5(h)
    return h[:d["n"]]


def owner_decrypts_to(stream, pw):
    """R2-R4: the 32 bytes /O decrypts to under the candidate's owner key (Algorithm 7 a-b)."""
    d = parse(stream)
    assert 2 <= d["R"] <= 4
    key = owner_key(d, pw)
    x = d["O"][:32]
    if d["R"] == 2:
        return O.rc4(key, x)
    for i in range(19, -1, -1):
        x = O.rc4(bytes(k ^ i for k in key), x)
    return x


def _aes_cbc(key, iv, data):
    out, prev = [], iv
    for i in range(0, len(data), 16):
        prev = O.aes_encrypt_block(key, bytes(a ^ b for a, b in zip(data[i:i + 16], prev)))
        out.append(prev)
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def r6_hash(pw, salt, udata):
    """ISO 32000-2 Algorithm 2.B with the owner's udata = U[0:48].  A pure function of three bytes objects, memoised:
    streams that differ only in O[0:32] or O[40:48] (tests/test_verdict_compare.py) share one evaluation."""
    k = O.sha256(pw + salt + udata)
    i = 0
    while True:
        e = _aes_cbc(k[:16], k[16:32], (pw + k + udata) * 64)
        k = (O.sha256, O.sha384, O.sha512)[sum(e[:16]) % 3](e)
        i += 1
        if i >= 64 and e[-1] <= i - 32:
            return k[:32]


def owner_verifies(stream, pw_bytes):
    d = parse(stream)
    pw = _as_bytes(pw_bytes)
    if d["R"] <= 4:
        return bool(_ctx(tuple(d["fields"])).verify(owner_decrypts_to(stream, pw)))
    o, u = d["O"], d["U"]
    assert len(o) >= 48 and len(u) >= 48
    if d["R"] == 5:
        return O.sha256(pw[:127] + o[32:40] + u[:48]) == o[:32]
    return r6_hash(pw, o[32:40], u[:48]) == o[:32]


def compared_bytes(stream, pw):
    """R3/R4: the 16 bytes the check compares with U[0:16] for the owner candidate pw -- the user check's RC4 output
    (pyoracle intermediates [48:64]) for the 32 bytes /O decrypts to.  They do not depend on U."""
    d = parse(stream)
    assert 3 <= d["R"] <= 4
    return _ctx(tuple(d["fields"])).intermediates(owner_decrypts_to(stream, pw))[48:64]


def index_of(pw, charset):
    i = 0
    for ch in pw:
        i = i * len(charset) + charset.index(ch)
    return i


def word(i, charset, n):
    out = []
    for _ in range(n):
        i, r = divmod(i, len(charset))
        out.append(charset[r])
    return "".join(reversed(out))


def window_hits(stream, charset, pwlen, start, count):
    """Indices relative to `start` of the window's candidates that verify as owner."""
    return [k for k in range(count) if owner_verifies(stream, word(start + k, charset, pwlen))]
