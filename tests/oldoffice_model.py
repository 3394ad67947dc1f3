"""Office 97-2003 RC4 (MS-OFFCRYPTO 2.3.6) and RC4 CryptoAPI (2.3.5) password verification, stated in Python
(TEST INFRASTRUCTURE: the tests' statement of what k_oldoffice computes; include/dprf.h "Office 97-2003").

Hashes come from hashlib, RC4 is the ten lines below.  There is no reference verifier for this stream: the definition
is pinned by the public example hashes of hashcat modes 9700 / 9800 (tests/golden/oldoffice_vectors.json,
tests/test_oldoffice_model.py).

Stream fields, as parse_verification_data returns them:
    ["oldoffice", type, salt, encryptedVerifier, encryptedVerifierHash]
type 0 / 1: MD5, 40-bit RC4 key material in a 16-byte key, 16 compared bytes; type 3 / 4: SHA-1, a 40-bit key
zero-extended to 16 bytes / a 128-bit key, 20 compared bytes.
"""
import hashlib
import random
import re

TYPES = (0, 1, 3, 4)


def rc4(key, data):
    S, j = list(range(256)), 0
    for i in range(256):
        j = (j + S[i] + key[i % len(key)]) & 255
        S[i], S[j] = S[j], S[i]
    out, i, j = bytearray(), 0, 0
    for b in data:
        i = (i + 1) & 255
        j = (j + S[i]) & 255
        S[i], S[j] = S[j], S[i]
        out.append(b ^ S[(S[i] + S[j]) & 255])
    return bytes(out)


def fields_of(stream_or_fields):
    """The five fields of either spelling ($oldoffice$<t>*... or $oldoffice$*<t>*...), a :::tail cut off."""
    if not isinstance(stream_or_fields, str):
        return list(stream_or_fields)
    f = re.split(r"\*", stream_or_fields)
    m = re.search(r"\$oldoffice\$([^*]*)$", f[0])
    assert m, f[0]
    f = ["oldoffice"] + ([m.group(1)] if m.group(1) else []) + f[1:]
    f[-1] = f[-1].split(":::", 1)[0]
    assert len(f) == 5, f
    return f


def derive_key(pw, typ, salt):
    """The 16-byte RC4 key of block 0 for the password pw (a str)."""
    pw16 = pw.encode("utf-16-le", "surrogatepass")
    if typ in (0, 1):
        h = hashlib.md5(pw16).digest()
        h = hashlib.md5((h[:5] + salt) * 16).digest()
        return hashlib.md5(h[:5] + b"\0\0\0\0").digest()
    h = hashlib.sha1(salt + pw16).digest()
    k = hashlib.sha1(h + b"\0\0\0\0").digest()
    return k[:5] + b"\0" * 11 if typ == 3 else k[:16]


def hash_of(typ):
    return (hashlib.md5, 16) if typ in (0, 1) else (hashlib.sha1, 20)


def verifies(stream_or_fields, pw):
    """The verdict of the definition for the password pw (a str)."""
    f = fields_of(stream_or_fields)
    typ = int(f[1])
    assert typ in TYPES
    H, n = hash_of(typ)
    salt, ev, evh = bytes.fromhex(f[2]), bytes.fromhex(f[3]), bytes.fromhex(f[4])
    assert len(salt) == 16 and len(ev) == 16 and len(evh) == n
    d = rc4(derive_key(pw, typ, salt), ev + evh)
    return H(d[:16]).digest() == d[16:16 + n]


def make_parts(pw, typ, seed):
    """(salt, encryptedVerifier, encryptedVerifierHash): a random salt and verifier from the seed, the verifier and its
    hash RC4-encrypted as one keystream under the key derived from pw."""
    rng = random.Random(seed)
    salt = bytes(rng.getrandbits(8) for _ in range(16))
    verifier = bytes(rng.getrandbits(8) for _ in range(16))
    H, n = hash_of(typ)
    c = rc4(derive_key(pw, typ, salt), verifier + H(verifier).digest())
    return salt, c[:16], c[16:16 + n]


def stream_of(typ, salt, ev, evh, name="made.doc", spelling="john"):
    """office2john's spelling (the type glued to the tag), or hashcat's with a '*' between them."""
    return "%s:$oldoffice$%s%d*%s*%s*%s" % (name, "" if spelling == "john" else "*", typ, salt.hex(), ev.hex(), evh.hex())


def make_stream(pw, typ, seed, name="made.doc", spelling="john"):
    """The verifier stream of a document protected with pw, as office2john prints it."""
    return stream_of(typ, *make_parts(pw, typ, seed), name=name, spelling=spelling)


def index_of(pw, charset):
    idx = 0
    for ch in pw:
        idx = idx * len(charset) + charset.index(ch)
    return idx


def word(idx, charset, n):
    out = []
    for _ in range(n):
        out.append(charset[idx % len(charset)])
        idx //= len(charset)
    return "".join(reversed(out))
