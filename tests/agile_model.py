"""Office 2010 / 2013 Agile Encryption, password key encryptor (MS-OFFCRYPTO 2.3.4.11-2.3.4.13), stated in Python
(TEST INFRASTRUCTURE: the tests' statement of what k_agile_kdf + k_agile_check compute; include/dprf.h "Agile").

Hashes come from hashlib, AES from the oracle's C block primitives (pinned by the FIPS 197 KATs of
tests/test_oracle_kat.py), the CBC chaining is spelled out here.  There is no reference verifier for this format:
the definition is pinned by the public example hashes of hashcat modes 9500 / 9600 (tests/golden/agile_vectors.json,
tests/test_agile_model.py).

Stream fields, as parse_verification_data returns them:
    ["office", version, spinCount, keyBits, saltSize, salt, encryptedVerifierHashInput, encryptedVerifierHashValue[0:32]]
version "2010": H = SHA-1, 20 compared bytes; "2013": H = SHA-512, 32 compared bytes.
"""
import hashlib
import os
import random
import re
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import pyoracle as O  # noqa: E402

BLOCK_KEY_INPUT = bytes.fromhex("fea7d2763b4b9e79")     # 2.3.4.13: encryptedVerifierHashInput
BLOCK_KEY_VALUE = bytes.fromhex("d7aa0f6d3061344e")     # encryptedVerifierHashValue
HASHES = {"2010": (hashlib.sha1, 20), "2013": (hashlib.sha512, 32)}   # version -> (H, compared bytes)


def fields_of(stream_or_fields):
    if not isinstance(stream_or_fields, str):
        return list(stream_or_fields)
    f = re.split(r"\*", stream_or_fields)
    assert re.search(r"\$office\$$", f[0]), f[0]
    f[0] = "office"
    return f


def spun_hash(pw, version, salt, spin):
    """h after the spinCount loop; pw is a str."""
    H = HASHES[str(version)][0]
    h = H(salt + pw.encode("utf-16-le")).digest()
    for i in range(spin):
        h = H(struct.pack("<I", i) + h).digest()
    return h


def derive_keys(pw, version, key_bits, salt, spin, pad=0x36):
    """(key1, key2): H(h || block key) cut to keyBits / 8 bytes, a hash shorter than that padded with 0x36."""
    H = HASHES[str(version)][0]
    kb = key_bits // 8
    h = spun_hash(pw, version, salt, spin)
    out = []
    for bk in (BLOCK_KEY_INPUT, BLOCK_KEY_VALUE):
        k = H(h + bk).digest()[:kb]
        out.append(k + bytes([pad]) * (kb - len(k)))
    return tuple(out)


def cbc_decrypt(key, iv, data):
    out, prev = [], iv
    for i in range(0, len(data), 16):
        ct = data[i:i + 16]
        out.append(bytes(a ^ b for a, b in zip(O.aes_decrypt_block(key, ct), prev)))
        prev = ct
    return b"".join(out)


def cbc_encrypt(key, iv, data):
    out, prev = [], iv
    for i in range(0, len(data), 16):
        prev = O.aes_encrypt_block(key, bytes(a ^ b for a, b in zip(data[i:i + 16], prev)))
        out.append(prev)
    return b"".join(out)


def verifies(stream_or_fields, pw, pad=0x36):
    """The verdict of the definition for the password pw (a str)."""
    f = fields_of(stream_or_fields)
    version, spin, key_bits = f[1], int(f[2]), int(f[3])
    H, n = HASHES[version]
    salt, evi, evh = bytes.fromhex(f[5]), bytes.fromhex(f[6]), bytes.fromhex(f[7])
    assert int(f[4]) == 16 and len(salt) == 16 and len(evi) == 16 and len(evh) == 32
    key1, key2 = derive_keys(pw, version, key_bits, salt, spin, pad)
    vin = cbc_decrypt(key1, salt, evi)
    vhv = cbc_decrypt(key2, salt, evh)
    return H(vin).digest()[:n] == vhv[:n]


def first_message_len(pw):
    """Bytes of salt || UTF16LE(pw): SHA-1 hashes it as two blocks above 55, SHA-512 as one block up to 111."""
    return 16 + len(pw.encode("utf-16-le"))


def make_parts(pw, version, key_bits, spin, seed):
    """(salt, encryptedVerifierHashInput, whole encryptedVerifierHashValue) of a random verifier encrypted under the
    keys derived from pw: what a document's password key encryptor holds."""
    version = str(version)
    H = HASHES[version][0]
    rng = random.Random(seed)
    salt = bytes(rng.getrandbits(8) for _ in range(16))
    verifier = bytes(rng.getrandbits(8) for _ in range(16))
    key1, key2 = derive_keys(pw, version, key_bits, salt, spin)
    hv = H(verifier).digest()
    hv += b"\0" * (-len(hv) % 16)                        # 2.3.4.13: padded to the block size
    return salt, cbc_encrypt(key1, salt, verifier), cbc_encrypt(key2, salt, hv)


def plain_parts(version, seed):
    """(salt, verifier, padded hash value): the plaintexts make_parts draws for this seed, before encryption."""
    H = HASHES[str(version)][0]
    rng = random.Random(seed)
    salt = bytes(rng.getrandbits(8) for _ in range(16))
    verifier = bytes(rng.getrandbits(8) for _ in range(16))
    hv = H(verifier).digest()
    return salt, verifier, hv + b"\0" * (-len(hv) % 16)


def make_parts_from(pw, version, key_bits, spin, salt, verifier, hash_value):
    """make_parts for given plaintexts: any 16-byte verifier and any hash value of whole blocks, encrypted under the
    keys derived from pw -- a document whose stored hash need not be the verifier's (tests/test_verdict_compare.py)."""
    assert len(verifier) == 16 and len(hash_value) % 16 == 0
    key1, key2 = derive_keys(pw, str(version), key_bits, salt, spin)
    return salt, cbc_encrypt(key1, salt, verifier), cbc_encrypt(key2, salt, hash_value)


def stream_of(version, key_bits, spin, salt, evi, evh, name="made.docx"):
    """The verifier stream of the three parts, as office2john prints it (the first 32 bytes of the hash value)."""
    return "%s:$office$*%s*%d*%d*%d*%s*%s*%s" % (name, version, spin, key_bits, 16, salt.hex(), evi.hex(),
                                                 evh.hex()[:64])


def make_stream(pw, version, key_bits, spin, seed, name="made.docx"):
    """The verifier stream of a document protected with pw, as office2john prints it."""
    salt, evi, evh = make_parts(pw, version, key_bits, spin, seed)
    return "%s:$office$*%s*%d*%d*%d*%s*%s*%s" % (name, version, spin, key_bits, 16, salt.hex(), evi.hex(),
                                                 evh.hex()[:64])


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
