"""ODF 1.0 / 1.1 password verification (Blowfish-CFB, SHA-1) as a Python statement of the definition in include/dprf.h
("ODF 1.0/1.1"): the model the device results and the parser are compared with.

    sk  = SHA1(pw)
    key = PBKDF2-HMAC-SHA1(P = sk, S = salt, c = iterations, dkLen = 16)
    pt  = Blowfish-CFB64-decrypt(key, iv, content[0:1024])
    the candidate verifies when SHA1(pt) == checksum

SHA-1 and PBKDF2 come from hashlib.  Blowfish is stated here, over initial subkeys this module computes itself (the
hexadecimal digits of pi, by a Machin-like formula other than the generator's): it reads nothing from
dprf_amd/csrc/blowfish_init.h.  tests/test_odf_legacy_model.py pins the words, the zero-key vector, and key schedule
and CFB output against libcrypto.

The stream is John's odf2john / hashcat 18600 spelling:
    $odf$*0*0*<iterations>*16*<checksum, 40 hex>*8*<iv, 16 hex>*16*<salt, 32 hex>*0*<content, 2048 hex>
"""
import hashlib
import struct

M32 = 0xffffffff
NWORDS = 18 + 4 * 256
CONTENT = 1024


def _atan_inv(x, one):
    total = term = one // x
    x2, k = x * x, 1
    while term:
        term //= x2
        total += (term // (2 * k + 1)) * (-1 if k & 1 else 1)
        k += 1
    return total


_INIT = None


def init_words():
    """the first 18 + 1024 words of pi's fractional part: pi / 4 = 12 atan(1/18) + 8 atan(1/57) - 5 atan(1/239)"""
    global _INIT
    if _INIT is None:
        bits, guard = 32 * NWORDS, 96
        one = 1 << (bits + guard)
        pi = 4 * (12 * _atan_inv(18, one) + 8 * _atan_inv(57, one) - 5 * _atan_inv(239, one))
        frac = (pi - 3 * one) >> guard
        _INIT = tuple((frac >> (bits - 32 * (i + 1))) & M32 for i in range(NWORDS))
    return _INIT


class Blowfish:
    """Blowfish with a key of 1..56 bytes: .P (18 words) and .S (4 x 256 words) after the key schedule"""

    def __init__(self, key):
        w = init_words()
        self.P = list(w[:18])
        self.S = [list(w[18 + 256 * k:18 + 256 * (k + 1)]) for k in range(4)]
        if key:
            for i in range(18):
                kw = 0
                for j in range(4):
                    kw = (kw << 8) | key[(4 * i + j) % len(key)]
                self.P[i] ^= kw
        l = r = 0
        for i in range(0, 18, 2):
            l, r = self.encrypt(l, r)
            self.P[i], self.P[i + 1] = l, r
        for k in range(4):
            for i in range(0, 256, 2):
                l, r = self.encrypt(l, r)
                self.S[k][i], self.S[k][i + 1] = l, r

    def _f(self, x):
        S = self.S
        return ((((S[0][x >> 24] + S[1][(x >> 16) & 255]) & M32) ^ S[2][(x >> 8) & 255]) + S[3][x & 255]) & M32

    def encrypt(self, l, r):
        P = self.P
        for i in range(16):
            l ^= P[i]
            r ^= self._f(l)
            l, r = r, l
        l, r = r, l
        return l ^ P[17], r ^ P[16]

    def encrypt_block(self, block):
        l, r = struct.unpack(">II", block)
        return struct.pack(">II", *self.encrypt(l, r))

    def state_words(self):
        """P then S[0..3], the order of libcrypto's BF_KEY"""
        return self.P + [v for s in self.S for v in s]


def cfb64(bf, iv, data, decrypt):
    """CFB with 64-bit feedback over whole blocks (len(data) a multiple of 8): only the encrypt direction is used"""
    out, prev = [], iv
    for o in range(0, len(data), 8):
        blk = data[o:o + 8]
        res = bytes(a ^ b for a, b in zip(blk, bf.encrypt_block(prev)))
        out.append(res)
        prev = blk if decrypt else res
    return b"".join(out)


def _bytes(pw):
    return pw.encode("utf-8") if isinstance(pw, str) else bytes(pw)


def derive_key(pw, salt, iterations):
    return hashlib.pbkdf2_hmac("sha1", hashlib.sha1(_bytes(pw)).digest(), salt, iterations, 16)


def _rand(seed, label, n):
    out, k = b"", 0
    while len(out) < n:
        out += hashlib.sha256(("%s/%s/%d" % (seed, label, k)).encode()).digest()
        k += 1
    return out[:n]


def format_stream(iterations, checksum, iv, salt, content):
    return "$odf$*0*0*%d*16*%s*8*%s*16*%s*0*%s" % (iterations, checksum.hex(), iv.hex(), salt.hex(), content.hex())


def encrypt_entry(pw, iterations, salt, iv, plain):
    """(checksum, ciphertext) of an entry's (deflated) bytes: SHA1/1K over the first 1024, Blowfish-CFB of them all (a
    trailing partial block is XORed with the leading bytes of the next keystream block)"""
    bf = Blowfish(derive_key(pw, salt, iterations))
    pad = -len(plain) % 8
    ct = cfb64(bf, iv, plain + b"\0" * pad, decrypt=False)[:len(plain)]
    return hashlib.sha1(plain[:CONTENT]).digest(), ct


def make_stream(pw, iterations=1024, seed=0):
    """a stream that `pw` verifies: salt, iv and 1024 plaintext bytes drawn from `seed`"""
    salt, iv, plain = _rand(seed, "salt", 16), _rand(seed, "iv", 8), _rand(seed, "plain", CONTENT)
    checksum, ct = encrypt_entry(pw, iterations, salt, iv, plain)
    return format_stream(iterations, checksum, iv, salt, ct)


def split_stream(stream):
    """[cipher, checksum type, iterations, key size, checksum, iv length, iv, salt length, salt, inplace, content]"""
    body = stream[stream.index("$odf$*") + 6:].split(":::", 1)[0]
    f = body.split("*")
    assert len(f) == 11 and f[0] == "0" and f[1] == "0" and f[3] == "16" and f[5] == "8" and f[7] == "16", f[:4]
    return f


def verifies(stream, pw):
    f = split_stream(stream)
    iterations, checksum = int(f[2]), bytes.fromhex(f[4])
    iv, salt, content = bytes.fromhex(f[6]), bytes.fromhex(f[8]), bytes.fromhex(f[10])
    assert len(checksum) == 20 and len(iv) == 8 and len(salt) == 16 and len(content) == CONTENT
    bf = Blowfish(derive_key(pw, salt, iterations))
    return hashlib.sha1(cfb64(bf, iv, content, decrypt=True)).digest() == checksum


def hits(stream, candidates):
    """indices of the candidates that verify"""
    return [k for k, pw in enumerate(candidates) if verifies(stream, pw)]


def word(idx, charset, n):
    """candidate `idx` of the n-character range over `charset` in itertools.product order"""
    out = []
    for _ in range(n):
        out.append(charset[idx % len(charset)])
        idx //= len(charset)
    return "".join(reversed(out))


def index_of(pw, charset):
    idx = 0
    for ch in pw:
        idx = idx * len(charset) + charset.index(ch)
    return idx
