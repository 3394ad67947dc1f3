"""tests/odf_legacy_model.py, the Python statement of ODF 1.0 / 1.1 verification (include/dprf.h "ODF 1.0/1.1"), pinned:
Blowfish's initial words against the known digits of pi and against dprf_amd/csrc/blowfish_init.h (what the device
starts from), the zero-key vector, and key schedule and CFB output against libcrypto's BF_set_key / BF_cfb64_encrypt.
There is no public test vector of the whole scheme here: the definition rests on this model (SHA-1 and PBKDF2 from
hashlib, Blowfish checked as above)."""
import ctypes
import ctypes.util
import hashlib
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import odf_legacy_model as model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "dprf_amd", "csrc", "blowfish_init.h")
KEYS = [b"\0" * 16, bytes(range(16)), hashlib.md5(b"a").digest(), hashlib.md5(b"b").digest(), b"\xff" * 16,
        b"k", b"Who is John Galt?", bytes(range(200, 256))]


def test_init_words_are_pi():
    w = model.init_words()
    assert len(w) == 18 + 1024
    assert list(w[:4]) == [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]
    assert w[17] == 0x8979fb1b and w[18] == 0xd1310ba6       # the last P word and S[0][0]
    assert w[-1] == 0x3ac372e6


def header_words():
    text = open(HEADER).read()
    return [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{8})u", text[text.index("BF_INIT_TABLE"):])]


def test_header_holds_the_same_words():
    assert header_words() == list(model.init_words())
    assert "#define BF_INIT_WORDS 1042" in open(HEADER).read()


def test_generator_reproduces_the_header():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_blowfish_init.py")], check=True,
                         capture_output=True, text=True).stdout
    assert out == open(HEADER).read()


def test_zero_key_vector():
    """Schneier's first test vector: key 0000000000000000, plaintext 0000000000000000 -> 4ef997456198dd78"""
    assert model.Blowfish(b"\0" * 8).encrypt_block(b"\0" * 8).hex() == "4ef997456198dd78"
    assert model.Blowfish(b"\xff" * 8).encrypt_block(b"\xff" * 8).hex() == "51866fd5b85ecb8a"


def _libcrypto():
    for name in (ctypes.util.find_library("crypto"), "libcrypto.so.3", "libcrypto.so.1.1", "libcrypto.so"):
        if not name:
            continue
        try:
            lib = ctypes.CDLL(name)
            lib.BF_set_key, lib.BF_cfb64_encrypt, lib.BF_ecb_encrypt
            return lib
        except (OSError, AttributeError):
            continue
    return None


LIB = _libcrypto()
needs_bf = pytest.mark.skipif(LIB is None, reason="libcrypto with BF_set_key / BF_cfb64_encrypt not found")


class BF_KEY(ctypes.Structure):
    _fields_ = [("P", ctypes.c_uint32 * 18), ("S", ctypes.c_uint32 * 1024)]


def _set_key(key):
    ks = BF_KEY()
    LIB.BF_set_key(ctypes.byref(ks), len(key), key)
    return ks


@needs_bf
@pytest.mark.parametrize("key", KEYS, ids=[k.hex()[:16] for k in KEYS])
def test_key_schedule_matches_libcrypto(key):
    ks = _set_key(key)
    assert model.Blowfish(key).state_words() == list(ks.P) + list(ks.S)


@needs_bf
@pytest.mark.parametrize("key", KEYS[:5], ids=[k.hex()[:16] for k in KEYS[:5]])
def test_cfb64_matches_libcrypto(key):
    text = model._rand(key.hex(), "text", 1024)
    iv = model._rand(key.hex(), "iv", 8)
    bf = model.Blowfish(key)
    for enc in (1, 0):
        ks, ivec, num = _set_key(key), ctypes.create_string_buffer(iv, 8), ctypes.c_int(0)
        out = ctypes.create_string_buffer(1024)
        LIB.BF_cfb64_encrypt(text, out, ctypes.c_long(1024), ctypes.byref(ks), ivec, ctypes.byref(num), enc)
        assert out.raw == model.cfb64(bf, iv, text, decrypt=not enc)
    assert model.cfb64(bf, iv, model.cfb64(bf, iv, text, decrypt=False), decrypt=True) == text


@pytest.mark.parametrize("iterations", [1, 2, 1024])
def test_make_stream_verifies(iterations):
    s = model.make_stream("pässwörd", iterations, seed=iterations)
    f = model.split_stream(s)
    assert f[2] == str(iterations) and len(f[4]) == 40 and len(f[6]) == 16 and len(f[8]) == 32 and len(f[10]) == 2048
    assert model.verifies(s, "pässwörd") and model.verifies(s, "pässwörd".encode())
    assert not model.verifies(s, "passwort") and not model.verifies(s, "")
    assert model.hits("x.odt:" + s + ":::tail", ["a", "pässwörd", "b"]) == [1]


def test_key_is_one_pbkdf2_block_of_the_sha1_start_key():
    key = model.derive_key(b"abc", b"s" * 16, 3)
    assert key == hashlib.pbkdf2_hmac("sha1", hashlib.sha1(b"abc").digest(), b"s" * 16, 3, 20)[:16]
