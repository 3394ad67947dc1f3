"""tests/oldoffice_model.py, the Python statement of the Office 97-2003 RC4 verifier check, pinned on the CPU: the
public vectors (hashcat modes 9700 / 9800), planted passwords of every length for every type, and one flipped bit in
each hex field.  The GPU tests (tests/test_oldoffice_gpu.py) compare k_oldoffice with this model."""
import pytest

import oldoffice_model as M
from conftest import load_golden

VECTORS = ["oldoffice_type1_hashcat", "oldoffice_type3_hashcat"]


def test_rc4_known_answers():
    """RFC 6229's first keystream bytes for the 40-bit key 01 02 03 04 05, and the classic "Key" / "Plaintext"."""
    assert M.rc4(bytes([1, 2, 3, 4, 5]), b"\0" * 16).hex() == "b2396305f03dc027ccc3524a0a1118a8"
    assert M.rc4(b"Key", b"Plaintext").hex() == "bbf316e8d940af0ad3"


@pytest.mark.parametrize("name", VECTORS)
def test_public_vectors(name):
    v = load_golden("oldoffice_vectors.json")[name]
    pw = v["password"]
    assert M.verifies(v["stream"], pw)
    near = {
        "one character changed": pw[:3] + "x" + pw[4:],
        "one character dropped": pw[:-1],
        "one character added": pw + "x",
        "an upper-cased letter": pw[:-1] + pw[-1].upper(),
    }
    for what, cand in near.items():
        assert cand != pw and not M.verifies(v["stream"], cand), what


def test_type3_key_is_five_bytes_zero_extended():
    """A type-3 key is k[0:5] || eleven 00 bytes, a 16-byte RC4 key: the 5-byte key schedules differently and misses
    the public vector."""
    v = load_golden("oldoffice_vectors.json")["oldoffice_type3_hashcat"]
    f = M.fields_of(v["stream"])
    salt, ev, evh = (bytes.fromhex(x) for x in f[2:5])
    key = M.derive_key(v["password"], 3, salt)
    assert len(key) == 16 and key[5:] == b"\0" * 11
    d = M.rc4(key[:5], ev + evh)
    assert M.hash_of(3)[0](d[:16]).digest() != d[16:36]


def _planted(L):
    return "".join(chr(33 + (7 * k + 5 * L + k * k) % 90) for k in range(L))


@pytest.mark.parametrize("typ", M.TYPES)
def test_planted_lengths_round_trip(typ):
    for L in range(1, 33):
        pw = _planted(L)
        s = M.make_stream(pw, typ, seed=1000 * typ + L)
        assert M.verifies(s, pw), L
        assert not M.verifies(s, pw[:-1] + "~") and not M.verifies(s, pw + "x"), L
        if L > 1:
            assert not M.verifies(s, pw[:-1]), L


@pytest.mark.parametrize("typ", M.TYPES)
def test_one_flipped_bit_is_rejected(typ):
    pw = "Ux7"
    f = M.fields_of(M.make_stream(pw, typ, seed=77 + typ))
    assert M.verifies(f, pw)
    for k in (2, 3, 4):
        raw = bytes.fromhex(f[k])
        for pos in (0, len(raw) // 2, len(raw) - 1):
            for bit in (0, 7):
                t = bytearray(raw)
                t[pos] ^= 1 << bit
                g = list(f)
                g[k] = bytes(t).hex()
                assert not M.verifies(g, pw), (k, pos, bit)


def test_both_spellings_give_the_same_fields():
    salt, ev, evh = M.make_parts("Ux7", 4, 9)
    a = M.stream_of(4, salt, ev, evh, spelling="john")
    b = M.stream_of(4, salt, ev, evh, spelling="hashcat")
    assert a != b and M.fields_of(a) == M.fields_of(b) == M.fields_of(b + ":::sum::made.doc")
    assert M.fields_of(a) == ["oldoffice", "4", salt.hex(), ev.hex(), evh.hex()]
