"""tests/agile_model.py -- the Python statement of Office 2010 / 2013 Agile Encryption's password verifier -- pinned
on the CPU: the public example hashes of hashcat modes 9500 / 9600 (tests/golden/agile_vectors.json) verify with their
password and with no near miss, agile_model.make_stream round-trips for every (version, keyBits) pair, and the document
writer (tests/agile_docgen.py) and the project's parser agree."""
import os

import pytest

import agile_docgen
import agile_model as M
from conftest import load_golden

PAIRS = [("2010", 128), ("2010", 256), ("2013", 128), ("2013", 256)]
SPINS = [0, 1, 3, 1000]


@pytest.mark.parametrize("name", ["office_2010_hashcat", "office_2013_hashcat"])
def test_public_vectors(name):
    v = load_golden("agile_vectors.json")[name]
    assert v["password"] == "hashcat"
    assert M.verifies(v["stream"], "hashcat")
    for near in ("hashcatx", "Hashcat", "hashca"):
        assert not M.verifies(v["stream"], near), near


@pytest.mark.parametrize("version,bits", PAIRS)
@pytest.mark.parametrize("spin", SPINS)
def test_make_stream_round_trips(version, bits, spin):
    s = M.make_stream("Ux7", version, bits, spin, seed=1000 * bits + spin)
    f = M.fields_of(s)
    assert f[:5] == ["office", version, str(spin), str(bits), "16"]
    assert [len(x) for x in f[5:]] == [32, 32, 64]
    assert M.verifies(s, "Ux7")
    for near in ("Ux6", "Ux8", "Ux", "Ux77", "ux7"):
        assert not M.verifies(s, near), near


def test_spin_changes_the_keys():
    salt = bytes(range(16))
    keys = {spin: M.derive_keys("Ux7", "2013", 256, salt, spin) for spin in SPINS}
    assert len({k for k in keys.values()}) == len(SPINS)
    assert all(len(k1) == 32 and len(k2) == 32 and k1 != k2 for k1, k2 in keys.values())


@pytest.mark.parametrize("spin", SPINS)
def test_sha1_256_bit_key_is_padded_with_0x36(spin):
    salt = bytes(range(1, 17))
    k128 = M.derive_keys("Ux7", "2010", 128, salt, spin)
    k256 = M.derive_keys("Ux7", "2010", 256, salt, spin)
    for a, b in zip(k128, k256):
        # the two key sizes differ only in the cut: 16 bytes of the hash, or all 20 and twelve bytes of 0x36
        assert len(a) == 16 and len(b) == 32 and b[:16] == a and b[20:] == b"\x36" * 12 and b[16:20] != b"\x36" * 4
    s = M.make_stream("Ux7", "2010", 256, spin, seed=77 + spin)
    assert M.verifies(s, "Ux7")
    assert not M.verifies(s, "Ux7", pad=0x00), "the padded key is what verifies: zero padding must not"
    assert not M.verifies(s, "Ux7", pad=0x5C)


def test_first_message_lengths():
    # SHA-1's first message crosses from one block to two at 20 characters; SHA-512's stays within one block
    assert M.first_message_len("a" * 19) == 54 and M.first_message_len("a" * 20) == 56
    assert M.first_message_len("a" * 32) == 80 <= 111
    assert M.first_message_len("\U0001F600ok") == 16 + 8          # a surrogate pair is two units


@pytest.mark.parametrize("version,bits", PAIRS)
def test_document_writer_and_parser_agree(tmp_path, version, bits):
    from dprf_amd.parsers import office2john
    path = os.path.join(str(tmp_path), "agile_%s_%d.docx" % (version, bits))
    made = agile_docgen.write_docx_agile(path, "Ux7", 4242 + bits, version=version, key_bits=bits, spin=1000)
    got = office2john.get_hash(path).strip()
    assert got.split(":", 1)[0] == os.path.basename(path)
    assert got.split(":", 1)[1] == made.split(":", 1)[1]
    assert made == M.make_stream("Ux7", version, bits, 1000, 4242 + bits)
    assert M.verifies(got, "Ux7") and not M.verifies(got, "Ux8")


def test_encryption_info_header_and_descriptor(tmp_path):
    import struct
    import xml.etree.ElementTree as et
    info = agile_docgen.encryption_info("Ux7", 9, "2013", 256, 1000)
    assert struct.unpack_from("<HHI", info, 0) == (4, 4, 0x40)
    root = et.fromstring(info[8:])
    ns = {"e": "http://schemas.microsoft.com/office/2006/encryption",
          "p": "http://schemas.microsoft.com/office/2006/keyEncryptor/password"}
    assert root.find("e:keyData", ns) is not None
    key = root.find("e:keyEncryptors/e:keyEncryptor/p:encryptedKey", ns)
    for attr in ("spinCount", "saltSize", "blockSize", "keyBits", "hashSize", "cipherAlgorithm", "cipherChaining",
                 "hashAlgorithm", "saltValue", "encryptedVerifierHashInput", "encryptedVerifierHashValue",
                 "encryptedKeyValue"):
        assert attr in key.attrib, attr
