"""The 40-bit key model (tests/key40_model.py) against the check values of include/dprf.h "40-bit key search", the
public hashcat vectors, the oracle and the Office model: what ties the key search's definition to the reference."""
import hashlib

import pytest

import key40_model as km
import oldoffice_model
from conftest import load_golden

VEC = load_golden("key40_vectors.json")
CASES = km.known_password_cases()


@pytest.mark.parametrize("name", sorted(VEC["streams"]))
def test_golden_stream_keys(name, streams):
    e = VEC["streams"][name]
    f = km.fields_of(streams[name]["stream"])
    key = bytes.fromhex(e["key"])
    assert km.key_index(key) == e["index"] and "%010x" % e["index"] == e["key"]
    assert km.key_verifies(f, key)
    assert km.key_of_password(f, streams[name]["password"]) == key


@pytest.mark.parametrize("name", sorted(VEC["public"]))
def test_public_hashcat_vectors(name):
    e = VEC["public"][name]
    f = km.fields_of(e["stream"])
    key = bytes.fromhex(e["key"])
    assert km.key_verifies(f, key)
    assert not km.key_verifies(f, km.key_bytes(km.key_index(key) ^ 1))
    if "password" in e:
        # SHA1(SHA1(salt || pw16) || 00000000)[0:5]
        salt = bytes.fromhex(f[2])
        h = hashlib.sha1(salt + e["password"].encode("utf-16-le")).digest()
        assert hashlib.sha1(h + b"\0" * 4).digest()[:5] == key == km.key_of_password(f, e["password"])


def test_type3_vector_is_the_golden_document():
    a = km.fields_of(VEC["public"]["oldoffice_type3_hashcat_9810"]["stream"])
    b = km.fields_of(load_golden("oldoffice_vectors.json")["oldoffice_type3_hashcat"]["stream"])
    assert a == b


def test_r2_keystream_vector():
    e = VEC["r2_keystream"]
    assert oldoffice_model.rc4(bytes.fromhex(e["key"]), km.PAD).hex() == e["rc4_of_pad"]


@pytest.mark.parametrize("label", [c[0] for c in CASES])
def test_password_key_verifies_and_reference_accepts_password(label, oracle):
    _, f, pw = [c for c in CASES if c[0] == label][0]
    if f[0] == "pdf":
        assert oracle.Ctx(f).verify(pw) == 1
    else:
        assert oldoffice_model.verifies(f, pw)
    key = km.key_of_password(f, pw)
    assert km.key_verifies(f, key)
    assert not km.key_verifies(f, km.key_bytes((km.key_index(key) + 1) % km.SPACE))


def test_cases_cover_the_four_families():
    assert set(km.family(c[1]) for c in CASES) == {"pdf_r2", "pdf_r34", "office_md5", "office_sha1"}


@pytest.mark.parametrize("fam", ["pdf_r2", "pdf_r34", "office_md5", "office_sha1"])
@pytest.mark.parametrize("index", [0, 0xff, 0x100, 0xffffffff, 0x100000000, km.SPACE - 1, 0x123456789a])
def test_planted_key_verifies_and_neighbours_do_not(fam, index):
    f = km.plant(km.base_documents()[fam], km.key_bytes(index), seed=index & 0xffff)
    assert km.key_verifies(f, km.key_bytes(index))
    for n in (index - 1, index + 1):
        if 0 <= n < km.SPACE:
            assert not km.key_verifies(f, km.key_bytes(n))


@pytest.mark.parametrize("index", [0, 0xff, 0x100, 0xffffffff, 0x100000000, km.SPACE - 1])
def test_index_bytes_round_trip(index):
    from dprf_amd import key40
    b = key40.key_bytes(index)
    assert b == km.key_bytes(index) == index.to_bytes(5, "big")
    assert b[0] == index >> 32 and b[4] == index & 0xff
    assert key40.key_index(b) == key40.key_index(b.hex()) == index == km.key_index(b)
    assert key40.key_hex(index) == "%010x" % index


def test_order_is_itertools_product():
    import itertools
    from dprf_amd import key40
    got = list(itertools.islice(itertools.product(range(256), repeat=5), 255, 258))
    assert [bytes(t) for t in got] == [key40.key_bytes(i) for i in (255, 256, 257)]
    for bad in (-1, 1 << 40):
        with pytest.raises(ValueError):
            key40.key_bytes(bad)
