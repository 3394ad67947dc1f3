"""The key derivation a known-key search compares (include/dprf.h "password for a known key") is
tests/key40_model.key_of_password.  Here it is tied to the public hashcat pairs of the collider-#2 modes 9720 / 9820
(hash:key, password "hashcat"), to the golden PDF streams' recorded keys, and -- for the FFFFFFFF tail of R4 without
EncryptMetadata, which none of those covers -- to the oracle: the document planted with key_of_password(pw) must accept
pw."""
import pytest

import key40_model as km
from conftest import load_golden

VEC = load_golden("collide_vectors.json")


@pytest.mark.parametrize("name", sorted(VEC["public"]))
def test_public_collider_pairs(name):
    e = VEC["public"][name]
    f = km.fields_of(e["stream"])
    assert km.key_of_password(f, e["password"]).hex() == e["key"]
    assert km.key_verifies(f, bytes.fromhex(e["key"]))
    assert km.key_of_password(f, e["password"] + "x").hex() != e["key"]


def test_public_pairs_are_the_key_search_vectors():
    """The collider-#2 pairs are the documents and keys of the collider-#1 vectors (key40_vectors.json)."""
    k40 = load_golden("key40_vectors.json")["public"]
    assert sorted((e["stream"], e["key"]) for e in VEC["public"].values()) == \
        sorted((e["stream"], e["key"]) for e in k40.values())


@pytest.mark.parametrize("name", sorted(VEC["streams"]))
def test_golden_pdf_streams(name, streams):
    e = VEC["streams"][name]
    f = km.fields_of(streams[name]["stream"])
    assert e["password"] == streams[name]["password"]
    assert km.key_of_password(f, e["password"]).hex() == e["key"]


def test_vectors_cover_the_four_families(streams):
    fams = {km.family(km.fields_of(e["stream"])) for e in VEC["public"].values()}
    fams |= {km.family(km.fields_of(streams[n]["stream"])) for n in VEC["streams"]}
    assert fams == {"pdf_r2", "pdf_r34", "office_md5", "office_sha1"}


@pytest.mark.parametrize("meta", [0, 1])
@pytest.mark.parametrize("pw", ["dog", "", "a-password-of-more-than-32-bytes-in-all"])
def test_r4_tail_is_the_reference(meta, pw, streams, oracle):
    """A golden R4 stream with Length set to 40: with EncryptMetadata 0 the first MD5 ends in FFFFFFFF, with 1 it
    does not.  The document planted with the model's key must accept the password in the reference."""
    f = km.fields_of(streams["pdf_synth_r4_meta0_dog"]["stream"])
    assert f[2] == "4"
    f[3], f[5] = "40", str(meta)
    key = km.key_of_password(f, pw)
    planted = km.plant(f, key)
    assert oracle.Ctx(planted).verify(pw) == 1
    assert oracle.Ctx(planted).verify(pw + "x") == (1 if len(pw.encode()) >= 32 else 0)
    # the tail matters: the other setting of EncryptMetadata gives another key
    g = list(f)
    g[5] = str(1 - meta)
    assert km.key_of_password(g, pw) != key
