"""tests/owner_model.py, the Python statement of the owner-password check, pinned on the CPU: against every
self-made PDF (written with owner password "owner"), against the reference's own test documents (made by third-party
software with one password: decrypting their /O gives that password padded, which anchors the R2-R4 definition
independently of this repository's document writer), and against hashlib / docgen on fresh R5 / R6 documents."""
import hashlib
import os

import pytest

import docgen
import owner_model as M
from conftest import load_golden


def _pdf_docs():
    docs = load_golden("docs.json")
    return sorted((name, e) for name, e in docs.items() if e["kind"] == "pdf")


@pytest.mark.parametrize("name", [n for n, _ in _pdf_docs()])
def test_golden_docs_verify_owner_only(oracle, name):
    e = dict(_pdf_docs())[name]
    stream = e["streams"]["std"]["stream"]
    assert M.owner_verifies(stream, b"owner")
    assert not M.owner_verifies(stream, e["password"].encode())
    assert not M.owner_verifies(stream, b"ownes")


@pytest.mark.parametrize("key", ["pdf_testdoc_r2", "pdf_testdoc_r4"])
def test_reference_documents_anchor_r24(oracle, streams, key):
    stream = streams[key]["stream"]
    assert M.owner_decrypts_to(stream, "password") == b"password" + M.PAD[:24]
    assert M.owner_verifies(stream, b"password")
    assert not M.owner_verifies(stream, b"passwore")


@pytest.mark.parametrize("R", [5, 6])
def test_r56_agree_with_docgen_and_hashlib(oracle, tmp_path, R):
    from dprf_amd.parsers import pdf2john
    path = os.path.join(str(tmp_path), "d.pdf")
    docgen.write_pdf(path, "usr", 0x0A11 + R, R=R, length=256, owner="0wner-pw")
    stream = pdf2john.get_hash(path)
    d = M.parse(stream)
    o, u = d["O"], d["U"]
    ow = b"0wner-pw"
    if R == 5:
        assert hashlib.sha256(ow + o[32:40] + u[:48]).digest() == o[:32]
    else:
        assert docgen.pdf_r6_hash(ow, o[32:40], u[:48]) == o[:32]
        assert M.r6_hash(ow, o[32:40], u[:48]) == o[:32]
    assert M.owner_verifies(stream, ow)
    assert not M.owner_verifies(stream, b"usr")
    assert not M.owner_verifies(stream, b"0wner-pv")
