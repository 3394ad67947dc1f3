"""What dprf_ctx_set_key40 decides without a device -- the accepted domain and the known-key family name per document,
the refusal sentence of every other family, the owner / key exclusion in both orders, and that dprf_plan_chunk knows the
names -- through the stand-alone program tests/host/collide_check.cpp over dprf_doc.cpp, built with plain g++ (no HIP):
one stream per family of tests/doc_layer.FAMILIES."""
import os
import subprocess

import pytest

import doc_layer as D
from conftest import REPO

KEY = "91b2e062b9"
# label of doc_layer.FAMILIES -> the family's known-key name, or a word its refusal must name
ACCEPTED = {"oldoffice_0": "office_rc4_md5_collide", "oldoffice_1": "office_rc4_md5_collide",
            "oldoffice_3": "office_rc4_sha1_collide", "pdf_r2": "pdf_r24_collide", "pdf_r3_40": "pdf_r24_collide"}
REFUSED = {"office_2007": "Office 2007", "agile_2010": "Agile", "agile_2013": "Agile", "oldoffice_4": "type 4",
           "odt": "ODF 1.2", "odf": "ODF 1.0/1.1", "pdf_r3_128": "128-bit", "pdf_r4_meta0": "128-bit", "pdf_r5": "R5",
           "pdf_r6": "R6"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    csrc = os.path.join(REPO, "dprf_amd", "csrc")
    out = os.path.join(str(tmp_path_factory.mktemp("collide_check")), "collide_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", csrc, os.path.join(REPO, "tests", "host", "collide_check.cpp"),
                    os.path.join(csrc, "dprf_doc.cpp"), "-o", out], check=True)
    return out


def test_every_family_is_listed():
    assert sorted(list(ACCEPTED) + list(REFUSED)) == sorted(D.LABELS)


@pytest.mark.parametrize("label", sorted(ACCEPTED))
def test_accepted_domain_and_family_name(exe, label):
    fields, _, family, _ = D.case(label)
    rows = D.run(exe, [D.ctx_line(fields), "key\t" + KEY, "words", "key\t0000000000", "key\t-", "key\t-"])
    assert rows[0] == ["0", family, ACCEPTED[label]]
    assert rows[1] == ["0", ACCEPTED[label]]
    assert rows[2] == ["62e0b291", "000000b9"]             # bytes 91 b2 e0 62 as an LE word, byte 4
    assert rows[3] == ["0", ACCEPTED[label]]               # a key may hold any byte, 00 included
    assert rows[4] == ["0", family] and rows[5] == ["0", family]   # cleared: the password family again; twice is fine


@pytest.mark.parametrize("label", sorted(REFUSED))
def test_refused_families_say_why_and_keep_their_name(exe, label):
    fields, _, family, _ = D.case(label)
    rows = D.run(exe, [D.ctx_line(fields), "key\t" + KEY, "key\t-"])
    assert rows[0][:2] == ["0", family]
    assert rows[0][2] == ("pdf_r24_collide" if family == "pdf_r24" else
                          "office_rc4_sha1_collide" if family == "office_rc4_sha1" else "-")
    code, text = rows[1]
    assert int(code) == D.E_DOMAIN
    assert "40-bit" in text and "not a 40-bit document" in text and REFUSED[label] in text, text
    assert rows[2] == ["0", family]                        # clearing is never refused, and nothing was set


def test_refusal_sentences_are_the_key_searchs(exe, tmp_path_factory):
    """The domain half is one function: dprf_ctx_set_key40 and dprf_search_key40 refuse with the same words."""
    csrc = os.path.join(REPO, "dprf_amd", "csrc")
    k40 = os.path.join(str(tmp_path_factory.mktemp("key40_check")), "key40_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", csrc, os.path.join(REPO, "tests", "host", "key40_check.cpp"),
                    os.path.join(csrc, "dprf_doc.cpp"), "-o", k40], check=True)
    for label in sorted(REFUSED):
        line = D.ctx_line(D.case(label)[0])
        assert D.run(exe, [line, "key\t" + KEY])[1] == D.run(k40, [line, "key40\t0\t1"])[1], label


@pytest.mark.parametrize("label", ["pdf_r2", "pdf_r3_40"])
def test_owner_and_key_exclude_each_other_in_both_orders(exe, label):
    fields = D.case(label)[0]
    # the key first: owner mode is refused, the key stays, user mode is still selectable
    rows = D.run(exe, [D.ctx_line(fields), "key\t" + KEY, "owner\t1", "owner\t0", "key\t-", "owner\t1"])
    assert rows[1] == ["0", "pdf_r24_collide"]
    assert int(rows[2][0]) == D.E_INVALID and "key" in rows[2][1]
    assert rows[3] == ["0", "pdf_r24_collide"]
    assert rows[4] == ["0", "pdf_r24"] and rows[5] == ["0", "pdf_r24_owner"]
    # owner mode first: the key is refused, the mode stays, clearing is fine, and user mode takes the key
    rows = D.run(exe, [D.ctx_line(fields), "owner\t1", "key\t" + KEY, "key\t-", "owner\t0", "key\t" + KEY])
    assert rows[1] == ["0", "pdf_r24_owner"]
    assert int(rows[2][0]) == D.E_INVALID and "owner" in rows[2][1]
    assert rows[3] == ["0", "pdf_r24_owner"]
    assert rows[4] == ["0", "pdf_r24"] and rows[5] == ["0", "pdf_r24_collide"]


def test_domain_is_judged_before_the_owner_mode(exe):
    rows = D.run(exe, [D.ctx_line(D.case("pdf_r5")[0]), "owner\t1", "key\t" + KEY])
    assert rows[1] == ["0", "pdf_r5_owner"] and int(rows[2][0]) == D.E_DOMAIN


def test_never_matching_context_accepts_a_key(exe):
    fields = list(D.case("pdf_r2")[0])
    fields[2] = "3"                                        # V 1 with R 3: the reference's verdict is constant
    rows = D.run(exe, [D.ctx_line(fields), "key\t" + KEY, "key\t-"])
    assert rows[0] == ["0", "none", "-"]
    assert rows[1] == ["0", "none"] and rows[2] == ["0", "none"]


@pytest.mark.parametrize("name,parent", [("pdf_r24_collide", "pdf_r24"), ("office_rc4_md5_collide", "office_rc4_md5"),
                                         ("office_rc4_sha1_collide", "office_rc4_sha1")])
def test_plan_chunk_knows_the_names(exe, name, parent):
    huge = 1 << 40
    first, first_parent, small, split = [int(r[0]) for r in D.run(exe, [
        "plan\t%s\t0\t%d\t%d\t1\t0" % (name, huge, huge), "plan\t%s\t0\t%d\t%d\t1\t0" % (parent, huge, huge),
        "plan\t%s\t0\t1000\t%d\t1\t0" % (name, huge), "plan\t%s\t5000000\t%d\t%d\t4\t1" % (name, 1 << 22, 1 << 30)])]
    assert first != 0 and first == first_parent            # the password family's first chunk
    assert small == 1000
    assert 0 < split <= 1 << 22
    # later chunks grow with the measured rate and stay powers of two
    last = 0
    for rate in (1e3, 1e5, 1e6, 1e7, 1e8):
        n = int(D.run(exe, ["plan\t%s\t%r\t%d\t%d\t1\t0" % (name, rate, huge, huge)])[0][0])
        assert n >= last and n & (n - 1) == 0 and n < 1 << 32
        last = n
    # the ceiling: 2^31, the most a launch's 32-bit count takes, where the password family stops at 2^30
    assert last == 1 << 31
    assert D.run(exe, ["plan\t%s\t1e8\t%d\t%d\t1\t0" % (parent, huge, huge)]) == [[str(1 << 30)]]
    assert D.run(exe, ["plan\tpdf_r5_collide\t0\t1\t1\t1\t0"]) == [["0"]]
