"""What dprf_search_key40 decides without a device -- the accepted domain, the refusal sentence of every other family
and the window check -- through the stand-alone program tests/host/key40_check.cpp over dprf_doc.cpp, built with plain
g++ (no HIP): one stream per family of tests/doc_layer.FAMILIES."""
import os
import subprocess

import pytest

import doc_layer as D
from conftest import REPO

SPACE = 1 << 40
# label of doc_layer.FAMILIES -> the family's key-search name, or a word its refusal must name
ACCEPTED = {"oldoffice_0": "office_rc4_md5_key40", "oldoffice_1": "office_rc4_md5_key40",
            "oldoffice_3": "office_rc4_sha1_key40", "pdf_r2": "pdf_r24_key40", "pdf_r3_40": "pdf_r24_key40"}
REFUSED = {"office_2007": "Office 2007", "agile_2010": "Agile", "agile_2013": "Agile", "oldoffice_4": "type 4",
           "odt": "ODF 1.2", "odf": "ODF 1.0/1.1", "pdf_r3_128": "128-bit", "pdf_r4_meta0": "128-bit", "pdf_r5": "R5",
           "pdf_r6": "R6"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    csrc = os.path.join(REPO, "dprf_amd", "csrc")
    out = os.path.join(str(tmp_path_factory.mktemp("key40_check")), "key40_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", csrc, os.path.join(REPO, "tests", "host", "key40_check.cpp"),
                    os.path.join(csrc, "dprf_doc.cpp"), "-o", out], check=True)
    return out


def test_every_family_is_listed():
    assert sorted(list(ACCEPTED) + list(REFUSED)) == sorted(D.LABELS)


@pytest.mark.parametrize("label", sorted(ACCEPTED))
def test_accepted_domain(exe, label):
    fields, _, family, _ = D.case(label)
    rows = D.run(exe, [D.ctx_line(fields), "key40\t0\t%d" % SPACE, "key40\t%d\t1" % (SPACE - 1), "key40\t12345\t0"])
    assert rows[0] == ["0", family, ACCEPTED[label]]
    assert rows[1:] == [["0"], ["0"], ["0"]]


@pytest.mark.parametrize("label", sorted(REFUSED))
def test_refused_families_say_why(exe, label):
    fields, _, family, _ = D.case(label)
    rows = D.run(exe, [D.ctx_line(fields), "key40\t0\t1"])
    assert rows[0][0] == "0" and rows[0][1] == family
    assert rows[0][2] == ("pdf_r24_key40" if family == "pdf_r24" else
                          "office_rc4_sha1_key40" if family == "office_rc4_sha1" else "-")
    code, text = rows[1]
    assert int(code) == D.E_DOMAIN
    assert "40-bit" in text and "not a 40-bit document" in text and REFUSED[label] in text, text


def test_window_check(exe):
    fields = D.case("pdf_r2")[0]
    lines = [D.ctx_line(fields),
             "key40\t0\t%d" % SPACE,                        # the whole space
             "key40\t0\t%d" % (SPACE + 1),
             "key40\t1\t%d" % SPACE,                        # start + count = 2^40 + 1
             "key40\t%d\t0" % SPACE,                        # an empty window at the end
             "key40\t%d\t0" % (SPACE + 1),
             "key40\t%d\t%d" % ((1 << 64) - 1, 2),          # start + count wraps 2^64 to 1
             "key40\t%d\t%d" % (2, (1 << 64) - 1),
             "key40\t%d\t%d" % ((1 << 63), (1 << 63))]     # wraps to 0
    rows = D.run(exe, lines)
    assert [r[0] for r in rows[1:]] == ["0", "-1", "-1", "0", "-1", "-1", "-1", "-1"]
    for r in rows[1:]:
        if r[0] != "0":
            assert "2^40" in r[1]


def test_window_is_judged_before_the_domain(exe):
    rows = D.run(exe, [D.ctx_line(D.case("pdf_r5")[0]), "key40\t0\t%d" % (SPACE + 1), "key40\t0\t1"])
    assert int(rows[1][0]) == D.E_INVALID and int(rows[2][0]) == D.E_DOMAIN


def test_owner_mode_does_not_change_the_domain(exe):
    rows = D.run(exe, [D.ctx_line(D.case("pdf_r3_40")[0]), "owner\t1", "key40\t0\t%d" % SPACE])
    assert rows[1] == ["0"] and rows[2] == ["0"]


def test_never_matching_context_passes(exe):
    """A never-matching context (kind none) answers "no hit" as in every search: the check lets it through."""
    fields = list(D.case("pdf_r2")[0])
    assert fields[1] == "1"
    fields[2] = "3"                                        # V 1 with R 3: the reference's verdict is constant
    rows = D.run(exe, [D.ctx_line(fields), "key40\t0\t10", "key40\t1\t%d" % SPACE])
    assert rows[0] == ["0", "none", "-"]
    assert rows[1] == ["0"] and int(rows[2][0]) == D.E_INVALID


@pytest.mark.parametrize("name,parent", [("pdf_r24_key40", "pdf_r24"), ("office_rc4_md5_key40", "office_rc4_md5"),
                                         ("office_rc4_sha1_key40", "office_rc4_sha1")])
def test_plan_chunk_knows_the_key_searches(exe, name, parent):
    args = [("0", 1 << 40, 1 << 40, 1, 0), ("5000000", 1 << 40, 1 << 40, 1, 0), ("5000000", 1 << 22, 1 << 30, 4, 1)]
    rows = D.run(exe, ["plan\t%s\t%s\t%d\t%d\t%d\t%d" % ((n,) + a) for a in args for n in (name, parent)])
    for k in range(0, len(rows), 2):
        assert rows[k] == rows[k + 1]
    assert int(rows[0][0]) != 0
    assert D.run(exe, ["plan\tpdf_r5_key40\t0\t1\t1\t1\t0"]) == [["0"]]
