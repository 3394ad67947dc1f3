"""check_combine (dprf_amd/csrc/dprf_doc.cpp), the device-free half of dprf_search_combine and dprf_spell_combine, in the
stand-alone program tests/host/combine_check.cpp built with g++ alone: the window against N1 * N2 in 128 bits, each
missing table, the DPRF_E_PWLEN sentence that names both words, and PDF R2-R4 taking tables of any word lengths."""
import os
import subprocess

import pytest

import doc_layer
from conftest import REPO

E_INVALID, E_PWLEN = doc_layer.E_INVALID, doc_layer.E_PWLEN


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    csrc = os.path.join(REPO, "dprf_amd", "csrc")
    out = os.path.join(str(tmp_path_factory.mktemp("combine_check")), "combine_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", csrc, os.path.join(REPO, "tests", "host", "combine_check.cpp"),
                    os.path.join(csrc, "dprf_doc.cpp"), "-o", out], check=True)
    return out


def ask(exe, label, tables, checks):
    """The program's answers to `checks` (start, count) on the document `label` holding `tables`."""
    fields = doc_layer.case(label)[0]
    lines = [doc_layer.ctx_line(fields), "tables\t" + "\t".join(str(v) for v in tables)]
    lines += ["check\t%d\t%d" % c for c in checks]
    rows = doc_layer.run(exe, lines)
    assert rows[0][0] == "0" and rows[1] == ["ok"], rows[:2]
    return [(int(r[0]), r[1]) for r in rows[2:]]


def test_window_at_the_keyspace_and_one_past_it(exe):
    n1, n2 = 300, 257
    got = ask(exe, "pdf_r5", (n1, 12, 4, n2, 9, 200),
              [(0, n1 * n2), (n1 * n2, 0), (n1 * n2 - 1, 1), (0, n1 * n2 + 1), (n1 * n2, 1), (1, n1 * n2), (5, 0)])
    assert [g[0] for g in got] == [0, 0, 0, E_INVALID, E_INVALID, E_INVALID, 0]
    assert got[0][1] == "21"                                               # the longest candidate: 12 + 9 bytes
    for code, text in got[3:6]:
        assert "exceeds the combinator keyspace of 300 left times 257 right words" in text


def test_keyspace_over_2_to_the_64_takes_a_window_just_below_it(exe):
    """N1 * N2 = (2^32 - 1) * (2^31 - 1) < 2^64 is exact; with 2^34 left words (no setter gives that many, but the bound
    is computed in 128 bits) N1 * N2 = 2^64 + ... and the last window below 2^64 passes instead of wrapping."""
    top = (1 << 64) - 1
    n1, n2 = (1 << 32) - 1, (1 << 31) - 1
    got = ask(exe, "pdf_r5", (n1, 3, 0, n2, 3, 0), [(n1 * n2 - 1000, 1000), (n1 * n2 - 1000, 1001), (top - 5, 5)])
    assert [g[0] for g in got] == [0, E_INVALID, E_INVALID]
    n1 = 1 << 34
    assert n1 * n2 > 1 << 64
    got = ask(exe, "pdf_r5", (n1, 3, 0, n2, 3, 0), [(top - 1000, 1000), (top - 1000, 1001), (top, 0), (1 << 63, 1 << 63)])
    assert [g[0] for g in got] == [0, 0, 0, 0]                             # start + count = 2^64 does not wrap to 0


def test_each_missing_table_is_named(exe):
    got = ask(exe, "pdf_r5", (0, 0, 0, 5, 3, 1), [(0, 0), (0, 1)])
    assert all(code == E_INVALID and "no left word table (dprf_ctx_set_words)" in text for code, text in got), got
    got = ask(exe, "pdf_r5", (5, 3, 1, 0, 0, 0), [(0, 0), (0, 1)])
    assert all(code == E_INVALID and "no right word table (dprf_ctx_set_right_words)" in text for code, text in got), got
    got = ask(exe, "pdf_r5", (0, 0, 0, 0, 0, 0), [(0, 0)])
    assert got[0][0] == E_INVALID and "left" in got[0][1]
    assert got[0][1].startswith("dprf_search_combine:")


@pytest.mark.parametrize("label", ["pdf_r5", "pdf_r6", "odt", "odf", "office_2007", "agile_2013", "oldoffice_3"])
def test_two_longest_words_over_a_slot_are_refused_by_name(exe, label):
    got = ask(exe, label, (10, 40, 7, 20, 25, 13), [(0, 200), (0, 0)])
    for code, text in got:
        assert code == E_PWLEN, (label, got)
        assert "left word 7 takes 40 bytes, right word 13 takes 25" in text and "65 bytes" in text, text
    # 63 + 1, 1 + 63 and 32 + 32 fill the slot; one byte more on either side does not fit
    for ll, rl, ok in ((63, 1, True), (1, 63, True), (32, 32, True), (64, 1, False), (1, 64, False), (33, 32, False)):
        code, text = ask(exe, label, (10, ll, 0, 20, rl, 0), [(0, 200)])[0]
        assert (code, text) == (0, "64") if ok else code == E_PWLEN, (label, ll, rl, code, text)


def test_r5_counts_the_cut_at_127_bytes(exe):
    """min(l + r, 127) > 64 for any sum over 64: the R5 cut never rescues a pair."""
    code, text = ask(exe, "pdf_r5", (2, 5000, 1, 2, 5000, 0), [(0, 4)])[0]
    assert code == E_PWLEN and "127 bytes" in text and "left word 1 takes 5000 bytes, right word 0 takes 5000" in text


@pytest.mark.parametrize("label", ["pdf_r2", "pdf_r3_40", "pdf_r3_128", "pdf_r4_meta0"])
def test_r2_to_r4_accept_tables_of_any_word_lengths(exe, label):
    got = ask(exe, label, (3, 5000, 1, 4, 70000, 2), [(0, 12), (11, 1), (0, 13)])
    assert [g[0] for g in got] == [0, 0, E_INVALID] and got[0][1] == "32"   # the longest candidate after the cut
    assert ask(exe, label, (3, 10, 1, 4, 7, 2), [(0, 12)])[0] == (0, "17")
