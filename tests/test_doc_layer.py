"""The device-free document layer (dprf_amd/csrc/dprf_doc.cpp) through its stand-alone program tests/host/doc_check.cpp,
built here with g++ alone -- no HIP, no GPU, no sanitizer (HISTORY records a run of the same input through a build with
-fsanitize=address,undefined).  What a stream gives -- family, format, flags, every kernel-argument word -- is computed
in tests/doc_layer.py from the fields; the refusals are the lists the GPU tests pin, read from those modules.

  (a) one stream per family: name, fmt, flags; the never-matching stream and the leading-00 flag
  (b) the params words and the word vector, at the sizes where a parser can go wrong
  (c) every stream refusal: code and the field the message names
  (d) candidates at the edges, per family: codes, converted lengths, sentences"""
import pytest

import doc_layer as D
from doc_layer import E_DOMAIN, E_INVALID, E_PWLEN

NUL = "contains NUL (argv cannot carry it)"
TOO_LONG = "longer than 131,071 bytes (no argv string can carry it to the reference's verifier)"
UNDEFINED = ("empty or invalid UTF-8 Office password (the reference's iconv path is undefined), or a PDF R6 password over "
             "176 bytes (the reference overflows its data buffer and aborts)")
NO_LONG = {
    "office_agile_sha1": "longer than 32 UTF-16 units: long Office Agile candidates are not supported yet",
    "office_agile_sha512": "longer than 32 UTF-16 units: long Office Agile candidates are not supported yet",
    "office_rc4_md5": "longer than 32 UTF-16 units: long Office 97-2003 candidates are not supported yet",
    "office_rc4_sha1": "longer than 32 UTF-16 units: long Office 97-2003 candidates are not supported yet",
    "odf_bf_sha1": "longer than 64 bytes: long ODF 1.0/1.1 candidates are not supported yet",
}
NO_LONG_OWNER = "longer than 64 bytes: long owner-password candidates (PDF R5/R6) are not supported yet"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return D.build_doc_check(tmp_path_factory.mktemp("doc_check"))


def _ok(row, f):
    """A successful ctx row against the fields: (family, fmt, flags) after checking every word."""
    assert row[0] == "0" and len(row) == 6, row[:2]
    params, vec = D.expected_words(f)
    assert D.words(row[4]) == params, f[:3]
    assert D.words(row[5]) == vec, f[:3]
    return row[1], int(row[2]), int(row[3])


# ---------------------------------------------------------------- (a) families and flags
def test_families_formats_and_flags(exe):
    cases = [D.case(label) for label in D.LABELS]
    rows = D.run(exe, [D.ctx_line(c[0]) for c in cases])
    for label, (f, _, family, fmt), row in zip(D.LABELS, cases, rows):
        assert _ok(row, f) == (family, fmt, D.expected_flags(f)), label


def test_the_two_flags(exe):
    from test_gpu_parity import NEVER_MATCHING
    r2 = D.case("pdf_r2")[0]
    zero_id = list(r2)
    zero_id[7] = "00" + r2[7][2:]
    agile = D.case("agile_2010")[0]
    zero_salt = list(agile)
    zero_salt[5] = "00" + agile[5][2:]
    rows = D.run(exe, [D.ctx_line(f) for f in (NEVER_MATCHING, r2, zero_id, zero_salt)])
    # a (V, R) pair off the whitelist: no kernel family, no params, DPRF_FLAG_NEVER_MATCHES
    assert rows[0] == ["0", "none", "3", str(D.FLAG_NEVER_MATCHES), "", ""]
    assert not r2[7].startswith("00") and _ok(rows[1], r2) == ("pdf_r24", 3, D.expected_flags(r2))
    # a hex field with a leading 00 byte: flagged, and decoded in full
    assert _ok(rows[2], zero_id) == ("pdf_r24", 3, D.expected_flags(r2) | D.FLAG_REF_NONDETERMINISTIC)
    assert _ok(rows[3], zero_salt) == ("office_agile_sha1", 1, 0)      # no reference verifier reads Agile: never flagged


# ---------------------------------------------------------------- (b) params words at the parsers' edges
def test_params_at_the_parser_edges(exe):
    r3 = D.case("pdf_r3_128")[0]
    assert r3[6] == "16"
    long_id = list(r3)
    long_id[6], long_id[7] = "64", "".join("%02x" % (7 * i + 1 & 0xff) for i in range(64))
    odt = D.case("odt")[0]
    enc = bytes((i * 37 + 11) & 0xff for i in range(1040))
    odt16, odt1040 = list(odt), list(odt)
    odt16[5], odt16[6] = enc[:16].hex(), "16"
    odt1040[5], odt1040[6] = enc.hex(), "1040"
    r4 = D.case("pdf_r4_meta0")[0]
    assert r4[5] == "0"
    streams = [r3, long_id, r4, odt16, odt1040]
    rows = D.run(exe, [D.ctx_line(f) for f in streams])
    for f, row in zip(streams, rows):
        _ok(row, f)
    tail_blocks = [D.expected_words(f)[0][26] for f in (r3, long_id, r4)]      # R, n, u[12], h2[4], pad[8], tail_blocks
    assert tail_blocks == [1, 2, 1]                                    # a 16-byte ID: one block; 64 bytes: two
    assert b"\xff\xff\xff\xff\x80" in b"".join(w.to_bytes(4, "little") for w in D.expected_words(r4)[0][27:91])
    assert D.expected_words(odt16)[0][16:18] == [16, 16] and len(D.expected_words(odt16)[1]) == 4
    assert D.expected_words(odt1040)[0][16:18] == [1040, 1024] and len(D.expected_words(odt1040)[1]) == 256


# ---------------------------------------------------------------- (c) stream refusals
def _changed(base, changes):
    f = list(base)
    for k, v in zip(changes[0::2], changes[1::2]):
        f[k] = v
    return f


def _refused(exe, cases):
    """cases: (fields, code, the text the message must carry or None)."""
    rows = D.run(exe, [D.ctx_line(f) for f, _, _ in cases])
    for (f, code, name), row in zip(cases, rows):
        assert len(row) == 2 and int(row[0]) == code, (f[:4], row)
        assert name is None or name in row[1], (name, row[1])


def test_stream_refusals_of_the_gpu_tests(exe):
    import test_agile_gpu as A
    import test_gpu_parity as P
    import test_odf_legacy_gpu as L
    import test_oldoffice_gpu as O
    cases = []
    base = A.refusal_base()[1]
    cases += [(_changed(base, (k, v)), E_DOMAIN, name) for k, v, name in A.bad_streams(base).values()]
    for typ in O.REFUSAL_TYPES:
        base = O.refusal_base(typ)[1]
        cases += [(_changed(base, (k, v)), E_DOMAIN, name) for name, k, v in O.bad_streams(base)]
        # the hash length belongs to the type: 40 digits with type 1, 32 with type 3
        cases.append((_changed(base, (4, O.refusal_base(4 - typ)[1][4])), E_DOMAIN, "encryptedVerifierHash"))
    base = L.refusal_base()[1]
    cases += [(_changed(base, changes), E_DOMAIN, name) for name, *changes in L.bad_streams(base)]
    cases += [(f, E_DOMAIN, None) for f in P.DOMAIN_STREAMS]
    assert len(cases) == 5 + 2 * 14 + 22 + 2
    _refused(exe, cases)


def test_a_wrong_field_count_per_tag(exe):
    cases = []
    for label in ("office_2007", "agile_2013", "oldoffice_1", "odt", "odf", "pdf_r5"):
        f = D.case(label)[0]
        cases += [(f[:-1], E_INVALID, "tag '%s', %d fields" % (f[0], len(f) - 1)),
                  (f + ["00"], E_INVALID, "tag '%s', %d fields" % (f[0], len(f) + 1))]
    cases.append((["docx"] + D.case("office_2007")[0][1:], E_INVALID, "tag 'docx'"))
    _refused(exe, cases)


def test_owner_mode_needs_48_bytes_of_u(exe):
    from test_owner_gpu import short_u_fields
    f = short_u_fields()
    rows = D.run(exe, [D.ctx_line(f), "owner\t1", D.cand_line("x" * 65), "owner\t0"])
    assert _ok(rows[0], f)[0] == "pdf_r6"
    assert int(rows[1][0]) == E_DOMAIN and "U (40 bytes)" in rows[1][1] and rows[1][2] == "pdf_r6"    # still user mode
    assert rows[2] == ["0", "65", ""]
    assert rows[3] == ["0", "", "pdf_r6"]
    # U below the 40 bytes the user check reads: refused as a stream
    g = list(f)
    g[8], g[9] = "32", f[9][:64]
    _refused(exe, [(g, E_DOMAIN, "U shorter than 40")])


# ---------------------------------------------------------------- (d) candidates
def _cands(exe, label, cands, owner=False):
    f, _, family, _ = D.case(label)
    lines = [D.ctx_line(f)] + (["owner\t1"] if owner else []) + [D.cand_line(c) for c in cands]
    rows = D.run(exe, lines)
    assert rows[0][:2] == ["0", family]
    if owner:
        assert rows[1] == ["0", "", family + "_owner"]
    return [(int(r[0]), int(r[1]), r[2]) for r in rows[len(lines) - len(cands):]]


@pytest.mark.parametrize("label", ["office_2007", "agile_2010", "agile_2013", "oldoffice_0", "oldoffice_1", "oldoffice_3",
                                   "oldoffice_4"])
def test_office_candidates(exe, label):
    family = D.case(label)[2]
    got = _cands(exe, label, ["z" * 32, "z" * 33, "é" * 32, "é" * 33, "", b"\xff\xfe", b"a\0b", "\U0001f600" * 16,
                              "z" * (D.MAX_PW + 1)])
    # Office 2007 has a long list: over 32 UTF-16 units is served; the families without one refuse with their sentence
    over = (0, 66, "") if family == "office_std" else (E_PWLEN, 66, NO_LONG[family])
    assert got == [(0, 64, ""), over, (0, 64, ""), over,                  # units count, not UTF-8 bytes
                   (E_DOMAIN, 0, UNDEFINED), (E_DOMAIN, 2, UNDEFINED),    # empty; invalid UTF-8
                   (E_INVALID, 0, NUL),
                   (0, 64, ""),                                           # 16 surrogate pairs fill the slot
                   (E_PWLEN, 0, TOO_LONG)]


def test_byte_candidates(exe):
    e = [b"y" * 64, b"y" * 65, b"", b"a\0b"]
    assert _cands(exe, "odt", e) == [(0, 64, ""), (0, 65, ""), (0, 0, ""), (E_INVALID, 0, NUL)]
    assert _cands(exe, "odf", e) == [(0, 64, ""), (E_PWLEN, 65, NO_LONG["odf_bf_sha1"]), (0, 0, ""), (E_INVALID, 0, NUL)]
    for label in ("pdf_r2", "pdf_r3_40", "pdf_r4_meta0"):                  # cut to 32 bytes: never long
        assert _cands(exe, label, [b"y" * 32, b"y" * 33, b"y" * 65, b"y" * D.MAX_PW, b"a\0b"]) == \
            [(0, 32, ""), (0, 32, ""), (0, 32, ""), (0, 32, ""), (E_INVALID, 0, NUL)]
    assert _cands(exe, "pdf_r5", [b"y" * 64, b"y" * 65, b"y" * 127, b"y" * 128, b"y" * (D.MAX_PW + 1)]) == \
        [(0, 64, ""), (0, 65, ""), (0, 127, ""), (0, 127, ""), (E_PWLEN, 0, TOO_LONG)]
    got = _cands(exe, "pdf_r6", [b"y" * 65, b"y" * 176, b"y" * 177])
    assert got == [(0, 65, ""), (0, 176, ""), (E_DOMAIN, 177, UNDEFINED)] and "176" in got[2][2]


def test_owner_candidates(exe):
    assert _cands(exe, "pdf_r3_128", [b"y" * 64, b"y" * 65], owner=True) == [(0, 32, ""), (0, 32, "")]
    assert _cands(exe, "pdf_r5", [b"y" * 64, b"y" * 65, b"y" * 128], owner=True) == \
        [(0, 64, ""), (E_PWLEN, 65, NO_LONG_OWNER), (E_PWLEN, 127, NO_LONG_OWNER)]
    assert _cands(exe, "pdf_r6", [b"y" * 64, b"y" * 65, b"y" * 177], owner=True) == \
        [(0, 64, ""), (E_PWLEN, 65, NO_LONG_OWNER), (E_DOMAIN, 177, UNDEFINED)]
