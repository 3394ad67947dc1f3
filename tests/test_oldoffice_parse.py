"""Office 97-2003 RC4 support as far as it runs without a GPU: parse_verification_data's two spellings, the .doc / .xls
cases of dprf_amd/parsers/office2john.py on the fixtures of tests/oldoffice_docgen.py, and the host-visible surface
(the chunk policy knows both families, the header documents the stream, the resource gate holds k_oldoffice at 0 B of
scratch).  dprf_ctx_create looks for its device before it reads the fields, so its refusals are tested on the GPU
(tests/test_oldoffice_gpu.py (g))."""
import contextlib
import io
import os
import re
import sys

import pytest

import oldoffice_docgen as G
import oldoffice_model as M
from conftest import GOLDEN, REPO, load_golden

FAMILIES = ["office_rc4_md5", "office_rc4_sha1"]
CSRC = os.path.join(REPO, "dprf_amd", "csrc")
HUGE = 1 << 40
PW = "Ux7"


def _parse(stream):
    from dprf_amd.brute_force import parse_verification_data
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        return parse_verification_data(stream), out.getvalue()


# ---------------------------------------------------------------- parse_verification_data
@pytest.mark.parametrize("typ", M.TYPES)
def test_both_spellings_and_a_tail_give_the_same_five_fields(typ):
    salt, ev, evh = M.make_parts(PW, typ, 31 + typ)
    want = ["oldoffice", str(typ), salt.hex(), ev.hex(), evh.hex()]
    john = M.stream_of(typ, salt, ev, evh, spelling="john")
    hashcat = M.stream_of(typ, salt, ev, evh, spelling="hashcat")
    for s in (john, hashcat, john + ":::a summary::/tmp/made.doc", hashcat + ":::x::y",
              hashcat.split(":", 1)[1]):                           # hashcat's own form has no file name in front
        assert _parse(s)[0] == want, s
        assert M.fields_of(s) == want


def test_public_vectors_parse():
    for v in load_golden("oldoffice_vectors.json").values():
        f, _ = _parse(v["stream"])
        assert f[0] == "oldoffice" and len(f) == 5 and M.verifies(f, v["password"])


@pytest.mark.parametrize("stream", [
    "x.doc:$oldoffice$1*00*11",                                     # three pieces
    "x.doc:$oldoffice$*1*00*11",                                    # four, the other spelling
    "x.doc:$oldoffice$1*00*11*22*33",                               # five pieces with the type glued on: six fields
    "x.doc:$oldoffice$*1*00*11*22*33",
    "x.doc:$oldoffice$*00*11*22",                                   # no type
    "x.doc:$newoffice$*1*00*11*22",
])
def test_wrong_piece_counts_exit_1(stream):
    from dprf_amd.brute_force import parse_verification_data
    out = io.StringIO()
    with contextlib.redirect_stdout(out), pytest.raises(SystemExit) as ei:
        parse_verification_data(stream)
    assert ei.value.code == 1 and "The input data is not supported." in out.getvalue()


def test_other_tags_parse_as_before(streams):
    for name in ("office_synth_ok", "odt_synth_e_ab", "pdf_synth_r5_cat"):
        f, _ = _parse(streams[name]["stream"])
        assert f[0] in ("office", "odt", "pdf") and len(f) == {"office": 8, "odt": 7, "pdf": 12}[f[0]]


# ---------------------------------------------------------------- the parser on docgen's files
@pytest.mark.parametrize("kind,typ", [("doc", 1), ("doc", 3), ("doc", 4), ("xls", 0), ("xls", 3), ("xls", 4)])
def test_parser_prints_the_stream_the_writer_was_given(tmp_path, kind, typ):
    from dprf_amd.parsers import office2john
    path = os.path.join(str(tmp_path), "old." + kind)
    want = (G.write_doc if kind == "doc" else G.write_xls)(path, PW, typ, 0xD0C + typ)
    got = office2john.get_hash(path)
    assert got == want == M.make_stream(PW, typ, 0xD0C + typ, name="old." + kind)
    assert re.match(r"old\.%s:\$oldoffice\$%d\*[0-9a-f]{32}\*[0-9a-f]{32}\*[0-9a-f]{%d}$" % (kind, typ, 32 if typ < 2 else 40),
                    got)
    assert M.verifies(got, PW) and not M.verifies(got, "Ux8")
    assert _parse(got)[0][1] == str(typ)


def test_doc_table_stream_is_the_one_the_fib_names(tmp_path):
    """fWhichTblStm = 0: the header is read from 0Table (the reference always opens 1Table)."""
    from dprf_amd.parsers import office2john
    path = os.path.join(str(tmp_path), "zero.doc")
    want = G.write_doc(path, PW, 1, 5, which=0)
    assert office2john.get_hash(path) == want


def test_parser_refusals(tmp_path):
    from dprf_amd.parsers import office2john
    t = str(tmp_path)
    G.write_doc_plain(os.path.join(t, "plain.doc"))
    G.write_doc_plain(os.path.join(t, "xor.doc"), xor=True)
    G.write_xls_xor(os.path.join(t, "xor.xls"))
    G.write_ppt(os.path.join(t, "deck.ppt"))
    for name, what in (("plain.doc", "not encrypted"), ("xor.doc", "XOR obfuscation"), ("xor.xls", "XOR obfuscation"),
                       ("deck.ppt", "PowerPoint 97-2003 is not supported")):
        with pytest.raises(ValueError) as ei:
            office2john.get_hash(os.path.join(t, name))
        assert what in str(ei.value), (name, str(ei.value))


def test_cryptoapi_size_asserts(tmp_path):
    """Salt size 16 and verifier hash size 20, as the reference asserts."""
    import struct
    import docgen
    from dprf_amd.parsers import office2john
    salt, ev, evh = M.make_parts(PW, 4, 3)
    good = G._cryptoapi(4, salt, ev, evh)
    at = len(good) - 60                                             # saltSize, salt, ev, hashSize, evh
    for off, val, what in ((at, 8, "salt size"), (at + 36, 16, "verifier hash size")):
        bad = good[:off] + struct.pack("<I", val) + good[off + 4:]
        path = os.path.join(str(tmp_path), "bad%d.doc" % off)
        with open(path, "wb") as f:
            f.write(docgen._cfb({"WordDocument": G._fib(0x01), "1Table": struct.pack("<HH", 2, 2) + bad}))
        with pytest.raises(ValueError) as ei:
            office2john.get_hash(path)
        assert what in str(ei.value)


def test_docx_fixtures_still_print_what_they_printed():
    from dprf_amd.parsers import office2john
    docs = load_golden("docs.json")
    seen = 0
    for name, e in docs.items():
        if e["kind"] == "docx":
            assert office2john.get_hash(os.path.join(GOLDEN, "docs", name)) == e["streams"]["std"]["stream"], name
            seen += 1
    assert seen >= 1


# ---------------------------------------------------------------- the ABI without a device
@pytest.mark.parametrize("family", FAMILIES)
def test_plan_chunk_knows_the_families(family):
    from dprf_amd import _lib
    first = _lib.plan_chunk(family, 0.0, HUGE, HUGE, 1)
    assert first != 0, "dprf_plan_chunk does not know %s" % family
    assert _lib.plan_chunk(family, 0, 1, 1, 1, 0) == 1              # the support probe of include/dprf.h
    assert first == _lib.plan_chunk("pdf_r24", 0.0, HUGE, HUGE, 1)  # pdf_r24's row
    for rate in (0.05, 1.0, 100.0, 1e5, 1e8):
        n = _lib.plan_chunk(family, rate, HUGE, HUGE, 1)
        assert 1 << 20 <= n <= 1 << 30 and n & (n - 1) == 0, (rate, n)
    assert _lib.plan_chunk("office_std", 0.0, HUGE, HUGE, 1) == 1 << 19
    assert _lib.plan_chunk("office_rc4", 0.0, HUGE, HUGE, 1) == 0
    assert _lib.lib().dprf_abi_version() == 9                       # no export or struct changed


def test_header_documents_the_stream():
    text = open(os.path.join(REPO, "include", "dprf.h")).read()
    for family in FAMILIES:
        assert '"%s"' % family in text
    assert '"oldoffice"' in text and "2.3.6" in text and "2.3.5" in text
    assert re.search(r"#define DPRF_ABI_VERSION 9\b", text)
    for out_of_scope in ("PowerPoint", "XOR obfuscation", "9710", "type 5"):
        assert out_of_scope in text, out_of_scope


def test_resource_gate_holds_the_kernel_at_zero():
    sys.path.insert(0, CSRC)
    try:
        import resource_gate
    finally:
        sys.path.remove(CSRC)
    assert resource_gate.SCRATCH_LIMIT.get("k_oldoffice") == 0


def test_built_object_reports_no_scratch():
    gate = os.path.join(REPO, "build", "obj", "dprf_kernels_oldoffice.o.gate")
    assert os.path.exists(gate), "no gate report of the Office 97-2003 object: run build() first"
    rows = [ln.split() for ln in open(gate).read().splitlines() if ln.strip()]
    seen = set()
    for r in rows:
        assert r[0] == "ok", r
        name = " ".join(r[1:r.index("VGPRs")])
        assert r[r.index("scratch") + 1] == "0", r
        seen.add(re.sub(r"^void ", "", name).split("<")[0])
    assert seen == {"k_oldoffice"}
    assert len(rows) == 4                                           # two candidate sources x two hashes
