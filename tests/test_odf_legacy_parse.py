"""ODF 1.0 / 1.1 (Blowfish-CFB, SHA-1) support as far as it runs without a GPU: odt2hashes on the packages of
tests/odf_legacy_docgen.py (the `$odf$` stream, the entry-selection rules, the refusals, ODF 1.2 unchanged),
parse_verification_data's 12 fields, and the host-visible surface (dprf_plan_chunk knows "odf_bf_sha1", the header
documents the stream, the resource gate holds both kernels at 0 B of scratch).  dprf_ctx_create looks for its device
before it reads the fields, so its refusals are tested on the GPU (tests/test_odf_legacy_gpu.py)."""
import contextlib
import io
import os
import random
import re
import sys

import pytest

import odf_legacy_docgen as G
import odf_legacy_model as M
from conftest import GOLDEN, REPO, load_golden

FAMILY = "odf_bf_sha1"
CSRC = os.path.join(REPO, "dprf_amd", "csrc")
HUGE = 1 << 40
PW = "Ux7"


def _parse(stream):
    from dprf_amd.brute_force import parse_verification_data
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        return parse_verification_data(stream), out.getvalue()


def _hashes(path, **kw):
    from dprf_amd.parsers import odt2hashes
    return odt2hashes.get_hashes(path, **kw)


@pytest.fixture(scope="module")
def package(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("odf11")), "old.odt")
    return path, G.write_odf11(path, PW, seed=0x0DF)


# ---------------------------------------------------------------- the parser on docgen's files
def test_parser_prints_the_stream_the_model_verifies(package):
    path, entries = package
    salt, iv, checksum, enc = entries["content.xml"]
    assert len(enc) > 1024                                          # the docgen's content.xml deflates to more than 1 KiB
    got = _hashes(path)
    assert got == "old.odt:" + M.format_stream(1024, checksum, iv, salt, enc[:1024])
    assert re.match(r"old\.odt:\$odf\$\*0\*0\*1024\*16\*[0-9a-f]{40}\*8\*[0-9a-f]{16}\*16\*[0-9a-f]{32}\*0\*[0-9a-f]{2048}$", got)
    assert M.verifies(got, PW) and not M.verifies(got, "Ux8")
    assert _hashes(path, experimental=True) == got                  # -e changes nothing for this scheme


def test_package_is_an_odf_1_1_package(package):
    import zipfile
    path, entries = package
    with zipfile.ZipFile(path) as z:
        manifest = z.read("META-INF/manifest.xml").decode()
        assert "manifest:version" not in manifest
        assert manifest.count('manifest:algorithm-name="Blowfish CFB"') == len(entries) == 3
        assert manifest.count('manifest:checksum-type="SHA1/1K"') == 3 and 'manifest:iteration-count="1024"' in manifest
        for name in entries:
            assert z.getinfo(name).compress_type == zipfile.ZIP_STORED
            assert z.read(name) == entries[name][3]


def test_urn_spelling_and_iteration_count(tmp_path):
    path = os.path.join(str(tmp_path), "urn.odt")
    G.write_odf11(path, PW, seed=3, iterations=3, algorithm=G.BLOWFISH_URN,
                  checksum_type="urn:oasis:names:tc:opendocument:xmlns:manifest:1.0#sha1-1k")
    got = _hashes(path)
    assert got.startswith("urn.odt:$odf$*0*0*3*16*")
    assert M.verifies(got, PW) and not M.verifies(got, "ux7")


def _files(rng, sizes):
    """[(name, plain)] whose deflated sizes are about 3 bytes per word"""
    return [(name, ("<x>%s</x>" % G._noise(rng, words)).encode()) for name, words in sizes]


def test_entry_selection(tmp_path):
    t = str(tmp_path)
    rng = random.Random(7)
    # content.xml short: the smallest entry by manifest size with at least 1024 stored bytes, ties in manifest order
    big = ("<x>%s</x>" % G._noise(rng, 900)).encode()
    same = ("<y>%s</y>" % G._noise(rng, 900)).encode()
    assert len(big) == len(same)
    files = [("content.xml", b"<short/>"), ("Pictures/huge.xml", big + big), ("styles.xml", big), ("settings.xml", same),
             ("meta.xml", b"<m/>")]
    path = os.path.join(t, "pick.odt")
    entries = G.write_odf11(path, PW, seed=11, files=files)
    salt, iv, checksum, enc = entries["styles.xml"]
    assert len(entries["content.xml"][3]) < 1024 <= len(entries["settings.xml"][3])
    assert _hashes(path) == "pick.odt:" + M.format_stream(1024, checksum, iv, salt, enc[:1024])
    # content.xml with at least 1024 stored bytes wins over a smaller entry
    files = [("styles.xml", ("<x>%s</x>" % G._noise(rng, 500)).encode()), ("content.xml", big)]
    path = os.path.join(t, "content.odt")
    entries = G.write_odf11(path, PW, seed=12, files=files)
    assert len(entries["styles.xml"][3]) >= 1024 and len(files[0][1]) < len(big)
    salt, iv, checksum, enc = entries["content.xml"]
    assert _hashes(path) == "content.odt:" + M.format_stream(1024, checksum, iv, salt, enc[:1024])


def test_parser_refusals(tmp_path):
    t = str(tmp_path)
    path = os.path.join(t, "short.odt")
    G.write_odf11(path, PW, seed=13, files=[("content.xml", b"<short/>"), ("meta.xml", b"<m/>")])
    with pytest.raises(ValueError) as ei:
        _hashes(path)
    assert "at least 1024 stored bytes" in str(ei.value)
    path = os.path.join(t, "des.odt")
    G.write_odf11(path, PW, seed=14, algorithm="Triple DES CBC")
    with pytest.raises(ValueError) as ei:
        _hashes(path)
    assert "Triple DES CBC" in str(ei.value)
    path = os.path.join(t, "sha256.odt")
    G.write_odf11(path, PW, seed=15, checksum_type="SHA256/1K")
    with pytest.raises(ValueError) as ei:
        _hashes(path)
    assert "SHA256/1K" in str(ei.value)


def test_odf_1_2_documents_print_what_they_printed(tmp_path):
    import docgen
    docs = load_golden("docs.json")
    seen = 0
    for name, e in docs.items():
        if e["kind"] == "odt":
            for key, exp in (("std", False), ("e", True)):
                if key in e["streams"]:
                    assert _hashes(os.path.join(GOLDEN, "docs", name), experimental=exp) == e["streams"][key]["stream"], name
                    seen += 1
    assert seen >= 1
    path = os.path.join(str(tmp_path), "new.odt")
    docgen.write_odt(path, "pw", 5)
    got = _hashes(path)
    assert got.startswith("new.odt:$odt$*1.2*") and len(_parse(got)[0]) == 7


# ---------------------------------------------------------------- parse_verification_data
def test_twelve_fields_with_and_without_prefix_and_tail():
    s = M.make_stream(PW, 2, seed=1)
    f = M.split_stream(s)
    want = ["odf", "0", "0", "2", "16", f[4], "8", f[6], "16", f[8], "0", f[10]]
    for stream in (s, "old.odt:" + s, "dir/a:b.odt:" + s, s + ":::::old.odt", "old.odt:" + s + ":::x::y"):
        assert _parse(stream)[0] == want, stream[:40]


@pytest.mark.parametrize("stream", ["x.odt:$odf$*0*0*1024*16*00*8*11*16*22*0",           # eleven fields
                                    "x.odt:$odf$*0*0*1024*16*00*8*11*16*22*0*33*44",     # thirteen
                                    "x.odt:$odg$*0*0*1024*16*00*8*11*16*22*0*33"])
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


# ---------------------------------------------------------------- the ABI without a device
def test_plan_chunk_knows_the_family():
    from dprf_amd import _lib
    first = _lib.plan_chunk(FAMILY, 0.0, HUGE, HUGE, 1)
    assert first != 0, "dprf_plan_chunk does not know %s" % FAMILY
    assert _lib.plan_chunk(FAMILY, 0, 1, 1, 1, 0) == 1              # the support probe of include/dprf.h
    assert first == _lib.plan_chunk("odf_aes256", 0.0, HUGE, HUGE, 1) == 1 << 22   # ODF 1.2's row
    for rate in (0.05, 1.0, 100.0, 1e4, 1e8):
        n = _lib.plan_chunk(FAMILY, rate, HUGE, HUGE, 1)
        assert 1 << 19 <= n <= 1 << 23 and n & (n - 1) == 0, (rate, n)
    assert _lib.plan_chunk(FAMILY, 16400.0, 1000, HUGE, 1) == 1000
    assert _lib.plan_chunk("odf_bf", 0.0, HUGE, HUGE, 1) == 0
    assert _lib.lib().dprf_abi_version() == 9                       # no export or struct changed


def test_chunk_policy_shapes(monkeypatch):
    """tests/test_chunk_policy.py's checks for this family: eight simulated devices finish every round together, a small
    call spreads over every device, rounds stay within the checkpoint bound.  The rate is ODF 1.2's: the policy row is
    the same, and the shapes do not depend on it."""
    import test_chunk_policy as T
    from dprf_amd import _lib, brute_force as bf
    monkeypatch.setitem(T.RATES, FAMILY, T.RATES["odf_aes256"])
    for r, rd in enumerate(T.run_search(_lib, FAMILY, 8, 4)):
        mean = sum(rd["finish"]) / 8
        assert max(rd["finish"]) <= 1.05 * mean and min(rd["launches"]) >= 1, (r, rd)
    for r, rd in enumerate(T.run_search(_lib, FAMILY, 8, 3, rate_spread=0.2)):
        assert max(rd["finish"]) <= 1.05 * sum(rd["finish"]) / 8, (r, rd)
    for n in (20000, 1 << 20):
        finish, cands, launches = T.simulate_call(_lib, FAMILY, n, [T.RATES[FAMILY][0]] * 8, 0.05, [0.0] * 8)
        assert sum(cands) == n and min(cands) > 0 and max(cands) <= 2 * n / 8 + 4096, (n, cands)
    for ndev in (1, 2, 8):
        for r, rd in enumerate(T.run_search(_lib, FAMILY, ndev, 4)):
            assert rd["wall_ms"] <= 1.15 * bf.ROUND_MAX_SECONDS * 1e3, (ndev, r, rd["wall_ms"])


def test_header_documents_the_stream():
    text = open(os.path.join(REPO, "include", "dprf.h")).read()
    assert '"%s"' % FAMILY in text and '"odf"' in text and "$odf$*0*0*" in text
    assert re.search(r"#define DPRF_ABI_VERSION 9\b", text) and re.search(r"#define DPRF_ODF_MAX_ITER 10000000\b", text)
    for out_of_scope in ("shorter than 1024", ".sxw", "$odf$*1*1*", "over 64 bytes", "decrypting the document"):
        assert out_of_scope in text, out_of_scope


def test_check_kernel_shape():
    """What the GPU tests size their windows by, and what the LDS layout needs: 32 columns of 1,024 words, and KDF
    blocks that are whole check blocks."""
    text = open(os.path.join(CSRC, "dprf_kernels_odf.hip")).read()
    cands = int(re.search(r"#define ODF_BF_CANDS (\d+)", text).group(1))
    kdf = int(re.search(r"#define ODF_KDF_THREADS (\d+)", text).group(1))
    assert cands == 32 and kdf % cands == 0 and 4096 * cands <= 160 * 1024


def test_resource_gate_holds_the_kernels_at_zero():
    sys.path.insert(0, CSRC)
    try:
        import resource_gate
    finally:
        sys.path.remove(CSRC)
    assert resource_gate.SCRATCH_LIMIT.get("k_odf_bf_kdf") == 0 and resource_gate.SCRATCH_LIMIT.get("k_odf_bf_check") == 0


def test_built_object_reports_no_scratch():
    gate = os.path.join(REPO, "build", "obj", "dprf_kernels_odf.o.gate")
    assert os.path.exists(gate), "no gate report of the ODF 1.0 / 1.1 object: run build() first"
    rows = [ln.split() for ln in open(gate).read().splitlines() if ln.strip()]
    seen = set()
    for r in rows:
        assert r[0] == "ok", r
        name = " ".join(r[1:r.index("VGPRs")])
        assert r[r.index("scratch") + 1] == "0", r
        seen.add(re.sub(r"^void ", "", name).split("<")[0])
    assert seen == {"k_odf_bf_kdf", "k_odf_bf_check"}
    assert len(rows) == 3                                           # two candidate sources of the KDF, one check
