"""ODF 1.2 at the manifest's PBKDF2 iteration count (the "$odf$*1*1*" stream, kernel family "odf_aes_sha256") without a
device: the model the GPU tests compare against, the parser branch, the document layer and the work counts.

  (a) the model (tests/odf12_docgen.py verifies) at 1024 iterations against the oracle -- and the reference verifier,
      where it is built -- on the "$odt$" stream of the same document; away from 1024 it answers by its count
  (b) odt2hashes: 1024 or no count gives the "$odt$" line as ever, any other count the "$odf$*1*1*" line; both
      manifest spellings, the entry choice, every ValueError
  (c) the document layer through tests/host/odf12_check.cpp, built with g++ alone: family row, format, flags, every
      kernel-argument word, every refusal and its message, a long candidate, the first chunk by count
  (d) the ABI without a device, the work counts, the build's resource report"""
import contextlib
import hashlib
import io
import os
import re
import subprocess
import sys

import pytest

import doc_layer as D
import odf12_docgen as G
from conftest import REPO

CSRC = os.path.join(REPO, "dprf_amd", "csrc")
FAMILY = "odf_aes_sha256"
PW = "Ux7"
MAX_ITER = 10000000
HUGE = 1 << 40
GENERATION = 256 * 4 * 5 * 64        # resident lanes of the KDF kernel: CUs x SIMDs x waves per SIMD x lanes


def _parse(stream):
    from dprf_amd.brute_force import parse_verification_data
    with contextlib.redirect_stdout(io.StringIO()):
        return parse_verification_data(stream)


# ---------------------------------------------------------------- (a) the model
def _flip_bit(hexfield, pos, bit):
    raw = bytearray(bytes.fromhex(hexfield))
    raw[pos] ^= 1 << bit
    return bytes(raw).hex()


def _reference_verdict(fields, pw):
    """The reference verifier's own verdict (exit status 1: verified), or None where it is not built"""
    exe = os.path.join(REPO, "oracle", "_ref", "odt")
    if not os.path.exists(exe):
        return None
    f = fields
    return subprocess.run([exe, pw, f[2], f[3], f[4], f[5], str(f[6])], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL).returncode


def test_model_equals_the_oracle_at_1024(oracle, tmp_path):
    path = os.path.join(str(tmp_path), "d.odt")
    e = G.write_odt12(path, PW, seed=0x0DF12, iterations=1024)["content.xml"]
    assert e["deflated"] >= 1024
    odt, odf = G.odt_stream(e), G.odf_stream(e, 1024)
    bad_ck = _flip_bit(e["checksum"].hex(), 17, 3)
    cases = [(odt, odf)]
    cases.append((odt.replace(e["checksum"].hex(), bad_ck), odf.replace(e["checksum"].hex(), bad_ck)))
    seen = []
    for s_odt, s_odf in cases:
        ctx = oracle.Ctx(s_odt)
        for pw in (PW, "Ux8", ""):
            want = ctx.verify(pw)
            assert int(G.verifies(s_odf, pw)) == want, (pw, want)
            ref = _reference_verdict(oracle.split_stream(s_odt), pw)
            assert ref in (None, want), (pw, ref, want)
            seen.append(want)
    assert seen == [1, 0, 0, 0, 0, 0]


def test_model_answers_by_its_count():
    assert G.key("x", b"s" * 16, 1024) == hashlib.pbkdf2_hmac("sha1", hashlib.sha256(b"x").digest(), b"s" * 16, 1024, 32)
    import docgen
    assert docgen.odt_key("x", b"s" * 16) == G.key("x", b"s" * 16, 1024)
    for c in (1, 2, 3, 1025):
        s = G.make_stream(PW, c, seed=c)
        f = G.fields_of(s)
        assert f[:5] == ["odf", "1", "1", str(c), "32"] and [len(f[k]) for k in (5, 7, 9, 11)] == [64, 32, 32, 2048]
        assert G.verifies(s, PW) and not G.verifies(s, "Ux8")
        for other in (c + 1, max(1, c - 1) if c > 1 else 2):
            g = list(f)
            g[3] = str(other)
            assert not G.verifies(g, PW), (c, other)
    assert G.verifies(G.make_stream(b"\xff\xfe\x80", 2, seed=9), b"\xff\xfe\x80")


# ---------------------------------------------------------------- (b) the parser
def _write(tmp_path, name, **kw):
    path = os.path.join(str(tmp_path), name)
    return path, G.write_odt12(path, PW, seed=0x12C, **kw)


def _parent_odt_line(path, experimental):
    """What odt2hashes printed for an AES-256-CBC package before the count was read: the reference's selection
    (odt2hashes.py:53-86) restated -- the smallest entry whose manifest size exceeds the limit, the whole entry in hex"""
    import base64
    import xml.etree.ElementTree as et
    import zipfile
    ns = "{urn:oasis:names:tc:opendocument:xmlns:manifest:1.0}"
    with zipfile.ZipFile(path) as z:
        root = et.fromstring(z.read("META-INF/manifest.xml"))
        best = None
        for fe in root.iter(ns + "file-entry"):
            size = fe.get(ns + "size")
            if size is not None and int(size) > (-1 if experimental else 1024) and \
                    (best is None or int(size) < int(best.get(ns + "size"))):
                best = fe
        enc = best.find(ns + "encryption-data")
        data = z.read(best.get(ns + "full-path"))
        d = lambda s: base64.b64decode(s).hex()
        return "%s:$odt$*%s*%s*%s*%s*%s*%d" % (
            os.path.basename(path), root.get(ns + "version"), d(enc.get(ns + "checksum")),
            d(enc.find(ns + "algorithm").get(ns + "initialisation-vector")),
            d(enc.find(ns + "key-derivation").get(ns + "salt")), data.hex(), len(data))


@pytest.mark.parametrize("spelling", ["urn", "short"])
def test_1024_or_no_count_prints_the_odt_line(tmp_path, spelling):
    from dprf_amd.parsers import odt2hashes
    for name, over in (("c1024.odt", {}), ("nocount.odt", {"count": None})):
        path, entries = _write(tmp_path, spelling + name, iterations=1024, spelling=spelling, **over)
        for experimental in (False, True):
            line = odt2hashes.get_hashes(path, experimental)
            assert line == _parent_odt_line(path, experimental), (name, experimental)
            assert "$odt$*1.2*" in line and "$odf$" not in line
        # -e takes the empty entry (16 bytes of padding), the plain call styles.xml: the smaller of the two over 1024
        assert odt2hashes.get_hashes(path, True).endswith("*16")
        assert entries["styles.xml"]["enc"].hex() in odt2hashes.get_hashes(path, False)
    # the package tests/docgen.py writes, which says 1024: untouched
    import docgen
    path = os.path.join(str(tmp_path), "old.odt")
    docgen.write_odt(path, PW, 5)
    assert odt2hashes.get_hashes(path) == _parent_odt_line(path, False)


@pytest.mark.parametrize("spelling", ["urn", "short"])
@pytest.mark.parametrize("c", [100000, 3])
def test_other_counts_print_the_odf_line(tmp_path, spelling, c):
    from dprf_amd.parsers import odt2hashes
    path, entries = _write(tmp_path, "c.odt", iterations=c, spelling=spelling)
    e = entries["content.xml"]
    for experimental in (False, True):                                     # -e changes nothing on this branch
        line = odt2hashes.get_hashes(path, experimental)
        assert line == G.odf_stream(e, c, name="c.odt")
    f = _parse(line)
    assert f == ["odf", "1", "1", str(c), "32", e["checksum"].hex(), "16", e["iv"].hex(), "16", e["salt"].hex(), "0",
                 e["enc"][:1024].hex()]
    assert f == G.fields_of(line)
    assert G.verifies(f, PW) and not G.verifies(f, "Ux8")
    from dprf_amd import brute_force
    with contextlib.redirect_stdout(io.StringIO()):
        assert brute_force.get_verification_data("2", path) == line


def test_entry_choice(tmp_path):
    """content.xml if it has at least 1024 stored bytes, else the smallest entry that has"""
    from dprf_amd.parsers import odt2hashes
    path, entries = _write(tmp_path, "small.odt", iterations=7, content_words=40, styles_words=700)
    assert len(entries["content.xml"]["enc"]) < 1024 <= len(entries["styles.xml"]["enc"])
    assert odt2hashes.get_hashes(path) == G.odf_stream(entries["styles.xml"], 7, name="small.odt")
    path, entries = _write(tmp_path, "big.odt", iterations=7, content_words=900, styles_words=400)
    assert 1024 <= len(entries["styles.xml"]["enc"]) < len(entries["content.xml"]["enc"])
    assert odt2hashes.get_hashes(path) == G.odf_stream(entries["content.xml"], 7, name="big.odt")
    path, _ = _write(tmp_path, "none.odt", iterations=7, content_words=40, styles_words=40)
    with pytest.raises(ValueError, match="at least 1024 stored bytes"):
        odt2hashes.get_hashes(path)


ARGON2ID = "urn:org:documentfoundation:names:experimental:office:manifest:argon2id"
AES_GCM = "http://www.w3.org/2009/xmlenc11#aes256-gcm"


@pytest.mark.parametrize("over,named", [
    ({"checksum_type": "SHA1/1K"}, "checksum type 'SHA1/1K'"),
    ({"checksum_type": None}, "checksum type None"),
    ({"skg_name": "SHA1"}, "start key generation 'SHA1'"),
    ({"skg_size": "20"}, "key size '20'"),
    ({"kd_name": ARGON2ID}, "argon2id"),
    ({"kd_size": "16"}, "derived key size '16'"),
    ({"algorithm": AES_GCM}, "aes256-gcm"),
    ({"checksum": b"c" * 20}, "20-byte checksum"),
    ({"iv": b"i" * 8}, "8-byte iv"),
    ({"salt": b"s" * 32}, "32-byte salt"),
    ({"count": "0"}, "iteration count 0"),
])
def test_parser_refusals(tmp_path, over, named):
    from dprf_amd.parsers import odt2hashes
    path, _ = _write(tmp_path, "bad.odt", iterations=5, **over)
    with pytest.raises(ValueError) as ei:
        odt2hashes.get_hashes(path)
    assert named in str(ei.value), str(ei.value)


def test_argon2id_is_refused_at_any_count(tmp_path):
    """An Argon2id package has no PBKDF2 count at all: it must not fall through to the "$odt$" line"""
    from dprf_amd.parsers import odt2hashes
    for over in ({"count": None}, {"count": "1024"}):
        path, _ = _write(tmp_path, "argon.odt", iterations=3, kd_name=ARGON2ID, **over)
        with pytest.raises(ValueError, match="argon2id"):
            odt2hashes.get_hashes(path, True)


# ---------------------------------------------------------------- (c) the document layer
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """tests/host/odf12_check.cpp and dprf_doc.cpp with g++ and nothing else.  DPRF_ODF12_CHECK names a program built by
    hand instead (the same two sources with -fsanitize=address,undefined)."""
    if os.environ.get("DPRF_ODF12_CHECK"):
        return os.environ["DPRF_ODF12_CHECK"]
    out = os.path.join(str(tmp_path_factory.mktemp("odf12_check")), "odf12_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(REPO, "tests", "host", "odf12_check.cpp"),
                    os.path.join(CSRC, "dprf_doc.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def base():
    return G.fields_of(G.make_stream(PW, 100000, seed=0xBA5E))


def test_family_row_and_every_argument_word(exe, base):
    for c in ("1", "1024", "100000", str(MAX_ITER)):
        f = list(base)
        f[3] = c
        row = D.run(exe, [D.ctx_line(f)])[0]
        assert row[:4] == ["0", FAMILY, "2", "0"], row[:4]                  # DPRF_FMT_ODT, no flag
        # 8 key words, DPRF_LONG_SHA256 (2) with keys written, one stream; no owner / key-search / collider name and
        # no refusal sentence for long candidates
        assert row[4] == "8 2 1 1 ----"
        h = bytes.fromhex
        # dprf_odt_params as k_odt_check reads it: checksum, iv, salt, enc_len, hash_len, a null pointer
        assert D.words(row[5]) == D.be(h(f[5])) + D.be(h(f[7])) + D.be(h(f[9])) + [1024, 1024, 0, 0]
        assert D.words(row[6]) == D.be(h(f[9])) + [int(c)]                   # dprf_odf_aes_params: salt, iterations
        assert D.words(row[7]) == D.be(h(f[11])) and len(D.words(row[7])) == 256
        assert row[8] == c
    # a leading 00 byte flags nothing here: no reference verifier reads this stream
    f = list(base)
    f[9] = "00" + f[9][2:]
    assert D.run(exe, [D.ctx_line(f)])[0][:4] == ["0", FAMILY, "2", "0"]


def bad_streams(base):
    """What is refused with DPRF_E_DOMAIN, as changes to `base`: (what the message carries, field index, value).
    tests/test_odf12_iter_gpu.py sends the same list to dprf_ctx_create."""
    return [
        ("key size", 4, "16"), ("key size", 4, ""), ("iv length", 6, "8"), ("salt length", 8, "32"), ("inplace", 10, "1"),
        ("iterations", 3, "0"), ("iterations", 3, str(MAX_ITER + 1)), ("iterations", 3, ""), ("iterations", 3, "1k"),
        ("iterations", 3, "-5"), ("iterations", 3, "1234567890"),
        ("checksum", 5, base[5][:-2]), ("checksum", 5, base[5] + "00"), ("checksum", 5, "g" + base[5][1:]),
        ("checksum", 5, base[5][:40]),
        ("iv", 7, base[7][:-2]), ("iv", 7, base[7][:16]), ("iv", 7, base[7][:5] + "x" + base[7][6:]),
        ("salt", 9, base[9] + "ab"), ("salt", 9, base[9][:-1] + "z"),
        ("content", 11, base[11][:-32]), ("content", 11, base[11] + "00"),
        ("content", 11, base[11][:100] + "q" + base[11][101:]),
    ]


def test_stream_refusals_name_the_field_and_the_odt_stream(exe, base):
    bad = bad_streams(base)
    lines = []
    for _, k, v in bad:
        f = list(base)
        f[k] = v
        lines.append(D.ctx_line(f))
    for (name, k, v), row in zip(bad, D.run(exe, lines)):
        assert len(row) == 2 and int(row[0]) == D.E_DOMAIN, (name, v[:12], row)
        assert name in row[1] and "$odt$" in row[1], (name, row[1])
    # the mixed pairs stay refused, with the messages they had; a wrong field count is no odf stream
    for k, v, name in ((1, "0", "checksum type"), (2, "0", "cipher"), (1, "2", "cipher")):
        f = list(base)
        f[k] = v
        row = D.run(exe, [D.ctx_line(f)])[0]
        assert int(row[0]) == D.E_DOMAIN and name in row[1], row
    for f in (base[:11], base + ["00"]):
        assert int(D.run(exe, [D.ctx_line(f)])[0][0]) == D.E_INVALID


def test_the_blowfish_stream_respelled_stays_refused(exe):
    """The yardstick of tests/test_odf_legacy_gpu.py bad_streams: a Blowfish stream with fields 1 and 2 set to "1" """
    f = list(D.case("odf")[0])
    f[1] = f[2] = "1"
    row = D.run(exe, [D.ctx_line(f)])[0]
    assert int(row[0]) == D.E_DOMAIN and "$odt$" in row[1] and "key size" in row[1]


def test_candidates_of_any_length(exe, base):
    rows = D.run(exe, [D.ctx_line(base)] + [D.cand_line(c) for c in (b"y" * 64, b"y" * 65, b"y" * 200, b"", b"a\0b",
                                                                   b"y" * (D.MAX_PW + 1))])
    assert rows[0][1] == FAMILY
    assert [(int(r[0]), int(r[1])) for r in rows[1:5]] == [(0, 64), (0, 65), (0, 200), (0, 0)]
    assert int(rows[5][0]) == D.E_INVALID and "NUL" in rows[5][2]
    assert int(rows[6][0]) == D.E_PWLEN


def _policy(exe, fields):
    rows = D.run(exe, [D.ctx_line(fields), "policy", "plan\t0\t%d\t%d\t1\t0" % (HUGE, HUGE)])
    assert rows[0][0] == "0", rows[0]
    init, lo, hi, tail, gran = (int(x) for x in rows[1])
    assert int(rows[2][0]) == init                                           # the first chunk is the policy's
    return init, lo, hi, tail, gran


def test_first_chunk_by_count(exe, base):
    """The row describes 1024 iterations; a context scales the first launch, the floor and the tail by 1024 / c, rounded
    up to the granularity, inside [one resident generation, the key buffer]."""
    odt_row = _policy(exe, D.case("odt")[0])
    assert odt_row == (1 << 22, 1 << 19, 1 << 23, 1 << 19, 512)
    got = {}
    for c in (1, 2, 1024, 1025, 1639, 100000, MAX_ITER):
        f = list(base)
        f[3] = str(c)
        got[c] = _policy(exe, f)
        init, lo, hi, tail, gran = got[c]
        assert (hi, gran) == (1 << 23, 512)
        for v, v1024 in ((init, 1 << 22), (lo, 1 << 19), (tail, 1 << 19)):
            scaled = -(-(-(-v1024 * 1024 // c)) // gran) * gran            # ceil, then up to whole granules
            assert v == min(hi, max(scaled, GENERATION)), (c, v, scaled)
            assert v % gran == 0 and GENERATION <= v <= hi
    assert got[1024] == odt_row                                              # ... and equals ODF 1.2's row there
    firsts = [got[c][0] for c in (1, 1024, 100000, MAX_ITER)]
    assert firsts == [1 << 23, 1 << 22, GENERATION, GENERATION]              # falls, never below a generation
    assert firsts == sorted(firsts, reverse=True)
    # 2^32 / 1025 = 4,190,213.9 -> 8,185 granules; 2^29 / 1639 = 327,560.6 is the first floor below a generation
    assert got[1025][0] == 8185 * 512 and got[1639][1] == GENERATION


def test_planned_chunks_stay_inside_the_key_buffer(exe, base):
    """Past 1638 iterations the floor is no power of two; doubling from it must stop at hi, which sizes the key buffer"""
    for c in (1, 1024, 2000, 100000):
        f = list(base)
        f[3] = str(c)
        lines = [D.ctx_line(f), "policy"] + ["plan\t%r\t%d\t%d\t1\t0" % (rate, HUGE, HUGE)
                                             for rate in (0.001, 1.0, 500.0, 2e4, 2.5e4, 3e4, 1e9)]
        rows = D.run(exe, lines)
        init, lo, hi, tail, gran = (int(x) for x in rows[1])
        for r in rows[2:]:
            assert lo <= int(r[0]) <= hi, (c, r)
        assert int(rows[-1][0]) == hi
        # eight devices, little left: never under the tail, in whole granules
        n = int(D.run(exe, [D.ctx_line(f), "plan\t0\t%d\t%d\t8\t0" % (3 * tail, HUGE)])[1][0])
        assert n == tail


# ---------------------------------------------------------------- (d) ABI, counts, build
def test_plan_chunk_knows_the_family_and_answers_for_1024():
    from dprf_amd import _lib
    assert _lib.plan_chunk(FAMILY, 0, 1, 1, 1, 0) == 1                       # the support probe of include/dprf.h
    assert _lib.plan_chunk(FAMILY, 0.0, HUGE, HUGE, 1) == _lib.plan_chunk("odf_aes256", 0.0, HUGE, HUGE, 1) == 1 << 22
    for rate in (0.05, 1.0, 100.0, 1e4, 1e8):
        assert _lib.plan_chunk(FAMILY, rate, HUGE, HUGE, 1) == _lib.plan_chunk("odf_aes256", rate, HUGE, HUGE, 1)
    assert _lib.plan_chunk("odf_bf_sha1", 0.0, HUGE, HUGE, 1) == 1 << 22      # the Blowfish family's plan is as it was
    assert _lib.lib().dprf_abi_version() == 9


def test_family_name_is_written_once():
    text = dict((f, open(os.path.join(CSRC, f)).read()) for f in sorted(os.listdir(CSRC)) if f.endswith((".cpp", ".h")))
    where = [(f, src.count('"%s"' % FAMILY)) for f, src in text.items() if '"%s"' % FAMILY in src]
    assert where == [("dprf_doc.cpp", 1)]


def test_header_documents_the_stream():
    text = open(os.path.join(REPO, "include", "dprf.h")).read()
    assert '"%s"' % FAMILY in text and "$odf$*1*1*<iterations>*32*" in text
    assert re.search(r"#define DPRF_ABI_VERSION 9\b", text)
    for out_of_scope in ("Argon2id", "AES-256-GCM", "shorter\n * than 1024 bytes"):
        assert out_of_scope in text, out_of_scope


def test_work_counts_by_iteration_count():
    from dprf_amd import work
    assert work.odf_aes_counts(1024) == (work.COUNTS["odt"], work.MAIN["odt"])
    for c in (1, 3, 100000):
        for blocks in (1, 2):
            counts, main = work.odf_aes_counts(c, blocks)
            assert counts["sha256c"] == blocks + 17 and main["sha256c"] == blocks
            assert counts["sha1c"] + counts["sha1c_hmac20"] == 2 + 4 * c and counts["sha1c_hmac20"] == 4 * c - 2
            assert main["sha1c"] + main["sha1c_hmac20"] == 2 + 4 * c
            assert counts["aes256_dec_block"] == 64 and "aes256_dec_block" not in main
    with pytest.raises(ValueError):
        work.odf_aes_counts(0)


def test_resource_gate_and_the_built_object():
    sys.path.insert(0, CSRC)
    try:
        import resource_gate
    finally:
        sys.path.remove(CSRC)
    assert resource_gate.SCRATCH_LIMIT.get("k_odf_aes_kdf") == 0
    gate = os.path.join(REPO, "build", "obj", "dprf_kernels_odfaes.o.gate")
    assert os.path.exists(gate), "no gate report of the odf_aes_sha256 object: run build() first"
    rows = [ln.split() for ln in open(gate).read().splitlines() if ln.strip()]
    assert len(rows) == 3                                                    # range, list and long-list sources
    for r in rows:
        assert r[0] == "ok" and "k_odf_aes_kdf" in r[2], r
        assert r[r.index("scratch") + 1] == "0", r
        assert int(r[r.index("VGPRs") + 1]) <= 96 and r[-1] == "5", r         # k_odt_kdf's budget: 5 waves per SIMD
