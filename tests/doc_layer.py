"""Shared by tests/test_doc_layer.py (CPU) and tests/test_doc_layer_gpu.py: one stream per kernel family, the stand-alone
document-layer program (tests/host/doc_check.cpp) built with g++, and the kernel-argument words of a stream computed
here from its fields -- big- / little-endian words as dprf_amd/csrc/dprf_params.h states them, hashlib for MD5."""
import contextlib
import functools
import hashlib
import io
import os
import subprocess
import zlib

from conftest import REPO, load_golden

E_INVALID, E_DOMAIN, E_PWLEN = -1, -2, -5
FLAG_NEVER_MATCHES, FLAG_REF_NONDETERMINISTIC = 1, 2
MAX_PW = 131071
PAD = bytes.fromhex("28BF4E5E4E758A4164004E56FFFA01082E2E00B6D0683E802F0CA9FE6453697A")
PW = "Ux7"          # the password of the generated streams

# One stream per kernel family: (label, where the stream comes from, the family it must give, its format).  The
# families are stated here, not read from the library.
FAMILIES = [
    ("office_2007", ("golden", "office_synth_ok"), "office_std", 1),
    ("agile_2010", ("agile", "2010", 128), "office_agile_sha1", 1),
    ("agile_2013", ("agile", "2013", 256), "office_agile_sha512", 1),
    ("oldoffice_0", ("oldoffice", 0), "office_rc4_md5", 1),
    ("oldoffice_1", ("oldoffice", 1), "office_rc4_md5", 1),
    ("oldoffice_3", ("oldoffice", 3), "office_rc4_sha1", 1),
    ("oldoffice_4", ("oldoffice", 4), "office_rc4_sha1", 1),
    ("odt", ("golden", "odt_synth_e_ab"), "odf_aes256", 2),
    ("odf", ("odf",), "odf_bf_sha1", 2),
    ("pdf_r2", ("golden", "pdf_synth_r2_key"), "pdf_r24", 3),
    ("pdf_r3_40", ("golden", "pdf_synth_r3_l40_cab"), "pdf_r24", 3),
    ("pdf_r3_128", ("golden", "pdf_synth_r3_l128_abc"), "pdf_r24", 3),
    ("pdf_r4_meta0", ("golden", "pdf_synth_r4_meta0_dog"), "pdf_r24", 3),
    ("pdf_r5", ("golden", "pdf_synth_r5_cat"), "pdf_r5", 3),
    ("pdf_r6", ("golden", "pdf_synth_r6_ox"), "pdf_r6", 3),
]
LABELS = [c[0] for c in FAMILIES]
# every name dprf_ctx_kernel can return for a context that launches
ALL_NAMES = sorted(set(c[2] for c in FAMILIES)) + ["pdf_r24_owner", "pdf_r5_owner", "pdf_r6_owner"]
assert len(ALL_NAMES) == 13


def fields_of(stream):
    from dprf_amd.brute_force import parse_verification_data
    with contextlib.redirect_stdout(io.StringIO()):
        return list(parse_verification_data(stream))


@functools.lru_cache(maxsize=None)
def _case(label):
    src = dict((c[0], c[1]) for c in FAMILIES)[label]
    seed = zlib.crc32(label.encode())
    if src[0] == "golden":
        e = load_golden("streams.json")[src[1]]
        return e["stream"], e["password"]
    if src[0] == "agile":
        import agile_model
        return agile_model.make_stream(PW, src[1], src[2], 3, seed=seed), PW
    if src[0] == "oldoffice":
        import oldoffice_model
        return oldoffice_model.make_stream(PW, src[1], seed=seed), PW
    import odf_legacy_model
    return odf_legacy_model.make_stream(PW, 2, seed=seed), PW


def case(label):
    """(fields, password, family, format) of one entry of FAMILIES; the stream is made once."""
    stream, pw = _case(label)
    _, _, family, fmt = [c for c in FAMILIES if c[0] == label][0]
    return fields_of(stream), pw, family, fmt


# ---------------------------------------------------------------- the program
def build_doc_check(tmp_dir):
    """tests/host/doc_check.cpp and dprf_doc.cpp, with g++ and nothing else (no HIP, no sanitizer) -> the program.
    DPRF_DOC_CHECK names a program built by hand instead (the same two sources under a host sanitizer, on a CPU box)."""
    if os.environ.get("DPRF_DOC_CHECK"):
        return os.environ["DPRF_DOC_CHECK"]
    csrc = os.path.join(REPO, "dprf_amd", "csrc")
    exe = os.path.join(str(tmp_dir), "doc_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", csrc, os.path.join(REPO, "tests", "host", "doc_check.cpp"),
                    os.path.join(csrc, "dprf_doc.cpp"), "-o", exe], check=True)
    return exe


def ctx_line(fields):
    assert not any("\t" in f or "\n" in f for f in fields)
    return "\t".join(["ctx"] + list(fields))


def cand_line(pw):
    return "cand\t" + (pw.encode("utf-8") if isinstance(pw, str) else bytes(pw)).hex()


def run(exe, lines):
    """The program's answer to `lines`: one list of columns per line."""
    text = "".join(ln + "\n" for ln in lines)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    rows = [ln.split("\t") for ln in out.split("\n")[:-1]]
    assert len(rows) == len(lines), (len(rows), len(lines))
    return rows


def words(col):
    return [int(w, 16) for w in col.split()]


# ---------------------------------------------------------------- the expected words
def be(b):
    assert len(b) % 4 == 0
    return [int.from_bytes(b[i:i + 4], "big") for i in range(0, len(b), 4)]


def le(b):
    assert len(b) % 4 == 0
    return [int.from_bytes(b[i:i + 4], "little") for i in range(0, len(b), 4)]


def md5_padded(msg):
    """msg with MD5's padding: 0x80, zeros to 56 mod 64, the bit count as 8 little-endian bytes."""
    out = bytearray(msg) + b"\x80"
    out += bytes((56 - len(out)) % 64)
    return bytes(out + (8 * len(msg)).to_bytes(8, "little"))


def expected_flags(f):
    """DPRF_FLAG_REF_NONDETERMINISTIC: a hex field the reference's verifiers decode that starts with a 00 byte (the
    Agile, oldoffice and $odf$ streams have no reference verifier and are never flagged)."""
    hexed = {"office": (5, 6, 7), "odt": (2, 3, 4, 5), "pdf": (7, 9, 11)}.get(f[0], ())
    if f[0] == "office" and f[1] in ("2010", "2013"):
        hexed = ()
    return FLAG_REF_NONDETERMINISTIC if any(f[k].startswith("00") for k in hexed) else 0


def expected_words(f):
    """(the params struct of the stream's family as u32 words, the context's word vector) from the fields alone."""
    h = bytes.fromhex
    if f[0] == "office" and f[1] in ("2010", "2013"):        # dprf_agile_params
        return be(h(f[5])) + be(h(f[6])) + be(h(f[7])) + [int(f[2]), int(f[1] == "2013"), int(f[3]) // 32], []
    if f[0] == "office":                                       # dprf_office_params
        return be(h(f[5])) + be(h(f[6])) + be(h(f[7])) + [int(f[2])], []
    if f[0] == "oldoffice":                                    # dprf_oldoffice_params
        typ, salt = int(f[1]), h(f[2])
        rep = bytearray(336)
        for k in range(16):
            rep[21 * k + 5:21 * k + 21] = salt                 # zeros where the five hash bytes of each copy go
        rep = md5_padded(bytes(rep))
        assert len(rep) == 384
        return ([int(typ >= 3), 5 if typ == 3 else 16] + be(salt) + le(h(f[3])) + le(h(f[4]).ljust(20, b"\0")) +
                le(rep)), []
    if f[0] == "odt":                                          # dprf_odt_params, .enc null
        enc, enc_len = h(f[5]), int(f[6])
        hash_len = min(enc_len, 1024)
        vec = be(enc[:hash_len])
        return (be(h(f[2])) + be(h(f[3])) + be(h(f[4])) + [enc_len, hash_len, 0, 0],
                vec + [0] * (max(4, hash_len // 4) - len(vec)))
    if f[0] == "odf":                                          # dprf_odf_params, .x null
        return be(h(f[5])) + be(h(f[9])) + [int(f[3]), 0, 0], be(h(f[7])) + be(h(f[11]))
    assert f[0] == "pdf"                                       # dprf_pdf_params
    R, length, P, meta = int(f[2]), int(f[3]), int(f[4]) & 0xffffffff, int(f[5])
    ident, U, O = h(f[7]), h(f[9]), h(f[11])
    u, h2, tail, o, osuf = [0] * 12, [0] * 4, [0] * 64, [0] * 8, [0] * 14
    n = tail_blocks = 0
    if R >= 5:
        u[:10] = be(U[:32]) + le(U[32:40])
        if len(O) >= 48 and len(U) >= 48:
            o = be(O[:32])
            osuf = le(O[32:40]) + le(U[:48])
    else:
        n = length // 8
        nu = 32 if R == 2 else 16
        u[:nu // 4] = le(U[:nu])
        h2 = le(hashlib.md5(PAD + ident).digest())
        msg = md5_padded(PAD + O + P.to_bytes(4, "little") + ident + (b"\xff" * 4 if R >= 4 and not meta else b""))
        t = le(msg[32:])
        tail[:len(t)] = t
        tail_blocks = len(msg) // 64 - 1
        if len(O) >= 32:
            o = le(O[:32])
    return [R, n] + u + h2 + le(PAD) + [tail_blocks] + tail + [0] + o + osuf, []
