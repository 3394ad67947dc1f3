"""The 40-bit key search stated in Python (TEST INFRASTRUCTURE: the tests' statement of what dprf_search_key40 computes;
include/dprf.h "40-bit key search").

Hashes come from hashlib, RC4 from tests/oldoffice_model.  Fields are what parse_verification_data returns:
    ["pdf", V, R, Length, P, EncryptMetadata, idlen, ID, ulen, U, olen, O]
    ["oldoffice", type, salt, encryptedVerifier, encryptedVerifierHash]
A key is five bytes; its index is the bytes read big-endian.
"""
import hashlib
import random

from oldoffice_model import rc4

SPACE = 1 << 40
PAD = bytes.fromhex("28BF4E5E4E758A4164004E56FFFA01082E2E00B6D0683E802F0CA9FE6453697A")


def key_bytes(index):
    assert 0 <= index < SPACE
    return index.to_bytes(5, "big")


def key_index(key):
    key = bytes.fromhex(key) if isinstance(key, str) else bytes(key)
    assert len(key) == 5
    return int.from_bytes(key, "big")


def family(fields):
    """"pdf_r2", "pdf_r34", "office_md5", "office_sha1", or None for a document that is not a 40-bit one."""
    if fields[0] == "pdf":
        rev = int(fields[2])
        if rev == 2:
            return "pdf_r2"
        return "pdf_r34" if rev in (3, 4) and int(fields[3]) // 8 == 5 else None
    if fields[0] == "oldoffice":
        return {0: "office_md5", 1: "office_md5", 3: "office_sha1"}.get(int(fields[1]))
    return None


def pdf_r34_chain(key, ident):
    c = rc4(key, hashlib.md5(PAD + ident).digest())
    for x in range(1, 20):
        c = rc4(bytes(b ^ x for b in key), c)
    return c


def office_plain(fam, key, ev, evh):
    """The decrypted verifier || verifier hash under the five key bytes."""
    if fam == "office_md5":
        return rc4(hashlib.md5(key + b"\0\0\0\0").digest(), ev + evh)
    return rc4(key + b"\0" * 11, ev + evh)


def key_verifies(fields, key):
    key = bytes(key)
    assert len(key) == 5
    fam = family(fields)
    assert fam, "not a 40-bit document"
    if fam == "pdf_r2":
        return rc4(key, PAD) == bytes.fromhex(fields[9])[:32]
    if fam == "pdf_r34":
        return pdf_r34_chain(key, bytes.fromhex(fields[7])) == bytes.fromhex(fields[9])[:16]
    d = office_plain(fam, key, bytes.fromhex(fields[3]), bytes.fromhex(fields[4]))
    if fam == "office_md5":
        return hashlib.md5(d[:16]).digest() == d[16:32]
    return hashlib.sha1(d[:16]).digest() == d[16:36]


def key_of_password(fields, pw):
    """The five key bytes the password pw (a str) gives on this document."""
    fam = family(fields)
    assert fam, "not a 40-bit document"
    if fam.startswith("pdf"):
        # ISO 32000-1 Algorithm 2; R2 takes a 5-byte key whatever Length says
        rev, perm, meta = int(fields[2]), int(fields[4]) & 0xffffffff, int(fields[5])
        padded = (pw.encode("utf-8") + PAD)[:32]
        h = hashlib.md5(padded + bytes.fromhex(fields[11]) + perm.to_bytes(4, "little") + bytes.fromhex(fields[7]) +
                        (b"\xff" * 4 if rev >= 4 and not meta else b"")).digest()
        if rev >= 3:
            for _ in range(50):
                h = hashlib.md5(h[:5]).digest()
        return h[:5]
    pw16 = pw.encode("utf-16-le", "surrogatepass")
    salt = bytes.fromhex(fields[2])
    if fam == "office_md5":
        h = hashlib.md5(pw16).digest()
        return hashlib.md5((h[:5] + salt) * 16).digest()[:5]
    h = hashlib.sha1(salt + pw16).digest()
    return hashlib.sha1(h + b"\0\0\0\0").digest()[:5]


def plant(fields, key, seed=0):
    """The fields with U, or encryptedVerifier / encryptedVerifierHash, rewritten so that exactly `key` verifies (no
    password is involved: U = RC4(key, PAD) for R2).  Bytes of U the check does not read come from the seed."""
    key = bytes(key)
    assert len(key) == 5
    fam = family(fields)
    assert fam, "not a 40-bit document"
    rng = random.Random(seed)
    out = list(fields)
    if fam == "pdf_r2":
        out[9] = rc4(key, PAD).hex()
    elif fam == "pdf_r34":
        out[9] = (pdf_r34_chain(key, bytes.fromhex(fields[7])) + bytes(rng.getrandbits(8) for _ in range(16))).hex()
    else:
        v = bytes(rng.getrandbits(8) for _ in range(16))
        H = hashlib.md5 if fam == "office_md5" else hashlib.sha1
        c = office_plain(fam, key, v, H(v).digest())       # RC4 encrypts as it decrypts
        out[3], out[4] = c[:16].hex(), c[16:].hex()
    assert key_verifies(out, key)
    return out


def stream_of(fields):
    """The fields as a verifier stream parse_verification_data takes."""
    if fields[0] == "pdf":
        return "made.pdf:$pdf$*" + "*".join(fields[1:])
    return "made.doc:$oldoffice$" + "*".join(fields[1:])


# ---------------------------------------------------------------- the streams the tests share
def fields_of(stream):
    import contextlib
    import io
    from dprf_amd.brute_force import parse_verification_data
    with contextlib.redirect_stdout(io.StringIO()):
        return list(parse_verification_data(stream))


def known_password_cases():
    """[(label, fields, password)]: every golden or generated 40-bit stream whose password is known."""
    import oldoffice_model
    from conftest import load_golden
    out = []
    for name, e in sorted(load_golden("streams.json").items()):
        if name.startswith("pdf"):
            f = fields_of(e["stream"])
            if family(f):
                out.append((name, f, e["password"]))
    for name, e in sorted(load_golden("oldoffice_vectors.json").items()):
        f = fields_of(e["stream"])
        if family(f):
            out.append((name, f, e["password"]))
    for typ in (0, 1, 3):
        out.append(("oldoffice_made_%d" % typ, fields_of(oldoffice_model.make_stream("Ux7", typ, seed=40 + typ)), "Ux7"))
    return out


def base_documents():
    """{family: fields}: one document per 40-bit family, to plant keys in."""
    import oldoffice_model
    from conftest import load_golden
    g = load_golden("streams.json")
    return {
        "pdf_r2": fields_of(g["pdf_synth_r2_key"]["stream"]),
        "pdf_r34": fields_of(g["pdf_synth_r3_l40_cab"]["stream"]),
        "office_md5": fields_of(oldoffice_model.make_stream("Ux7", 1, seed=41)),
        "office_sha1": fields_of(oldoffice_model.make_stream("Ux7", 3, seed=43)),
    }
