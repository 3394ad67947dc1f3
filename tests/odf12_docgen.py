"""ODF 1.2 packages (AES-256-CBC, SHA-256/1K) with a chosen PBKDF2 iteration count, their streams, and the Python
statement of the ``$odf$*1*1*`` check (include/dprf.h "ODF 1.2 at the manifest's iteration count").

tests/docgen.py writes such packages at the count the reference verifier hard-codes, 1024; here the count is an
argument, content.xml deflates to well over the 1024 bytes the checksum covers, and the manifest can be spelled both
ways (the URNs LibreOffice writes, the short names of the ODF 1.2 text) or wrongly, attribute by attribute.  The AES
block function and the manifest frame are tests/docgen.py's (libcrypto through the oracle's bindings).

  key(pw, salt, c)             PBKDF2-HMAC-SHA1(SHA256(pw), salt, c, 32), by hashlib
  make_entry(...)              one encrypted package entry: ciphertext, checksum, iv, salt
  odf_stream / odt_stream      the "$odf$*1*1*<c>*..." line of an entry, and (c = 1024 only) its "$odt$" line
  make_stream(pw, c, seed)     the $odf$*1*1* line of a generated entry, without a package
  verifies(stream, pw)         the model: what the device must answer
  write_odt12(path, ...)       a package, for odt2hashes
"""
import base64
import hashlib
import random
import zipfile
import zlib

from docgen import MANIFEST_NS, O, _aes_cbc, _rand

URN = MANIFEST_NS + "#"
SPELLINGS = {
    "urn": {"checksum_type": URN + "sha256-1k", "algorithm": "http://www.w3.org/2001/04/xmlenc#aes256-cbc",
            "skg_name": "http://www.w3.org/2000/09/xmldsig#sha256", "kd_name": "PBKDF2"},
    "short": {"checksum_type": "SHA256/1K", "algorithm": URN + "aes256-cbc", "skg_name": "SHA256",
              "kd_name": URN + "pbkdf2"},
}
COVERED = 1024          # the bytes the SHA256/1K checksum covers, and the content bytes the stream carries


def _bytes(pw):
    return pw.encode("utf-8") if isinstance(pw, str) else bytes(pw)


def key(pw, salt, iterations):
    return hashlib.pbkdf2_hmac("sha1", hashlib.sha256(_bytes(pw)).digest(), salt, iterations, 32)


def _aes_cbc_decrypt(k, iv, data):
    out, prev = [], iv
    for i in range(0, len(data), 16):
        ct = data[i:i + 16]
        out.append(bytes(a ^ b for a, b in zip(O.aes_decrypt_block(k, ct), prev)))
        prev = ct
    return b"".join(out)


def content_xml(rng, nwords=900):
    """A content.xml of hex words, which deflate to about half their size: well over COVERED bytes from 400 words on"""
    words = ["%06x" % rng.getrandbits(24) for _ in range(nwords)]
    return ('<?xml version="1.0" encoding="UTF-8"?><office:document-content><office:body><office:text><text:p>%s'
            '</text:p></office:text></office:body></office:document-content>' % " ".join(words)).encode()


def make_entry(rng, pw, data, iterations, whole=True):
    """data deflated, padded and encrypted under pw at `iterations`: {"enc", "checksum", "iv", "salt"}.
    whole=False encrypts only the COVERED bytes a stream carries (CBC: the same first bytes, a fraction of the time)."""
    salt, iv = _rand(rng, 16), _rand(rng, 16)
    comp = zlib.compressobj(9, zlib.DEFLATED, -15)
    deflated = comp.compress(data) + comp.flush()
    checksum = hashlib.sha256(deflated[:COVERED]).digest()
    pad = 16 - len(deflated) % 16                      # W3C xmlenc padding: random bytes, then the count
    plain = deflated + bytes(rng.getrandbits(8) for _ in range(pad - 1)) + bytes([pad])
    if not whole:
        assert len(deflated) >= COVERED
        plain = plain[:COVERED]
    return {"enc": _aes_cbc(key(pw, salt, iterations), iv, plain), "checksum": checksum, "iv": iv, "salt": salt,
            "deflated": len(deflated)}


def odf_stream(e, iterations, name=None):
    assert len(e["enc"]) >= COVERED
    s = "$odf$*1*1*%d*32*%s*16*%s*16*%s*0*%s" % (iterations, e["checksum"].hex(), e["iv"].hex(), e["salt"].hex(),
                                                e["enc"][:COVERED].hex())
    return s if name is None else name + ":" + s


def odt_stream(e, name="doc.odt"):
    """The reference's line for the same entry: it means 1024 iterations and has no field to say so"""
    return "%s:$odt$*1.2*%s*%s*%s*%s*%d" % (name, e["checksum"].hex(), e["iv"].hex(), e["salt"].hex(), e["enc"].hex(),
                                           len(e["enc"]))


def make_stream(pw, iterations, seed):
    rng = random.Random(seed)
    return odf_stream(make_entry(rng, pw, content_xml(rng, 500), iterations, whole=False), iterations)


def fields_of(stream):
    """The 12 fields dprf_ctx_create takes, split here and not by the code under test"""
    f = stream.split(":", 1)[-1].split("*") if "$odf$" in stream.split("*", 1)[0] else None
    assert f and f[0] == "$odf$" and len(f) == 12, stream[:40]
    return ["odf"] + f[1:]


def verifies(stream, pw):
    """The definition: SHA256(AES-256-CBC-decrypt(PBKDF2(SHA256(pw), salt, c, 32), iv, content[0:1024])) == checksum"""
    f = stream if isinstance(stream, (list, tuple)) else fields_of(stream)
    assert f[1] == "1" and f[2] == "1" and f[4] == "32" and f[6] == "16" and f[8] == "16" and f[10] == "0"
    checksum, iv, salt, content = (bytes.fromhex(f[k]) for k in (5, 7, 9, 11))
    assert (len(checksum), len(iv), len(salt), len(content)) == (32, 16, 16, COVERED)
    return hashlib.sha256(_aes_cbc_decrypt(key(pw, salt, int(f[3])), iv, content)).digest() == checksum


def _encryption_data(e, iterations, spelling, over):
    a = dict(SPELLINGS[spelling], skg_size="32", kd_size="32", count=iterations)
    a.update(over)
    b64 = lambda b: base64.b64encode(b).decode()
    attr = lambda name, v: "" if v is None else ' manifest:%s="%s"' % (name, v)
    return ('<manifest:encryption-data%s manifest:checksum="%s"><manifest:algorithm%s manifest:initialisation-vector='
            '"%s"/><manifest:start-key-generation%s%s/><manifest:key-derivation%s%s%s manifest:salt="%s"/>'
            '</manifest:encryption-data>'
            % (attr("checksum-type", a["checksum_type"]), b64(a.get("checksum", e["checksum"])),
               attr("algorithm-name", a["algorithm"]), b64(a.get("iv", e["iv"])),
               attr("start-key-generation-name", a["skg_name"]), attr("key-size", a["skg_size"]),
               attr("key-derivation-name", a["kd_name"]), attr("key-size", a["kd_size"]),
               attr("iteration-count", a["count"]), b64(a.get("salt", e["salt"]))))


def write_odt12(path, pw, seed, iterations=100000, spelling="urn", content_words=900, styles_words=700, **over):
    """A package of content.xml, styles.xml and an empty entry, every entry encrypted under pw at `iterations`.
    over: attributes of every entry's encryption-data to replace (None leaves one out) -- checksum_type, algorithm,
    skg_name, skg_size, kd_name, kd_size, count (the iteration-count attribute's text, whatever the key was derived
    with), and
    checksum / iv / salt bytes.  Returns {full-path: entry}."""
    rng = random.Random(seed)
    files = [("content.xml", content_xml(rng, content_words)),
             ("styles.xml", ('<?xml version="1.0" encoding="UTF-8"?><office:document-styles>%s</office:document-styles>'
                             % " ".join("%06x" % rng.getrandbits(24) for _ in range(styles_words))).encode()),
             ("Configurations2/accelerator/current.xml", b"")]
    entries = {}
    manifest = ['<?xml version="1.0" encoding="UTF-8"?>',
                '<manifest:manifest xmlns:manifest="%s" manifest:version="1.2">' % MANIFEST_NS,
                ' <manifest:file-entry manifest:full-path="/" manifest:version="1.2" '
                'manifest:media-type="application/vnd.oasis.opendocument.text"/>']
    for name, data in files:
        while True:
            e = make_entry(rng, pw, data, iterations)
            if e["enc"][0]:                              # as tests/docgen.py: no leading 00 byte in the $odt$ line
                break
        entries[name] = e
        manifest.append(' <manifest:file-entry manifest:full-path="%s" manifest:media-type="text/xml" '
                        'manifest:size="%d">%s</manifest:file-entry>'
                        % (name, len(data), _encryption_data(e, iterations, spelling, over)))
    manifest.append('</manifest:manifest>')
    with zipfile.ZipFile(path, "w") as z:
        z.writestr(zipfile.ZipInfo("mimetype"), "application/vnd.oasis.opendocument.text", zipfile.ZIP_STORED)
        for name, _ in files:
            z.writestr(zipfile.ZipInfo(name), entries[name]["enc"], zipfile.ZIP_STORED)
        z.writestr(zipfile.ZipInfo("META-INF/manifest.xml"), "\n".join(manifest), zipfile.ZIP_DEFLATED)
    return entries

