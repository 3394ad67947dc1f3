"""Writes password-protected ODF 1.0 / 1.1 packages as OpenOffice.org and Apache OpenOffice write them: no
manifest:version, every entry deflated (raw), then Blowfish-CFB encrypted, then STORED in the zip; the manifest
carries manifest:size (the plain size), checksum-type SHA1/1K with the SHA-1 of the first 1024 deflated bytes,
algorithm-name "Blowfish CFB" with an 8-byte iv, and key-derivation PBKDF2 with iteration-count 1024 and a 16-byte
salt (one salt and iv per entry).  The cipher comes from tests/odf_legacy_model.py."""
import base64
import os
import random
import sys
import zipfile
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import odf_legacy_model as model  # noqa: E402

MANIFEST_NS = "urn:oasis:names:tc:opendocument:xmlns:manifest:1.0"
BLOWFISH_URN = "urn:oasis:names:tc:opendocument:xmlns:manifest:1.0#blowfish"


def _deflate(data):
    comp = zlib.compressobj(9, zlib.DEFLATED, -15)
    return comp.compress(data) + comp.flush()


def _b64(b):
    return base64.b64encode(b).decode()


def _noise(rng, n):
    """n words that deflate poorly: about three bytes of deflated data each"""
    return " ".join("%06x" % rng.getrandbits(24) for _ in range(n))


def default_files(rng, content_words=900, styles_words=700):
    return [
        ("content.xml", ('<?xml version="1.0" encoding="UTF-8"?><office:document-content><office:body><office:text>'
                         '<text:p>%s</text:p></office:text></office:body></office:document-content>'
                         % _noise(rng, content_words)).encode()),
        ("styles.xml", ('<?xml version="1.0" encoding="UTF-8"?><office:document-styles>%s</office:document-styles>'
                        % _noise(rng, styles_words)).encode()),
        ("meta.xml", b'<?xml version="1.0" encoding="UTF-8"?><office:document-meta/>'),
    ]


def write_odf11(path, password, seed=0, files=None, iterations=1024, algorithm="Blowfish CFB",
                checksum_type="SHA1/1K"):
    """Write the package; returns {full-path: (salt, iv, checksum, encrypted bytes)}.  files: [(name, plain bytes)] in
    manifest order (default: a content.xml that deflates to more than 1024 bytes, a styles.xml, a short meta.xml)."""
    rng = random.Random(seed)
    if files is None:
        files = default_files(rng)
    out = {}
    manifest = ['<?xml version="1.0" encoding="UTF-8"?>',
                '<manifest:manifest xmlns:manifest="%s">' % MANIFEST_NS,
                ' <manifest:file-entry manifest:media-type="application/vnd.oasis.opendocument.text" '
                'manifest:full-path="/"/>']
    for name, data in files:
        salt = bytes(rng.getrandbits(8) for _ in range(16))
        iv = bytes(rng.getrandbits(8) for _ in range(8))
        checksum, enc = model.encrypt_entry(password, iterations, salt, iv, _deflate(data))
        out[name] = (salt, iv, checksum, enc)
        manifest.append(
            ' <manifest:file-entry manifest:media-type="text/xml" manifest:full-path="%s" manifest:size="%d">'
            '<manifest:encryption-data manifest:checksum-type="%s" manifest:checksum="%s">'
            '<manifest:algorithm manifest:algorithm-name="%s" manifest:initialisation-vector="%s"/>'
            '<manifest:key-derivation manifest:key-derivation-name="PBKDF2" manifest:iteration-count="%d" '
            'manifest:salt="%s"/></manifest:encryption-data></manifest:file-entry>'
            % (name, len(data), checksum_type, _b64(checksum), algorithm, _b64(iv), iterations, _b64(salt)))
    manifest.append('</manifest:manifest>')
    with zipfile.ZipFile(path, "w") as z:
        z.writestr(zipfile.ZipInfo("mimetype"), "application/vnd.oasis.opendocument.text", zipfile.ZIP_STORED)
        for name, _ in files:
            z.writestr(zipfile.ZipInfo(name), out[name][3], zipfile.ZIP_STORED)
        z.writestr(zipfile.ZipInfo("META-INF/manifest.xml"), "\n".join(manifest), zipfile.ZIP_DEFLATED)
    return out
