"""ODF verification-data extractor: Python-3 counterpart of
/root/reference/src/odt-impl/odt2hashes.py (get_hashes :53-86, template :43).

ODF 1.2 (AES-256-CBC; ``manifest:algorithm-name`` absent or naming AES-256-CBC):
``<basename>:$odt$*<version>*<checksum hex>*<iv hex>*<salt hex>*<encrypted hex>*<len>``.
The encryption data of the SMALLEST file-entry whose manifest size exceeds 1024 (or -1 with
``-e``/experimental) is used, ties resolved in manifest order (:66-72).

ODF 1.2 with a PBKDF2 ``manifest:iteration-count`` other than 1024 (LibreOffice writes 100000 today; 3.5 to 5.x wrote
1024, which the line above means and has no field for): the AES spelling of John's odf2john / hashcat 18400 stream,
``<basename>:$odf$*1*1*<iterations>*32*<checksum hex>*16*<iv hex>*16*<salt hex>*0*<first 1024 encrypted bytes, hex>``
(include/dprf.h "ODF 1.2 at the manifest's iteration count").  The entry is chosen as for Blowfish below; ``-e`` changes
nothing.  The manifest must say SHA256/1K, a 32-byte SHA-256 start key and PBKDF2, in either spelling: anything else
(Argon2id, AES-GCM) is a ValueError naming it.  A count of 1024, or none, prints the ``$odt$`` line as ever.

ODF 1.0 / 1.1 (``manifest:algorithm-name`` "Blowfish CFB" or its URN spelling; OpenOffice.org, StarOffice, Apache
OpenOffice, LibreOffice before 3.5 or with its "ODF 1.0/1.1" setting): the stream of John's odf2john / hashcat 18600,
``<basename>:$odf$*0*0*<iterations>*16*<checksum hex>*8*<iv hex>*16*<salt hex>*0*<first 1024 encrypted bytes, hex>``
(include/dprf.h "ODF 1.0/1.1").  The entry is content.xml if its stored data is at least 1024 bytes, otherwise the
smallest entry (by manifest size, ties in manifest order) with at least 1024 stored bytes; ``-e`` changes nothing here.
Any other algorithm is a ValueError naming it.
"""
import argparse
import base64
import os
import sys
import xml.etree.ElementTree as et
import zipfile

NS = "{urn:oasis:names:tc:opendocument:xmlns:manifest:1.0}"
TEMPLATE = "{0}:$odt$*{1}*{2}*{3}*{4}*{5}*{6}"
TEMPLATE_BF = "{0}:$odf$*0*0*{1}*16*{2}*8*{3}*16*{4}*0*{5}"
AES_NAMES = (None, "http://www.w3.org/2001/04/xmlenc#aes256-cbc", "urn:oasis:names:tc:opendocument:xmlns:manifest:1.0#aes256-cbc")
BLOWFISH_NAMES = ("Blowfish CFB", "urn:oasis:names:tc:opendocument:xmlns:manifest:1.0#blowfish")
BF_CONTENT = 1024      # the bytes the SHA1/1K checksum covers
TEMPLATE_AES = "{0}:$odf$*1*1*{1}*32*{2}*16*{3}*16*{4}*0*{5}"
URN = "urn:oasis:names:tc:opendocument:xmlns:manifest:1.0#"
SHA256_1K_NAMES = ("SHA256/1K", URN + "sha256-1k")
SHA256_NAMES = ("SHA256", "http://www.w3.org/2000/09/xmldsig#sha256", "http://www.w3.org/2001/04/xmlenc#sha256")
PBKDF2_NAMES = ("PBKDF2", URN + "pbkdf2")
ODT_ITERATIONS = 1024  # the count the $odt$ line means (the reference verifier's constant)


def _algorithm(fe):
    """manifest:algorithm-name of an encrypted file-entry (None: the attribute or the element is missing)"""
    enc = fe.find(NS + "encryption-data")
    alg = enc.find(NS + "algorithm") if enc is not None else None
    return alg.get(NS + "algorithm-name") if alg is not None else None


def _iterations(fe):
    """manifest:iteration-count of an encrypted file-entry's key derivation; None: the attribute is missing"""
    kd = fe.find(NS + "encryption-data").find(NS + "key-derivation")
    n = kd.get(NS + "iteration-count") if kd is not None else None
    return None if n is None else int(n)


def _content_entry(filename, z, entries, what):
    """content.xml if it has at least 1024 stored bytes, else the smallest such entry (ties in manifest order)"""
    stored = {}
    for fe in entries:
        try:
            stored[id(fe)] = z.getinfo(fe.get(NS + "full-path")).file_size
        except KeyError:
            stored[id(fe)] = -1
    fit = [fe for fe in entries if stored[id(fe)] >= BF_CONTENT]
    best = next((fe for fe in fit if fe.get(NS + "full-path") == "content.xml"), None)
    if best is None and fit:
        best = min(fit, key=lambda fe: int(fe.get(NS + "size") or stored[id(fe)]))   # min keeps the first of a tie
    if best is None:
        raise ValueError("%s: no %s-encrypted entry with at least %d stored bytes (the %s/1K checksum of a "
                         "shorter entry is not supported)" % (filename, what, BF_CONTENT,
                                                              "SHA1" if what == "Blowfish" else "SHA256"))
    return best


def _blowfish_hashes(filename, z, entries):
    """the $odf$ stream of an ODF 1.0 / 1.1 package; entries: its encrypted file-entries in manifest order"""
    best = _content_entry(filename, z, entries, "Blowfish")
    enc = best.find(NS + "encryption-data")
    kd = enc.find(NS + "key-derivation")
    checksum = base64.b64decode(enc.get(NS + "checksum"))
    iv = base64.b64decode(enc.find(NS + "algorithm").get(NS + "initialisation-vector"))
    salt = base64.b64decode(kd.get(NS + "salt"))
    ctype = enc.get(NS + "checksum-type")
    if ctype not in (None, "SHA1/1K", "urn:oasis:names:tc:opendocument:xmlns:manifest:1.0#sha1-1k"):
        raise ValueError("%s: checksum type %r with Blowfish CFB is not supported" % (filename, ctype))
    if len(checksum) != 20 or len(iv) != 8 or len(salt) != 16:
        raise ValueError("%s: Blowfish CFB entry with a %d-byte checksum, %d-byte iv, %d-byte salt (20, 8, 16 expected)"
                         % (filename, len(checksum), len(iv), len(salt)))
    data = z.read(best.get(NS + "full-path"))[:BF_CONTENT]
    return TEMPLATE_BF.format(os.path.basename(filename), int(kd.get(NS + "iteration-count")), checksum.hex(), iv.hex(),
                              salt.hex(), data.hex())


def _aes_hashes(filename, z, entries):
    """the $odf$*1*1* stream of an ODF 1.2 package whose PBKDF2 count is not the $odt$ line's 1024"""
    best = _content_entry(filename, z, entries, "AES-256-CBC")
    enc = best.find(NS + "encryption-data")
    kd = enc.find(NS + "key-derivation")
    skg = enc.find(NS + "start-key-generation")
    ctype = enc.get(NS + "checksum-type")
    if ctype not in SHA256_1K_NAMES:
        raise ValueError("%s: checksum type %r with AES-256-CBC is not supported (SHA256/1K is)" % (filename, ctype))
    sk_name = skg.get(NS + "start-key-generation-name") if skg is not None else None
    sk_size = skg.get(NS + "key-size") if skg is not None else None
    if sk_name not in SHA256_NAMES or sk_size not in (None, "32"):
        raise ValueError("%s: start key generation %r with key size %r is not supported (SHA256, 32 bytes)"
                         % (filename, sk_name, sk_size))
    kd_name = kd.get(NS + "key-derivation-name") if kd is not None else None
    if kd_name not in PBKDF2_NAMES:
        raise ValueError("%s: key derivation %r is not supported (PBKDF2 is)" % (filename, kd_name))
    if kd.get(NS + "key-size") not in (None, "32"):
        raise ValueError("%s: derived key size %r is not supported (32 bytes)" % (filename, kd.get(NS + "key-size")))
    iterations = _iterations(best)
    if iterations is None or iterations < 1:
        raise ValueError("%s: PBKDF2 iteration count %r" % (filename, iterations))
    checksum = base64.b64decode(enc.get(NS + "checksum"))
    iv = base64.b64decode(enc.find(NS + "algorithm").get(NS + "initialisation-vector"))
    salt = base64.b64decode(kd.get(NS + "salt"))
    if len(checksum) != 32 or len(iv) != 16 or len(salt) != 16:
        raise ValueError("%s: AES-256-CBC entry with a %d-byte checksum, %d-byte iv, %d-byte salt (32, 16, 16 expected)"
                         % (filename, len(checksum), len(iv), len(salt)))
    data = z.read(best.get(NS + "full-path"))[:BF_CONTENT]
    return TEMPLATE_AES.format(os.path.basename(filename), iterations, checksum.hex(), iv.hex(), salt.hex(), data.hex())


def get_hashes(filename, experimental=False):
    with zipfile.ZipFile(filename, "r") as z:
        root = et.fromstring(z.read("META-INF/manifest.xml"))
        version = root.get(NS + "version")
        encrypted = [fe for fe in root.iter(NS + "file-entry") if fe.find(NS + "encryption-data") is not None]
        names = {_algorithm(fe) for fe in encrypted}
        if names & set(BLOWFISH_NAMES):
            if names - set(BLOWFISH_NAMES):
                raise ValueError("%s: entries encrypted with different algorithms: %s"
                                 % (filename, ", ".join(sorted(map(str, names)))))
            return _blowfish_hashes(filename, z, encrypted)
        for name in names:
            if name not in AES_NAMES:
                raise ValueError("%s: encryption algorithm %r is not supported (AES-256-CBC of ODF 1.2 and Blowfish CFB "
                                 "of ODF 1.0 / 1.1 are)" % (filename, name))
        for fe in encrypted:
            kd = fe.find(NS + "encryption-data").find(NS + "key-derivation")
            kd_name = kd.get(NS + "key-derivation-name") if kd is not None else None
            if kd_name is not None and kd_name not in PBKDF2_NAMES:   # Argon2id: no $odt$ line means it either
                raise ValueError("%s: key derivation %r is not supported (PBKDF2 is)" % (filename, kd_name))
        if any(_iterations(fe) not in (None, ODT_ITERATIONS) for fe in encrypted):
            return _aes_hashes(filename, z, encrypted)
        size_limit = -1 if experimental else 1024
        best, best_size = None, None
        for fe in root.iter(NS + "file-entry"):
            size = fe.get(NS + "size")
            if size is not None and int(size) > size_limit and (best is None or int(size) < best_size):
                best, best_size = fe, int(size)
        if best is None:
            raise ValueError("%s: no encrypted file-entry above the size limit" % filename)
        enc = best.find(NS + "encryption-data")
        checksum = base64.b64decode(enc.get(NS + "checksum"))
        iv = base64.b64decode(enc.find(NS + "algorithm").get(NS + "initialisation-vector"))
        salt = base64.b64decode(enc.find(NS + "key-derivation").get(NS + "salt"))
        data = z.read(best.get(NS + "full-path"))
    return TEMPLATE.format(os.path.basename(filename), version, checksum.hex(), iv.hex(), salt.hex(),
                           data.hex(), len(data))


def main(argv=None):
    p = argparse.ArgumentParser(prog="odt2hashes")
    p.add_argument("-v", "--verbose", default=False, action="store_true")
    p.add_argument("-e", "--experimental", default=False, action="store_true")
    p.add_argument("filename")
    a = p.parse_args(argv)
    sys.stdout.write(get_hashes(a.filename, a.experimental) + "\n")


if __name__ == "__main__":
    main()
