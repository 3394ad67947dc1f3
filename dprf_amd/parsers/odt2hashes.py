"""ODF verification-data extractor: Python-3 counterpart of
/root/reference/src/odt-impl/odt2hashes.py (get_hashes :53-86, template :43).

ODF 1.2 (AES-256-CBC; ``manifest:algorithm-name`` absent or naming AES-256-CBC):
``<basename>:$odt$*<version>*<checksum hex>*<iv hex>*<salt hex>*<encrypted hex>*<len>``.
The encryption data of the SMALLEST file-entry whose manifest size exceeds 1024 (or -1 with
``-e``/experimental) is used, ties resolved in manifest order (:66-72).

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


def _algorithm(fe):
    """manifest:algorithm-name of an encrypted file-entry (None: the attribute or the element is missing)"""
    enc = fe.find(NS + "encryption-data")
    alg = enc.find(NS + "algorithm") if enc is not None else None
    return alg.get(NS + "algorithm-name") if alg is not None else None


def _blowfish_hashes(filename, z, entries):
    """the $odf$ stream of an ODF 1.0 / 1.1 package; entries: its encrypted file-entries in manifest order"""
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
        raise ValueError("%s: no Blowfish-encrypted entry with at least %d stored bytes (the SHA1/1K checksum of a "
                         "shorter entry is not supported)" % (filename, BF_CONTENT))
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
