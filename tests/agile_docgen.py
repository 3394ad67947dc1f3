"""A self-generated Office 2010 / 2013 document with Agile Encryption (TEST INFRASTRUCTURE, beside docgen.py).

``write_docx_agile`` writes an MS-CFB compound file (docgen._cfb) whose ``EncryptionInfo`` stream is version 4.4,
flags 0x40, followed by the XML descriptor of MS-OFFCRYPTO 2.3.4.10: ``keyData`` and the password ``encryptedKey`` with
every attribute, ``encryptedKeyValue`` included.  The verifier fields are real: a random verifier encrypted under the
keys derived from the password (agile_model.make_parts), so the project's office2john.get_hash turns the file into the
stream agile_model.make_stream gives for the same inputs, and the password verifies.

The ``EncryptedPackage`` stream is PLACEHOLDER bytes and ``encryptedKeyValue`` / ``dataIntegrity`` are random: nothing
available to the tests can open such a document, so only what a password search reads is real.  The file is not meant
to be opened by Office.
"""
import base64
import random
import struct

import agile_model as M
import docgen

_HASH = {"2010": ("SHA1", 20), "2013": ("SHA512", 64)}


def encryption_info(pw, seed, version, key_bits, spin):
    version = str(version)
    alg, hsize = _HASH[version]
    salt, evi, evh = M.make_parts(pw, version, key_bits, spin, seed)
    rng = random.Random(seed ^ 0x5EED)
    rnd = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    b64 = lambda b: base64.b64encode(b).decode()
    common = ('saltSize="16" blockSize="16" keyBits="%d" hashSize="%d" cipherAlgorithm="AES" cipherChaining='
              '"ChainingModeCBC" hashAlgorithm="%s"' % (key_bits, hsize, alg))
    hmac_len = hsize + (-hsize % 16)
    xml = ('<?xml version="1.0" encoding="UTF-8" standalone="yes"?>\r\n'
           '<encryption xmlns="http://schemas.microsoft.com/office/2006/encryption" '
           'xmlns:p="http://schemas.microsoft.com/office/2006/keyEncryptor/password">'
           '<keyData %s saltValue="%s"/>'
           '<dataIntegrity encryptedHmacKey="%s" encryptedHmacValue="%s"/>'
           '<keyEncryptors><keyEncryptor uri="http://schemas.microsoft.com/office/2006/keyEncryptor/password">'
           '<p:encryptedKey spinCount="%d" %s saltValue="%s" encryptedVerifierHashInput="%s" '
           'encryptedVerifierHashValue="%s" encryptedKeyValue="%s"/>'
           '</keyEncryptor></keyEncryptors></encryption>'
           % (common, b64(rnd(16)), b64(rnd(hmac_len)), b64(rnd(hmac_len)), spin, common, b64(salt), b64(evi),
              b64(evh), b64(rnd(key_bits // 8))))
    return struct.pack("<HHI", 4, 4, 0x40) + xml.encode("utf-8")


def write_docx_agile(path, pw, seed, version="2013", key_bits=256, spin=100000):
    """Write the document; returns the stream agile_model.make_stream gives for the same inputs (basename aside).
    EncryptedPackage is placeholder bytes (module docstring): the file carries a real password verifier only."""
    info = encryption_info(pw, seed, version, key_bits, spin)
    rng = random.Random(seed ^ 0xC0FFEE)
    package = struct.pack("<Q", 4000) + bytes(rng.getrandbits(8) for _ in range(4096))
    with open(path, "wb") as f:
        f.write(docgen._cfb({"EncryptionInfo": info, "EncryptedPackage": package}))
    return M.make_stream(pw, version, key_bits, spin, seed)
