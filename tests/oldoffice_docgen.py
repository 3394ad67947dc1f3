"""Self-generated Office 97-2003 binary documents with RC4 / RC4 CryptoAPI encryption (TEST INFRASTRUCTURE, beside
docgen.py, whose compound-file writer this uses).

These are PARSER FIXTURES, not documents Word or Excel would open: a .doc is a WordDocument stream holding a FIB base
(wIdent, the fEncrypted / fWhichTblStm / fObfuscated bits) and a table stream that starts with the encryption header;
an .xls is a Workbook stream of BOF, FILEPASS and EOF records.  What a password search reads is real: a random
verifier RC4-encrypted under the key derived from the password (oldoffice_model.make_parts), so the project's
office2john.get_hash prints the stream oldoffice_model.make_stream gives for the same inputs, and the password
verifies.  Nothing else of the document exists.
"""
import os
import struct

import docgen
import oldoffice_model as M

CSP = {3: "Microsoft Base Cryptographic Provider v1.0", 4: "Microsoft Strong Cryptographic Provider"}


def _cryptoapi(typ, salt, ev, evh):
    """MS-OFFCRYPTO 2.3.5.1 past the version: flags, header size, EncryptionHeader, EncryptionVerifier."""
    csp = (CSP[typ] + "\0").encode("utf-16-le")
    header = struct.pack("<IIIIIIII", 0x04, 0, 0x6801, 0x8004, 40 if typ == 3 else 128, 1, 0, 0) + csp
    return struct.pack("<II", 0x04, len(header)) + header + struct.pack("<I", 16) + salt + ev + struct.pack("<I", 20) + evh


def _header(typ, salt, ev, evh):
    """The encryption header from its version on: 1.1 for RC4, 2.2 for RC4 CryptoAPI."""
    if typ in (0, 1):
        return struct.pack("<HH", 1, 1) + salt + ev + evh
    return struct.pack("<HH", 2, 2) + _cryptoapi(typ, salt, ev, evh)


def _fib(flags11, which=1):
    """The first 32 bytes of a FIB: wIdent 0xA5EC, nFib 0x00C1, byte 11 = the encryption bits."""
    return struct.pack("<HH", 0xA5EC, 0x00C1) + b"\0" * 7 + bytes([flags11 | (0x02 if which else 0)]) + b"\0" * 20


def write_doc(path, pw, typ, seed, which=1):
    """A .doc with type 1 (RC4), 3 or 4 (CryptoAPI); which: the table stream fWhichTblStm names.  Returns the stream
    office2john prints for it."""
    assert typ in (1, 3, 4)
    salt, ev, evh = M.make_parts(pw, typ, seed)
    table = _header(typ, salt, ev, evh) + b"\0" * 64
    with open(path, "wb") as f:
        f.write(docgen._cfb({"WordDocument": _fib(0x01, which), "1Table" if which else "0Table": table}))
    return M.stream_of(typ, salt, ev, evh, name=os.path.basename(path))


def _rec(typ, data):
    return struct.pack("<HH", typ, len(data)) + data


def write_xls(path, pw, typ, seed):
    """An .xls with type 0 (RC4), 3 or 4 (CryptoAPI): BOF, FILEPASS, EOF.  Returns the stream office2john prints."""
    assert typ in (0, 3, 4)
    salt, ev, evh = M.make_parts(pw, typ, seed)
    bof = _rec(0x0809, struct.pack("<HHHHII", 0x0600, 0x0005, 0x0DBB, 0x07CC, 0, 6))
    filepass = _rec(0x2F, struct.pack("<H", 1) + _header(typ, salt, ev, evh))
    with open(path, "wb") as f:
        f.write(docgen._cfb({"Workbook": bof + filepass + _rec(0x0A, b"")}))
    return M.stream_of(typ, salt, ev, evh, name=os.path.basename(path))


def write_doc_plain(path, xor=False):
    """A .doc that is not encrypted, or XOR-obfuscated (fEncrypted and fObfuscated)."""
    with open(path, "wb") as f:
        f.write(docgen._cfb({"WordDocument": _fib(0x81 if xor else 0x00), "1Table": b"\0" * 64}))


def write_xls_xor(path):
    """An .xls whose FILEPASS says XOR obfuscation (wEncryptionType 0, key, verifier)."""
    bof = _rec(0x0809, struct.pack("<HHHHII", 0x0600, 0x0005, 0x0DBB, 0x07CC, 0, 6))
    with open(path, "wb") as f:
        f.write(docgen._cfb({"Workbook": bof + _rec(0x2F, struct.pack("<HHH", 0, 0x1234, 0x5678)) + _rec(0x0A, b"")}))


def write_ppt(path):
    with open(path, "wb") as f:
        f.write(docgen._cfb({"PowerPoint Document": b"\0" * 64, "Current User": b"\0" * 32}))
