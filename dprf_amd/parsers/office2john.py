"""MS Office (OOXML in an OLE container) verification-data extractor: Python-3 counterpart of the
encrypted-OOXML path of /root/reference/src/ms-offcrypto-impl/office2john.py (process_new_office
:1728-1821), which the reference engine calls for document type 1 (brute_force.py:236).

Output, Standard Encryption (Office 2007, the form the reference verifier handles):
    ``<basename>:$office$*2007*<verifierHashSize>*<keySize>*<saltSize>*<salt>*<encVerifier>*<encVerifierHash[0:32]>``
Agile Encryption (Office 2010/2013) is printed in the reference's form too
    ``<basename>:$office$*<2010|2013>*<spinCount>*<keyBits>*<saltSize>*<salt>*<encHashInput>*<encHashValue[0:32]>``
and libdprf.so verifies it on the device (kernel families "office_agile_sha1" / "office_agile_sha512",
include/dprf.h "Agile"): keyBits 128 or 256, saltSize 16, spinCount up to 10,000,000.

Password-protected binary documents of Office 97-2003 (no EncryptionInfo stream; the reference's process_file
:1949-1982, find_rc4_passinfo_xls :1472-1537, find_rc4_passinfo_doc :1576-1629) are printed in the reference's form
    ``<basename>:$oldoffice$<type>*<salt>*<encVerifier>*<encVerifierHash>``
type 0 / 1: RC4 (MS-OFFCRYPTO 2.3.6) in an .xls / .doc, 16-byte verifier hash; type 3 / 4: RC4 CryptoAPI (2.3.5) with
a 40-bit / 128-bit key, 20-byte verifier hash.  libdprf.so verifies them on the device (kernel families
"office_rc4_md5" / "office_rc4_sha1", include/dprf.h "Office 97-2003").  The reference's ``:::summary::filename`` tail
(John's GECOS fields, not verifier data) is left out.  XOR obfuscation and PowerPoint 97-2003 raise ValueError.  A
.doc's header is read from the table stream its FIB names (fWhichTblStm); the reference always opens 1Table.

The OLE compound file (MS-CFB) is read by a small reader of our own: header, DIFAT/FAT chains,
directory, mini stream.
"""
import base64
import os
import struct
import sys
import xml.etree.ElementTree as et

_SIG = bytes.fromhex("d0cf11e0a1b11ae1")
_END, _FREE = 0xFFFFFFFE, 0xFFFFFFFF


class CompoundFile:
    def __init__(self, data):
        if data[:8] != _SIG:
            raise ValueError("not an OLE compound file")
        self.d = data
        self.ss = 1 << struct.unpack_from("<H", data, 0x1E)[0]
        self.mss = 1 << struct.unpack_from("<H", data, 0x20)[0]
        nfat, self.dir_start = struct.unpack_from("<II", data, 0x2C)
        self.cutoff, mfat_start, nmfat, difat_start, ndifat = struct.unpack_from("<IIIII", data, 0x38)
        difat = list(struct.unpack_from("<109I", data, 0x4C))
        s = difat_start
        for _ in range(ndifat):
            if s in (_END, _FREE):
                break
            vals = struct.unpack_from("<%dI" % (self.ss // 4), self._sector(s))
            difat += vals[:-1]
            s = vals[-1]
        fat = []
        for sec in difat[:nfat]:
            fat += struct.unpack_from("<%dI" % (self.ss // 4), self._sector(sec))
        self.fat = fat
        self.entries = self._directory()
        root = self.entries[0]
        self.mini_stream = self._chain_bytes(root["start"], root["size"], self.fat, self._sector)
        mfat_bytes = self._chain_bytes(mfat_start, nmfat * self.ss, self.fat, self._sector) if nmfat else b""
        self.mfat = list(struct.unpack_from("<%dI" % (len(mfat_bytes) // 4), mfat_bytes))

    def _sector(self, n):
        off = (n + 1) * self.ss
        return self.d[off:off + self.ss]

    def _mini_sector(self, n):
        return self.mini_stream[n * self.mss:(n + 1) * self.mss]

    def _chain_bytes(self, start, size, table, reader):
        out, s, seen = [], start, set()
        while s not in (_END, _FREE) and s < len(table) and s not in seen and len(out) * 1 < 1 << 24:
            seen.add(s)
            out.append(reader(s))
            s = table[s]
        return b"".join(out)[:size]

    def _directory(self):
        raw = self._chain_bytes(self.dir_start, 1 << 30, self.fat, self._sector)
        ents = []
        for off in range(0, len(raw) - 127, 128):
            nlen = struct.unpack_from("<H", raw, off + 0x40)[0]
            name = raw[off:off + max(0, nlen - 2)].decode("utf-16-le", errors="replace")
            typ = raw[off + 0x42]
            start = struct.unpack_from("<I", raw, off + 0x74)[0]
            size = struct.unpack_from("<Q", raw, off + 0x78)[0]
            if self.ss == 512:
                size &= 0xFFFFFFFF
            ents.append({"name": name, "type": typ, "start": start, "size": size})
        return ents

    def open_stream(self, name):
        for e in self.entries[1:]:
            if e["type"] == 2 and e["name"].lower() == name.lower():
                if e["size"] < self.cutoff:
                    return self._chain_bytes(e["start"], e["size"], self.mfat, self._mini_sector)
                return self._chain_bytes(e["start"], e["size"], self.fat, self._sector)
        raise KeyError(name)

    def has_stream(self, name):
        return any(e["type"] == 2 and e["name"].lower() == name.lower() for e in self.entries[1:])


def _cryptoapi(filename, s, off):
    """RC4 CryptoAPI EncryptionHeader + EncryptionVerifier (MS-OFFCRYPTO 2.3.5.1) at s[off:], off just past the
    version: (keySize, CSP name lower-cased, salt, encryptedVerifier, encryptedVerifierHash)."""
    try:
        header_size = struct.unpack_from("<I", s, off + 4)[0]         # after the 4 flag bytes
        hdr = off + 8
        key_size = struct.unpack_from("<I", s, hdr + 16)[0]           # flags, sizeExtra, algID, algIDHash, keySize
        csp = s[hdr + 32:hdr + header_size].decode("utf-16-le", errors="replace").lower()
        v = hdr + header_size
        salt_size = struct.unpack_from("<I", s, v)[0]
        if salt_size != 16:
            raise ValueError("%s : salt size %d (expected 16)" % (filename, salt_size))
        vh_size = struct.unpack_from("<I", s, v + 36)[0]
        if vh_size != 20:
            raise ValueError("%s : verifier hash size %d (expected 20)" % (filename, vh_size))
        salt, ev, evh = s[v + 4:v + 20], s[v + 20:v + 36], s[v + 40:v + 60]
    except struct.error:
        raise ValueError("%s : truncated RC4 CryptoAPI header" % filename)
    if len(evh) != 20:
        raise ValueError("%s : truncated RC4 CryptoAPI verifier" % filename)
    return key_size, csp, salt, ev, evh


def _rc4_plain(filename, s, off):
    """RC4 encryption header (MS-OFFCRYPTO 2.3.6.1) past its version: salt, encryptedVerifier, encryptedVerifierHash."""
    if len(s) < off + 48:
        raise ValueError("%s : truncated RC4 encryption header" % filename)
    return s[off:off + 16], s[off + 16:off + 32], s[off + 32:off + 48]


def _old_xls(filename, wb):
    """FILEPASS (0x2F) of the Workbook stream's BIFF records -> (type, salt, ev, evh)."""
    pos = 0
    while pos + 4 <= len(wb):
        rec, length = struct.unpack_from("<HH", wb, pos)
        data = wb[pos + 4:pos + 4 + length]
        pos += 4 + length
        if rec != 0x2F:
            continue
        if data[0:2] == b"\x00\x00":
            raise ValueError("%s : XOR obfuscation is not supported" % filename)
        if data[0:6] == b"\x01\x00\x01\x00\x01\x00":
            return (0,) + _rc4_plain(filename, data, 6)
        if data[0:4] in (b"\x01\x00\x02\x00", b"\x01\x00\x03\x00"):
            key_size, _, salt, ev, evh = _cryptoapi(filename, data, 6)
            return (3 if key_size == 40 else 4, salt, ev, evh)
        raise ValueError("%s : unknown FILEPASS encryption header %s" % (filename, data[0:6].hex()))
    raise ValueError("%s : Document is not encrypted (no FILEPASS record)" % filename)


def _old_doc(filename, cf):
    """The FIB of WordDocument and the encryption header at the start of the table stream -> (type, salt, ev, evh)."""
    fib = cf.open_stream("WordDocument")
    if len(fib) < 12 or struct.unpack_from("<H", fib, 0)[0] != 0xA5EC:
        raise ValueError("%s : WordDocument does not start with a FIB (wIdent 0xA5EC)" % filename)
    flags = fib[11]                                   # bit 0 fEncrypted, bit 1 fWhichTblStm, bit 7 fObfuscated
    if not flags & 0x01:
        raise ValueError("%s : Document is not encrypted" % filename)
    if flags & 0x80:
        raise ValueError("%s : XOR obfuscation is not supported" % filename)
    table = cf.open_stream("1Table" if flags & 0x02 else "0Table")
    if len(table) < 4:
        raise ValueError("%s : truncated table stream" % filename)
    major, minor = struct.unpack_from("<HH", table, 0)
    if major == 1 or minor == 1:
        return (1,) + _rc4_plain(filename, table, 4)
    if major >= 2 and minor == 2:
        _, csp, salt, ev, evh = _cryptoapi(filename, table, 4)
        return (4 if "strong" in csp else 3, salt, ev, evh)
    raise ValueError("%s : unknown encryption header version %d.%d" % (filename, major, minor))


def _old_office(filename, cf):
    if cf.has_stream("WordDocument"):
        typ, salt, ev, evh = _old_doc(filename, cf)
    elif cf.has_stream("Workbook") or cf.has_stream("Book"):
        typ, salt, ev, evh = _old_xls(filename, cf.open_stream("Workbook" if cf.has_stream("Workbook") else "Book"))
    elif cf.has_stream("PowerPoint Document"):
        raise ValueError("PowerPoint 97-2003 is not supported")
    else:
        raise KeyError("EncryptionInfo")
    return "%s:$oldoffice$%d*%s*%s*%s" % (os.path.basename(filename), typ, salt.hex(), ev.hex(), evh.hex())


def get_hash(filename):
    cf = CompoundFile(open(filename, "rb").read())
    if not cf.has_stream("EncryptionInfo"):
        return _old_office(filename, cf)
    s = cf.open_stream("EncryptionInfo")
    major, minor, flags = struct.unpack_from("<HHI", s, 0)
    if flags == 16:
        raise ValueError("%s : An external cryptographic provider is not supported!" % filename)
    base = os.path.basename(filename)
    if major == 4 and minor == 4:                    # Agile (Office 2010/2013), XML descriptor
        if flags != 0x40:
            raise ValueError("%s : The encryption flags are not consistent with the encryption type" % filename)
        root = et.fromstring(s[8:])
        for node in root.iter("{http://schemas.microsoft.com/office/2006/keyEncryptor/password}encryptedKey"):
            a = node.attrib
            version = {"SHA1": 2010, "SHA512": 2013}.get(a.get("hashAlgorithm"))
            if version is None:
                raise ValueError("%s uses un-supported hashing algorithm %s" % (filename, a.get("hashAlgorithm")))
            hv = base64.b64decode(a["encryptedVerifierHashValue"]).hex()
            return "%s:$office$*%d*%d*%d*%d*%s*%s*%s" % (
                base, version, int(a["spinCount"]), int(a["keyBits"]), int(a["saltSize"]),
                base64.b64decode(a["saltValue"]).hex(), base64.b64decode(a["encryptedVerifierHashInput"]).hex(),
                hv[0:64])
        raise ValueError("%s : no password key encryptor" % filename)
    # Standard Encryption (Office 2007): EncryptionHeader then EncryptionVerifier (MS-OFFCRYPTO 2.3.4.5)
    header_len = struct.unpack_from("<I", s, 8)[0]
    key_size = struct.unpack_from("<I", s, 12 + 16)[0]        # flags, sizeExtra, algId, algHashId, keySize
    off = 12 + header_len
    salt_size = struct.unpack_from("<I", s, off)[0]
    if salt_size != 16:
        raise ValueError("%s : salt size %d (expected 16)" % (filename, salt_size))
    salt = s[off + 4:off + 20]
    ev = s[off + 20:off + 36]
    vh_size = struct.unpack_from("<I", s, off + 36)[0]
    evh = s[off + 40:off + 72]
    return "%s:$office$*%d*%d*%d*%d*%s*%s*%s" % (base, 2007, vh_size, key_size, salt_size, salt.hex(), ev.hex(),
                                                 evh.hex()[0:64])


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    for f in argv:
        sys.stdout.write(get_hash(f) + "\n")


if __name__ == "__main__":
    main()
