"""40-bit key search: the key index, its five bytes and the CLI's window (include/dprf.h "40-bit key search").

A key index ``i`` lies in ``[0, 2^40)`` and stands for the five bytes of ``i`` written big-endian: ``b0 = i >> 32`` and
``b4 = i & 0xff``, hex spelling ``"%010x" % i``.  That is the order ``itertools.product(range(256), repeat=5)`` gives.
Pure Python: nothing here touches the library.
"""
import re

SPACE = 1 << 40

# What the five bytes are, per key-search family (dprf_plan_chunk knows the names)
SENTENCES = {
    "pdf_r2": "The five bytes are the document's RC4 file key (PDF R2: RC4 of the padding string under it gives /U).",
    "pdf_r34": "The five bytes are the document's 40-bit RC4 file key (PDF R3/R4, Length 40: the 20-pass RC4 chain "
               "under it gives /U).",
    "office_rc4_md5": "The five bytes are h[0:5] of the password hash (Office 97-2003 RC4): MD5 of them and the block "
                      "number is the RC4 key of each 512-byte block.",
    "office_rc4_sha1": "The five bytes are the 40-bit RC4 CryptoAPI key material (Office 97-2003 type 3): they and "
                       "eleven zero bytes are the 16-byte RC4 key of block 0.",
}


def key_bytes(index):
    """The five key bytes of a key index, most significant first."""
    index = int(index)
    if not 0 <= index < SPACE:
        raise ValueError("key index %d outside [0, 2^40)" % index)
    return index.to_bytes(5, "big")


def key_hex(index):
    """The ten hex digits of a key index."""
    return key_bytes(index).hex()


def key_index(key):
    """The index of a key given as five bytes or as ten hex digits."""
    if isinstance(key, str):
        if not re.fullmatch(r"[0-9a-fA-F]{10}", key):
            raise ValueError("a 40-bit key is ten hex digits (got %r)" % key)
        key = bytes.fromhex(key)
    key = bytes(key)
    if len(key) != 5:
        raise ValueError("a 40-bit key is five bytes (got %d)" % len(key))
    return int.from_bytes(key, "big")


# After a key search's hit: how the key becomes a password (brute_force --key)
KEY_HINT = ("To search a password with this key, run the password search with --key %s (and -pr, --mask or --wordlist): "
            "any password it finds opens the document.")
# After a hit of a password search against a known key
COLLISION_NOTE = ("It is a password with the document's key %s: it opens the document, and it is not necessarily the "
                  "password the document was saved with.")


def known_key(key):
    """The five bytes of a known key given as five bytes or as ten hex digits (--key, Context.set_key40); ValueError
    for anything else."""
    if not isinstance(key, (str, bytes, bytearray)):
        raise ValueError("a 40-bit key is five bytes or ten hex digits (got %r)" % (key,))
    return key_bytes(key_index(key))


def parse_window(text):
    """"FROM-TO", ten hex digits each, both ends inclusive -> (first index, last index).  An empty string or None is
    the whole space."""
    if text is None or text == "":
        return 0, SPACE - 1
    m = re.fullmatch(r"([0-9a-fA-F]{10})-([0-9a-fA-F]{10})", text)
    if not m:
        raise ValueError("a key window is FROM-TO with ten hex digits each, both inclusive (got %r)" % text)
    lo, hi = key_index(m.group(1)), key_index(m.group(2))
    if lo > hi:
        raise ValueError("key window %s: FROM is above TO" % text)
    return lo, hi


def family(fields):
    """The SENTENCES entry of a verifier field list (brute_force.parse_verification_data), or None when the document is
    not a 40-bit one.  The library decides the domain (dprf_search_key40); this only picks the sentence."""
    try:
        if fields[0] == "pdf":
            rev, length = int(fields[2]), int(fields[3])
            if rev == 2:
                return "pdf_r2"
            return "pdf_r34" if rev in (3, 4) and length // 8 == 5 else None
        if fields[0] == "oldoffice":
            return {"0": "office_rc4_md5", "1": "office_rc4_md5", "3": "office_rc4_sha1"}.get(fields[1])
    except (ValueError, IndexError):
        pass
    return None
