"""The final compare of every verification kernel, in the rejecting direction.

The rest of the suite plants a password and checks that it is found and its neighbours are not.  A wrong candidate
differs from the stored verifier in every word, so that pins the hash chain but not the compare: a kernel comparing a
quarter of the verifier would pass.  Here the document is almost right instead.

A  Tampered verifiers.  From a stream its password verifies, one stream per byte position k of the stored verifier,
   differing in bit (3k + 1) % 8 of that byte (no bit lane and no byte lane of a word favoured), over the whole field,
   ignored bytes included.  Office and Agile verifiers are tampered in the plaintext and re-encrypted under the
   password's key.  The expected verdict is the CPU statement's -- pyoracle (Office 2007, ODF, PDF user), tests/
   agile_model.py, tests/owner_model.py -- and WIDTH below states what it must be, checked on the CPU first.  Every
   tampered stream goes through each compare site of its family (a Case's sites: the dispatch conditions are asserted
   on the CPU and cite dprf_host.cpp / the launchers declared in dprf_launch.h).
B  Prefilter survivors.  PDF R3/R4 throw a wave's candidates out after 2 keystream bytes and redo the wave in full
   when a lane's 2 bytes equal U[0:2].  The 16 compared bytes of a candidate do not depend on U, so a scan of a small
   keyspace finds pairs (A, B) with equal first two bytes; with U = bytes16(A) || ... A is the password and B a wrong
   candidate that passes the gate, placed in A's batch, the batch before or after it, or another workgroup.  R2 and
   R5 gate on 32 bits (no collision to be had): their mirror case tampers only the gated bytes.
C  The oracle's own widths against the reference executables (tests/golden/tamper_verdicts.json, written by tests/
   golden/make_tamper.py from part A's streams).

All comparisons are of whole hit sets, bit-exact.  Conditions on every stream, checked on the CPU: the context's flags
are 0, no hex field starts with a 00 byte (the seed is re-drawn instead), the untampered stream verifies the password
and rejects the near misses.

tests/owner_model.py costs 0.25 s per R6 candidate, so for R6 owner streams the model is evaluated for the password on
every tampered stream and for the other candidates once, on the untampered stream; a tampered stream is taken to reject
them too (they would need a 256-bit collision not to).
"""
import collections
import functools
import hashlib
import itertools
import random

import pytest

import agile_model as A
import docgen
import owner_model as M
import pyoracle as O
from conftest import load_golden
from test_planted_edges import OFFICE_HASH_SIZES

NT = 16
PDF_P = -3904


# ---------------------------------------------------------------- tampering
def tbit(k):
    return 1 << ((3 * k + 1) % 8)


def tamper(field, k):
    b = bytearray(field)
    b[k] ^= tbit(k)
    return bytes(b)


def _nz(*fields):
    """no hex field may begin with a 00 byte (the reference's decoder drops it: DPRF_FLAG_REF_NONDETERMINISTIC)"""
    return all(f[0] != 0 for f in fields)


def _draw(make, seed):
    """make(seed) -> a document (all its tampered streams included) or None when some field starts with 00"""
    for s in itertools.count(seed):
        doc = make(s)
        if doc is not None:
            return doc


def _rnd(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


# ---------------------------------------------------------------- documents: {None: stream, k: tampered stream}
def _pdf_line(name, R, n, meta, ID, U, O_):
    V = {2: 1, 3: 2, 4: 4, 5: 5, 6: 5}[R]
    return "%s.pdf:$pdf$*%d*%d*%d*%d*%d*%d*%s*%d*%s*%d*%s" % (name, V, R, 8 * n if R <= 4 else 256, PDF_P,
                                                                1 if meta else 0, len(ID), ID.hex(), len(U), U.hex(),
                                                                len(O_), O_.hex())


def pdf24_parts(user, owner, R, n, meta, seed):
    """ID, O and U of an R2-R4 document with these two passwords (tests/docgen.py's algorithms 2-5)."""
    rng = random.Random(seed)
    ID = _rnd(rng, 16)
    O_ = docgen._pdf_owner(owner, user, R, n)
    key = docgen._pdf_key(user, O_, PDF_P, ID, R, n, meta)
    if R == 2:
        U = O.rc4(key, docgen.PDF_PAD)
    else:
        c = O.rc4(key, hashlib.md5(docgen.PDF_PAD + ID).digest())
        for i in range(1, 20):
            c = O.rc4(bytes(k ^ i for k in key), c)
        U = c + _rnd(rng, 16)
    return ID, O_, U


def _pdf24_doc(name, user, owner, R, n, meta, seed0):
    def make(seed):
        ID, O_, U = pdf24_parts(user, owner, R, n, meta, seed)
        us = [U] + [tamper(U, k) for k in range(32)]
        if not _nz(ID, O_, *us):
            return None
        return {k: _pdf_line(name, R, n, meta, ID, u, O_) for k, u in zip([None] + list(range(32)), us)}
    return _draw(make, seed0)


def pdf56_parts(user, owner, R, seed):
    """ID, O and U (48 bytes each) of an R5 / R6 document: tests/docgen.py write_pdf's construction, the R6 user hash
    from the oracle's intermediates (as tests/golden/make_golden.py takes it), the owner hash from owner_model."""
    rng = random.Random(seed)
    ID, vs, ks, ovs, oks = _rnd(rng, 16), _rnd(rng, 8), _rnd(rng, 8), _rnd(rng, 8), _rnd(rng, 8)
    ub, ob = user.encode(), owner.encode()
    if R == 5:
        uh = hashlib.sha256(ub[:127] + vs).digest()
    else:
        dummy = _pdf_line("d", R, 32, True, b"\x01" * 16, b"\x01" * 32 + vs + ks, b"\x01" * 48)
        uh = O.Ctx(dummy).intermediates(ub)[:32]
    U = uh + vs + ks
    oh = hashlib.sha256(ob[:127] + ovs + U).digest() if R == 5 else M.r6_hash(ob, ovs, U)
    return ID, oh + ovs + oks, U


def _pdf56_doc(name, user, owner, R, field, seed0):
    def make(seed):
        ID, O_, U = pdf56_parts(user, owner, R, seed)
        if not _nz(ID, O_, U, tamper(O_, 0), tamper(U, 0)):
            return None
        out = {None: _pdf_line(name, R, 32, True, ID, U, O_)}
        for k in range(48):
            out[k] = (_pdf_line(name, R, 32, True, ID, tamper(U, k), O_) if field == "U" else
                      _pdf_line(name, R, 32, True, ID, U, tamper(O_, k)))
        return out
    return _draw(make, seed0)


@functools.lru_cache(maxsize=None)
def _office_key(pw, salt):
    return docgen.office_key(pw, salt)


def _office_line(name, hs, salt, key, verifier, vh):
    ev, evh = docgen._aes_ecb(key, verifier), docgen._aes_ecb(key, vh)
    return _nz(salt, ev, evh) and "%s.docx:$office$*2007*%d*128*16*%s*%s*%s" % (name, hs, salt.hex(), ev.hex(),
                                                                              evh.hex())


def office_parts(pw, seed):
    rng = random.Random(seed)
    salt, verifier = _rnd(rng, 16), _rnd(rng, 16)
    return salt, _office_key(pw, salt), verifier, hashlib.sha1(verifier).digest() + b"\0" * 12


def _office_doc(name, pw, field, seed0):
    """field "hash": the 32 plaintext bytes of the verifier hash tampered before AES-ECB encryption under the
    password's key; "verifier": the 16 plaintext verifier bytes, the hash kept."""
    def make(seed):
        salt, key, verifier, vh = office_parts(pw, seed)
        if salt[0] == 0:
            return None
        out = {None: _office_line(name, 20, salt, key, verifier, vh)}
        for k in range(32 if field == "hash" else 16):
            out[k] = (_office_line(name, 20, salt, key, verifier, tamper(vh, k)) if field == "hash" else
                      _office_line(name, 20, salt, key, tamper(verifier, k), vh))
        return out if all(out.values()) else None
    return _draw(make, seed0)


def _agile_doc(name, pw, version, bits, field, seed0):
    def make(seed):
        salt, verifier, hv = A.plain_parts(version, seed)
        out = {}
        for k in [None] + list(range(32 if field == "hash" else 16)):
            v, h = verifier, hv
            if k is not None and field == "hash":
                h = tamper(hv, k)
            elif k is not None:
                v = tamper(verifier, k)
            parts = A.make_parts_from(pw, version, bits, 3, salt, v, h)
            if not _nz(*parts):
                return None
            out[k] = A.stream_of(version, bits, 3, *parts, name=name + ".docx")
        return out
    return _draw(make, seed0)


def _odt_line(name, checksum, iv, salt, enc):
    return _nz(checksum, iv, salt, enc) and "%s.odt:$odt$*1.2*%s*%s*%s*%s*%d" % (name, checksum.hex(), iv.hex(),
                                                                               salt.hex(), enc.hex(), len(enc))


def odt_parts(pw, n, seed):
    rng = random.Random(seed)
    salt, iv, plain = _rnd(rng, 16), _rnd(rng, 16), _rnd(rng, n)
    return salt, iv, docgen.odt_key(pw, salt), plain


def _odt_doc(name, pw, seed0):
    def make(seed):
        salt, iv, key, plain = odt_parts(pw, 64, seed)
        enc, checksum = docgen._aes_cbc(key, iv, plain), hashlib.sha256(plain).digest()
        out = {None: _odt_line(name, checksum, iv, salt, enc)}
        for k in range(32):
            out[k] = _odt_line(name, tamper(checksum, k), iv, salt, enc)
        return out if all(out.values()) else None
    return _draw(make, seed0)


# ---------------------------------------------------------------- cases, sites and the width table
Site = collections.namedtuple("Site", "id doc kind cs words hit cond cite positions half")
# kind "range" / "mask": a window of `half` each side of the password in cs ^ len(pw); "list": `words`, of which the
# indices `hit` are the password (or equal to it as far as the reference reads).  cond(site, pw): the dispatch
# condition that sends the call through the compare site, cite: where the library decides it.


def _range(id, cs, cond=None, cite="", doc="short", kind="range", positions=None, half=150):
    return Site(id, doc, kind, cs, None, None, cond or (lambda s, pw: True), cite, positions, half)


def _list(id, words, hit, cond=None, cite="", doc="short"):
    return Site(id, doc, "list", None, tuple(words), tuple(hit), cond or (lambda s, pw: True), cite, None, 0)


class Case:
    def __init__(self, id, kind, mode, n, miss, pws, doc, sites):
        self.id, self.kind, self.mode, self.n, self.miss = id, kind, mode, n, frozenset(miss)
        self.pws, self._doc, self.sites = pws, doc, sites

    @functools.lru_cache(maxsize=None)
    def doc(self, which):
        return self._doc(which)

    def fields(self, stream):
        return A.fields_of(stream) if self.kind == "agile" else O.split_stream(stream)


U_PW, U_LONG32, U_LONG64 = "Tq8$z", "Tq8$z" * 8, "Tq8$z" * 14          # 5, 40 (> 32) and 70 (> 64) bytes
O_PW, O_LONG32 = "Ow7", "Ow7#k" * 8

CITE_R24 = ("dprf_kernels.hip launch_pdf_r24 (declared in dprf_launch.h): e.mode 0 -> k_pdf_r24<0, ..>, the list "
            "-> <1, ..>; dprf_doc.cpp convert_candidate: the pdf_r24 row of FAMILIES cuts at 32 bytes, so the word "
            "stays in the slot sub-list of dprf_verify_list")
CITE_R5 = ("dprf_kernels.hip launch_pdf_r5 (dprf_launch.h): L5W picks runs of 16 for e.cslen >= 16, else PER 8, and "
           "k_pdf_r5 takes the run path only when e.cslen >= PER; list launches: e.pwlen <= 8 -> L5(1, 2, 8), "
           "<= 16 -> L5(1, 4, 8) (one block, sha256_block_matches), else L5(1, 8, 8) (sha256_msg2); dprf_host.cpp "
           "dprf_verify_list: a candidate over the 64-byte slot goes to the long sub-list (e.mode 2, DPRF_LONG_R5)")
CITE_R6 = ("dprf_kernels_r6.hip launch_pdf_r6 (dprf_launch.h): e.mode 0 / 1 / 2 -> k_pdf_r6<0 / 1 / 2>, p.owner -> "
           "k_pdf_r6_owner; dprf_host.cpp dprf_verify_list: over 64 bytes -> the long sub-list (e.mode 2)")
CITE_2K = ("dprf_host.cpp launch(): launch_office / launch_agile / launch_odt (dprf_launch.h) run the format's KDF "
           "kernel in e.mode 0 (range) or 1 (list), then its check kernel (k_office_check / k_agile_check<SHA512, "
           "KEY256> / k_odt_check), which holds the compare")


def _near(pw):
    return [pw[:-1] + ("y" if pw[-1] != "y" else "x"), pw, pw[:-1]]


def _cut32(pw):
    return [pw[:31] + "!" + pw[32:], pw, pw[:32] + "#tail"]


def _all_over(n):
    return lambda s, pw: all(len(w.encode()) > n for w in s.words)


def _cases():
    out = []
    seed = itertools.count(0x7A00, 0x40)
    # PDF R2-R4, user and owner: U, 32 bytes.  R2 compares all of them, R >= 3 the first 16 (pdf...c:184-189).
    for vid, R, n, meta in (("r2", 2, 5, True), ("r3-40", 3, 5, True), ("r3-128", 3, 16, True), ("r4", 4, 16, True),
                            ("r4-nometa", 4, 16, False)):
        s0 = next(seed)
        doc = functools.partial(
            lambda which, vid, R, n, meta, s0: _pdf24_doc(
                "%s-%s" % (vid, which), U_PW if which == "short" else U_LONG32,
                O_PW if which == "short" else O_LONG32, R, n, meta, s0 + (which == "long")),
            vid=vid, R=R, n=n, meta=meta, s0=s0)
        miss = range(32) if R == 2 else range(16)
        out.append(Case("pdf-%s-user" % vid, "pdf", "user", 32, miss, {"short": U_PW, "long": U_LONG32}, doc, [
            _range("range", "$8Tqz", cite=CITE_R24),
            _list("list32", _cut32(U_LONG32), [1, 2], _all_over(32), CITE_R24, doc="long"),
            _range("mask", "$8Tqz", cite=CITE_R24, kind="mask", positions="edges")]))
        out.append(Case("pdf-%s-owner" % vid, "pdf", "owner", 32, miss, {"short": O_PW, "long": O_LONG32}, doc, [
            _range("range", "7#Owk", cite=CITE_R24),
            _list("list32", _cut32(O_LONG32), [1, 2], _all_over(32), CITE_R24, doc="long"),
            _range("mask", "7#Owk", cite=CITE_R24, kind="mask", positions="edges")]))
    # PDF R5 / R6 user: U, 48 bytes = hash[32] || validation salt[8] || key salt[8]; the key salt is not read
    r5_sites = [
        _range("range-cs5", "$8Tqz", lambda s, pw: len(s.cs) < 8, CITE_R5),
        _range("range-cs9", "$8Tqz7ayk", lambda s, pw: 8 <= len(s.cs) < 16, CITE_R5),
        _range("range-cs17", "$8Tqzabcdefghijkl", lambda s, pw: len(s.cs) >= 16, CITE_R5),
        _list("list-8", _near(U_PW), [1], lambda s, pw: max(len(w) for w in s.words) <= 8, CITE_R5),
        _list("list-2blk", [U_PW + "x" * 15, U_PW, U_PW[:-1]], [1],
              lambda s, pw: 16 < max(len(w) for w in s.words) <= 64, CITE_R5),
        _list("list-long", _near(U_LONG64), [1], _all_over(64), CITE_R5, doc="long"),
        _range("mask", "$8Tqz", cite=CITE_R5, kind="mask", positions=(0, 31, 32, 39, 40))]
    r6_sites = [
        _range("range", "$8Tqz", cite=CITE_R6, half=64),
        _list("list", _near(U_PW), [1], cite=CITE_R6),
        _list("list-long", _near(U_LONG64), [1], _all_over(64), CITE_R6, doc="long"),
        _range("mask", "$8Tqz", cite=CITE_R6, kind="mask", positions=(0, 31, 32, 39, 40), half=64)]
    for R, sites in ((5, r5_sites), (6, r6_sites)):
        s0 = next(seed)
        doc = functools.partial(
            lambda which, R, s0: _pdf56_doc("r%d-%s" % (R, which), U_PW if which == "short" else U_LONG64, O_PW, R,
                                            "U", s0 + (which == "long")), R=R, s0=s0)
        out.append(Case("pdf-r%d-user" % R, "pdf", "user", 48, range(40), {"short": U_PW, "long": U_LONG64}, doc,
                        sites))
    # PDF R5 / R6 owner: SHA-256 / 2.B of pw || O[32:40] || U[0:48] against O[0:32] (tests/owner_model.py): every
    # byte of U counts, and O like a user's U
    for R in (5, 6):
        s0 = next(seed)
        pw, cs = (O_PW, "7#Owk") if R == 5 else ("aba", "ab")
        for field, miss in (("O", range(40)), ("U", range(48))):
            doc = functools.partial(
                lambda which, R, field, pw, s0: _pdf56_doc("r%d-own%s" % (R, field), U_PW, pw, R, field, s0),
                R=R, field=field, pw=pw, s0=s0)
            out.append(Case("pdf-r%d-owner-%s" % (R, field), "pdf", "owner", 48, miss, {"short": pw}, doc, [
                _range("range", cs, cite=CITE_R5 if R == 5 else CITE_R6),
                _list("list", _near(pw), [1], cite=CITE_R5 if R == 5 else CITE_R6),
                _range("mask", cs, cite=CITE_R5 if R == 5 else CITE_R6, kind="mask", positions=(0, 31, 32, 39, 40))]))
    # Office 2007: decryptedVerifierHash, 32 bytes: SHA-1 in 0-19, then the byte hash_size = 20 must be zero
    # (msoffcrypto...c:168), the rest is padding nobody reads; and the 16-byte verifier
    k2 = [_range("range", "678Ux", cite=CITE_2K), _list("list", _near("Ux7"), [1], cite=CITE_2K),
          _range("mask", "678Ux", cite=CITE_2K, kind="mask", positions="edges")]
    for field, n, miss in (("hash", 32, range(21)), ("verifier", 16, range(16))):
        s0 = next(seed)
        out.append(Case("office-" + field, "office", "user", n, miss, {"short": "Ux7"}, functools.partial(
            lambda which, field, s0: _office_doc("tamper-" + field, "Ux7", field, s0), field=field, s0=s0), k2))
    # Agile: SHA-1 compares 20 bytes of the hash value, SHA-512 the 32 the stream keeps
    for version, bits in (("2010", 128), ("2010", 256), ("2013", 128), ("2013", 256)):
        for field, n, miss in (("hash", 32, range(20 if version == "2010" else 32)), ("verifier", 16, range(16))):
            s0 = next(seed)
            name = "agile-%s-%d-%s" % (version, bits, field)
            out.append(Case(name, "agile", "user", n, miss, {"short": "Ux7"}, functools.partial(
                lambda which, name, version, bits, field, s0: _agile_doc(name, "Ux7", version, bits, field, s0),
                name=name, version=version, bits=bits, field=field, s0=s0), k2))
    # ODF: the SHA-256 checksum, 32 bytes
    s0 = next(seed)
    out.append(Case("odt-checksum", "odt", "user", 32, range(32), {"short": "Lk9"},
                    functools.partial(lambda which, s0: _odt_doc("tamper", "Lk9", s0), s0=s0),
                    [_range("range", "#9Lkq", cite=CITE_2K), _list("list", _near("Lk9"), [1], cite=CITE_2K),
                     _range("mask", "#9Lkq", cite=CITE_2K, kind="mask", positions="edges")]))
    return out


CASES = _cases()
PARAMS = [pytest.param(c, s, id="%s-%s" % (c.id, s.id)) for c in CASES for s in c.sites]


def _parts(case, site):
    """The families whose candidates cost most (R6's hardened hash, Office 2007's 50,000 iterations) take the tampered
    positions of a whole field in four tests, not one."""
    return 4 if site.positions is None and (case.kind == "office" or "-r6-" in case.id) else 1


GPU_PARAMS = [pytest.param(c, s, (i, _parts(c, s)), id="%s-%s%s" % (c.id, s.id, "-%d" % i if _parts(c, s) > 1 else ""))
              for c in CASES for s in c.sites for i in range(_parts(c, s))]

# family -> (tampered field bytes, positions at which the password must miss); the rest must still hit
WIDTH = {"pdf-r2": (32, range(32)), "pdf-r3": (32, range(16)), "pdf-r4": (32, range(16)),
         "pdf-r5-user": (48, range(40)), "pdf-r6-user": (48, range(40)),
         "pdf-r5-owner-O": (48, range(40)), "pdf-r6-owner-O": (48, range(40)),
         "pdf-r5-owner-U": (48, range(48)), "pdf-r6-owner-U": (48, range(48)),
         "office-hash": (32, range(21)), "office-verifier": (16, range(16)),
         "agile-2010": (32, range(20)), "agile-2013": (32, range(32)), "agile-verifier": (16, range(16)),
         "odt-checksum": (32, range(32))}


def _width_of(case):
    if case.id.endswith("-verifier") and case.kind == "agile":
        return WIDTH["agile-verifier"]
    keys = [k for k in WIDTH if case.id.startswith(k)]
    assert keys, case.id
    return WIDTH[max(keys, key=len)]


# ---------------------------------------------------------------- the CPU statement
def _pw_only(case):
    return case.mode == "owner" and "-r6-" in case.id


def _verdict(case, stream, pw):
    if case.kind == "agile":
        return int(A.verifies(stream, pw))
    if case.mode == "owner":
        return int(M.owner_verifies(stream, pw))
    return O.Ctx(stream).verify(pw)


def _window(site, pw):
    idx, total = A.index_of(pw, site.cs), len(site.cs) ** len(pw)
    start = max(0, idx - site.half)
    return idx, start, min(2 * site.half, total - start)


@functools.lru_cache(maxsize=None)
def _want_cached(case, site, stream):
    return tuple(_want_raw(case, site, stream))


def _want_raw(case, site, stream):
    pw = case.pws[site.doc]
    if site.kind == "list":
        if case.kind == "pdf" and case.mode == "user" or case.kind in ("office", "odt"):
            v = O.Ctx(stream).verify_list(site.words, nthreads=NT)
        else:
            v = [_verdict(case, stream, w) for w in site.words]
        return [i for i, x in enumerate(v) if x == 1]
    idx, start, count = _window(site, pw)
    if case.kind == "agile":
        return [i for i in range(start, start + count) if A.verifies(stream, A.word(i, site.cs, len(pw)))]
    if case.mode == "owner":
        return [start + k for k in M.window_hits(stream, site.cs, len(pw), start, count)]
    return O.Ctx(stream).search_range(site.cs, len(pw), start, count, nthreads=NT)[0]


def want(case, site, k):
    """The CPU statement's hit set for the site's call on the stream tampered at k (None: untampered)."""
    doc = case.doc(site.doc)
    if k is None or not _pw_only(case):
        return list(_want_cached(case, site, doc[k])) if k is None else _want_raw(case, site, doc[k])
    base = list(_want_cached(case, site, doc[None]))
    pw = case.pws[site.doc]
    mine = list(site.hit) if site.kind == "list" else [A.index_of(pw, site.cs)]
    assert base == mine
    return base if _verdict(case, doc[k], pw) == 1 else []


def table(case, site, k):
    """What WIDTH says the hit set must be."""
    if k is not None and k in case.miss:
        return []
    return list(site.hit) if site.kind == "list" else [A.index_of(case.pws[site.doc], site.cs)]


def positions(case, site, part=None):
    """None (the untampered stream) and the tampered positions of the site: all of the field, or for the device-spelled
    call "edges" -- both ends of the compared width and the first byte outside it -- or the ones it names.  part: the
    slice (i, of) of them a split test takes."""
    if site.positions == "edges":
        ks = sorted({0, max(case.miss)} | ({max(case.miss) + 1} if max(case.miss) + 1 < case.n else set()))
    else:
        ks = list(range(case.n) if site.positions is None else site.positions)
    ks = [None] + ks
    if part is None:
        return ks
    i, of = part
    step = -(-len(ks) // of)
    return ks[i * step:(i + 1) * step]


# ---------------------------------------------------------------- A, on the CPU
def test_tamper_bits_favour_no_lane():
    assert sorted({tbit(k) for k in range(8)}) == [1 << b for b in range(8)]
    for w in range(12):                                   # the four bytes of every word flip four different bits
        assert len({tbit(4 * w + j) for j in range(4)}) == 4
    assert tamper(b"\0" * 4, 1) == b"\0\x10\0\0"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_width_table_agrees_with_the_cpu_statement(case):
    n, miss = _width_of(case)
    assert (n, frozenset(miss)) == (case.n, case.miss)
    words = {k // 4 for k in case.miss}
    assert words == set(range((max(case.miss) + 4) // 4)), "a tampered position in every word of the compared width"
    for which in sorted({s.doc for s in case.sites}):
        doc, pw = case.doc(which), case.pws[which]
        assert sorted(doc, key=lambda k: -1 if k is None else k) == [None] + list(range(n))
        assert len(set(doc.values())) == n + 1
        for k, stream in doc.items():
            f = case.fields(stream)
            assert all(x[:2] != "00" for x in f[1:] if len(x) >= 16), (k, "a hex field starts with 00")
            if case.kind != "agile":
                assert O.Ctx(stream).flags == 0, k
            assert _verdict(case, stream, pw) == (0 if k in case.miss else 1), (case.id, which, k)


@pytest.mark.parametrize("case,site", PARAMS)
def test_sites_meet_their_dispatch_condition(case, site):
    pw = case.pws[site.doc]
    assert site.cite and site.cond(site, pw), (case.id, site.id, site.cite)
    if site.kind == "list":
        assert all(site.words[i] == pw or case.id.startswith("pdf-r") and site.words[i][:32] == pw[:32]
                   for i in site.hit) and len(site.words) == 3 and 1 in site.hit
    else:
        idx, start, count = _window(site, pw)
        assert len(set(site.cs)) == len(site.cs) and start <= idx < start + count <= len(site.cs) ** len(pw)
        assert count <= 300 and len(pw) <= 32
    # the untampered stream verifies the password and rejects the near misses
    assert want(case, site, None) == table(case, site, None)
    ks = positions(case, site)[1:]
    assert all(0 <= k < case.n for k in ks) and any(k in case.miss for k in ks)
    if max(case.miss) + 1 < case.n:
        assert any(k not in case.miss for k in ks)
    assert sum((positions(case, site, (i, _parts(case, site))) for i in range(_parts(case, site))), []) == [None] + ks


def test_r5_and_r24_cases_cover_every_site():
    r5 = {s.id for c in CASES if c.id == "pdf-r5-user" for s in c.sites}
    assert {"range-cs5", "range-cs9", "range-cs17", "list-8", "list-2blk", "list-long"} <= r5
    r6 = {s.id for c in CASES if c.id == "pdf-r6-user" for s in c.sites}
    assert {"range", "list", "list-long"} <= r6 and any(c.id.startswith("pdf-r6-owner") for c in CASES)
    for v in ("r2", "r3-40", "r3-128", "r4", "r4-nometa"):
        for mode in ("user", "owner"):
            assert {"range", "list32", "mask"} == {s.id for c in CASES if c.id == "pdf-%s-%s" % (v, mode)
                                                   for s in c.sites}
    assert len(U_LONG32) > 32 and len(O_LONG32) > 32 and 64 < len(U_LONG64) <= 176


# ---------------------------------------------------------------- A, on the device
@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device: GPU tests need the MI355X box"
    return _lib


def _call(ctx, case, site):
    pw = case.pws[site.doc]
    if site.kind == "list":
        hits, n, st = ctx.verify_list(site.words)
        return hits, n, st, len(site.words)
    _, start, count = _window(site, pw)
    if site.kind == "mask":
        hits, n, st = ctx.search_mask([site.cs] * len(pw), start, count)
    else:
        hits, n, st = ctx.search_range(site.cs, len(pw), start, count)
    return hits, n, st, count


@pytest.mark.gpu
@pytest.mark.parametrize("case,site,part", GPU_PARAMS)
def test_gpu_tampered_verifier(dprf, case, site, part):
    """The password on a stream tampered at k hits exactly where WIDTH (and the CPU statement) say so, through this
    site; the whole hit set is compared, so a missing and an extra hit both fail."""
    doc = case.doc(site.doc)
    for k in positions(case, site, part):
        exp = want(case, site, k)
        assert exp == table(case, site, k), (case.id, site.id, k)
        with dprf.Context(case.fields(doc[k]), device=0, pdf_password=case.mode) as ctx:
            assert ctx.flags == 0
            hits, n, st, count = _call(ctx, case, site)
            assert hits == exp and n == len(exp), (case.id, site.id, k, hits, exp)
            assert st["candidates"] == count, (case.id, site.id, k)


# ---------------------------------------------------------------- A: Office hash_size gate, rejecting direction
def office_gate_stream(hs):
    """decrypted byte hs non-zero while SHA1(verifier) == dec[0:20]: inside the hash a verifier whose SHA-1 has a
    non-zero byte there, past it a non-zero padding byte.  Returns (stream, the stream with the byte as written by a
    real document where that differs -- hs >= 20 -- else None)."""
    def make(seed):
        salt, key, verifier, vh = office_parts("Ux7", seed)
        bad = vh if hs < 20 else vh[:hs] + bytes([0x5A]) + vh[hs + 1:]
        if bad[hs] == 0 or salt[0] == 0:
            return None
        assert hashlib.sha1(verifier).digest() == bad[:20]
        s = _office_line("gate%d" % hs, hs, salt, key, verifier, bad)
        good = _office_line("gate%d" % hs, hs, salt, key, verifier, vh) if hs >= 20 else None
        return (s, good) if s and good is not False else None
    return _draw(make, 0x6A7E + 64 * hs)


@pytest.mark.parametrize("hs", OFFICE_HASH_SIZES)
def test_office_gate_streams_on_the_oracle(hs):
    s, good = office_gate_stream(hs)
    assert O.Ctx(s).flags == 0 and O.Ctx(s).verify(b"Ux7") == 0
    if good:
        assert O.Ctx(good).verify(b"Ux7") == 1             # the gate byte alone decides


@pytest.mark.gpu
def test_gpu_office_hash_size_gate_rejects(dprf):
    cs, words = "678Ux", _near("Ux7")
    idx = A.index_of("Ux7", cs)
    for hs in OFFICE_HASH_SIZES:
        s, good = office_gate_stream(hs)
        for stream in filter(None, (s, good)):
            octx = O.Ctx(stream)
            exp_l = [i for i, v in enumerate(octx.verify_list(words, nthreads=NT)) if v == 1]
            exp_r = octx.search_range(cs, 3, 0, 125, nthreads=NT)[0]
            assert exp_r == ([] if stream is s else [idx]) and exp_l == ([] if stream is s else [1])
            with dprf.Context(O.split_stream(stream), device=0) as ctx:
                assert ctx.flags == 0
                assert ctx.verify_list(words)[0] == exp_l, hs
                assert ctx.search_range(cs, 3, 0, 125)[0] == exp_r, hs


# ---------------------------------------------------------------- A: ODF 2-byte check and checksum coverage
ODT_E = [("0300", True), ("0300ffff", True), ("0301", False), ("0200", False), ("0003", False), ("0380", False)]


def odt_e_stream(prefix_hex):
    pre = bytes.fromhex(prefix_hex)

    def make(seed):
        salt, iv, key, plain = odt_parts("Lk9", 16, seed)
        plain = pre + plain[len(pre):]
        return _odt_line("e-" + prefix_hex, hashlib.sha256(plain).digest(), iv, salt,
                         docgen._aes_cbc(key, iv, plain)) or None
    return _draw(make, 0x0E00 + int(prefix_hex[:4], 16))


def odt_cover_stream(n, at):
    """enc_len n, plaintext bit flipped at byte `at` after the checksum was taken over the first min(n, 1024) bytes"""
    def make(seed):
        salt, iv, key, plain = odt_parts("Lk9", n, seed)
        checksum = hashlib.sha256(plain[:1024]).digest()
        return _odt_line("cover%d" % n, checksum, iv, salt, docgen._aes_cbc(key, iv, tamper(plain, at))) or None
    return _draw(make, 0xC0E0 + n)


ODT_EXTRA = ([("e-" + p, functools.partial(odt_e_stream, p), hit) for p, hit in ODT_E] +
             [("cover-1024-last-block", functools.partial(odt_cover_stream, 1024, 1015), False),
              ("cover-1040-byte-1030", functools.partial(odt_cover_stream, 1040, 1030), True)])


@pytest.mark.parametrize("name,make,hit", ODT_EXTRA, ids=[e[0] for e in ODT_EXTRA])
def test_odt_extra_streams_on_the_oracle(name, make, hit):
    octx = O.Ctx(make())
    assert octx.flags == 0 and octx.verify(b"Lk9") == int(hit)
    assert 1008 <= 1015 < 1024 <= 1030 < 1040


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,hit", ODT_EXTRA, ids=[e[0] for e in ODT_EXTRA])
def test_gpu_odt_extra_streams(dprf, name, make, hit):
    cs, words, stream = "#9Lkq", _near("Lk9"), make()
    octx = O.Ctx(stream)
    exp_l = [i for i, v in enumerate(octx.verify_list(words, nthreads=NT)) if v == 1]
    exp_r = octx.search_range(cs, 3, 0, 125, nthreads=NT)[0]
    assert (1 in exp_l) == hit and (A.index_of("Lk9", cs) in exp_r) == hit
    with dprf.Context(O.split_stream(stream), device=0) as ctx:
        assert ctx.flags == 0
        assert ctx.verify_list(words)[0] == exp_l
        assert ctx.search_range(cs, 3, 0, 125)[0] == exp_r
        assert ctx.search_mask([cs] * 3, 0, 125)[0] == exp_r


# ---------------------------------------------------------------- B: R3/R4 survivors by collision
COLL_CS, COLL_N = "$8Tqyz7", 5
COLL_TOTAL = len(COLL_CS) ** COLL_N                                  # 16 807
COLL = {"r3-128": (3, 16, True, 99), "r3-40": (3, 5, True, 99), "r4-nometa": (4, 16, False, 99)}
OWN_CS, OWN_N = "7#Owk$8T", 4                                        # 4096 owner candidates


def relation(a, b, start):
    """Where the survivor b sits relative to the password a in a launch that starts at `start` (k_pdf_r24: batches of
    64 lanes, 12 batches per workgroup, both counted from the launch's first candidate)."""
    ba, bb = (a - start) // 64, (b - start) // 64
    if ba == bb:
        return "same-batch"
    if ba // 12 != bb // 12:
        return "other-workgroup"
    return {1: "batch-before", -1: "batch-after"}.get(ba - bb, "same-workgroup")


@functools.lru_cache(maxsize=None)
def coll_scan(inst, owner=False):
    """(ID, O, U, the 16 compared bytes of every candidate, ordered pairs (A, B) with equal first two bytes)"""
    R, n, meta, seed = COLL[inst]
    cs, npw = (OWN_CS, OWN_N) if owner else (COLL_CS, COLL_N)
    def make(s):
        parts = pdf24_parts("Tq8$z", "7Owk", R, n, meta, s)
        return parts if _nz(*parts) else None
    ID, O_, U = _draw(make, seed)
    stream = _pdf_line("coll", R, n, meta, ID, U, O_)
    if owner:
        b16 = [M.compared_bytes(stream, A.word(i, cs, npw)) for i in range(len(cs) ** npw)]
    else:
        octx = O.Ctx(stream)
        b16 = [octx.intermediates(A.word(i, cs, npw))[48:64] for i in range(len(cs) ** npw)]
    by2 = collections.defaultdict(list)
    for i, b in enumerate(b16):
        by2[b[:2]].append(i)
    pairs = [(a, b) for g in by2.values() if len(g) > 1 for a in g for b in g
             if a != b and b16[a] != b16[b] and b16[a][0] != 0]
    return ID, O_, U, b16, sorted(pairs)


def coll_doc(inst, rel, owner=False):
    """(stream, A, B, start, count) of the document for one relation.  A is the password, except in "both-survive",
    where A and B both pass the gate and neither verifies."""
    R, n, meta, _ = COLL[inst]
    ID, O_, U, b16, pairs = coll_scan(inst, owner)
    total = len(b16)
    start, count = 0, total
    pick = lambda want, s=0: next((a, b) for a, b in pairs if min(a, b) >= s and relation(a, b, s) == want)
    if rel == "both-survive":
        # the shared first two bytes, then half of B's and half of A's remaining bytes: both lanes pass the gate and the
        # full pass must reject both (A[0:2] || B[2:16] would simply be B's bytes, the two prefixes being equal)
        a, b = next((a, b) for a, b in pairs if relation(a, b, 0) == "same-batch" and b16[a][2:9] != b16[b][2:9]
                    and b16[a][9:] != b16[b][9:])
        u16 = b16[a][:2] + b16[b][2:9] + b16[a][9:]
    elif rel == "odd-start":
        # relation 1's document from a start that puts the later of the two on lane 0 of a batch
        a, b = next((a, b) for a, b in pairs if relation(a, b, 0) == "same-batch" and 0 < max(a, b) % 64 <= min(a, b)
                    and relation(a, b, max(a, b) % 64) in ("batch-before", "batch-after"))
        start, u16 = max(a, b) % 64, b16[a]
        count = total - start
    elif rel == "partial-last-batch":
        a, b = next((a, b) for a, b in pairs if a + 64 < b and (b + 1) % 64 and relation(a, b, 0) == "other-workgroup")
        count, u16 = b + 1, b16[a]
    else:
        a, b = pick(rel)
        u16 = b16[a]
    stream = _pdf_line("coll-" + rel, R, n, meta, ID, u16 + U[16:], O_)
    return stream, a, b, start, count


COLL_PARAMS = ([(i, r, False) for i in COLL for r in ("same-batch", "batch-before", "batch-after", "other-workgroup")] +
               [("r3-128", r, False) for r in ("both-survive", "odd-start", "partial-last-batch")] +
               [("r3-128", "same-batch", True), ("r3-128", "other-workgroup", True)])
COLL_IDS = ["%s-%s%s" % (i, r, "-owner" if o else "") for i, r, o in COLL_PARAMS]


def coll_want(inst, rel, owner):
    stream, a, b, start, count = coll_doc(inst, rel, owner)
    if not owner:
        return O.Ctx(stream).search_range(COLL_CS, COLL_N, start, count, nthreads=NT)[0]
    # owner_model's statement of every candidate's compared bytes against the 16 bytes of U the check reads
    b16, u16 = coll_scan(inst, True)[3], M.parse(stream)["U"][:16]
    return [i for i in range(start, start + count) if b16[i] == u16]


@pytest.mark.parametrize("inst,rel,owner", COLL_PARAMS, ids=COLL_IDS)
def test_collision_documents_on_the_cpu(inst, rel, owner):
    from dprf_amd import _lib
    stream, a, b, start, count = coll_doc(inst, rel, owner)
    b16 = coll_scan(inst, owner)[3]
    u = M.parse(stream)["U"]
    assert O.Ctx(stream).flags == 0 and u[0] != 0
    assert b16[b][:2] == u[:2] and b16[b] != u[:16], "B passes the 2-byte gate and is not the password"
    if rel == "both-survive":
        assert b16[a][:2] == u[:2] and b16[a] != u[:16], "so does A, and neither is the password"
    assert start <= b < start + count
    assert coll_want(inst, rel, owner) == ([] if rel == "both-survive" else [a])
    cs, n = (OWN_CS, OWN_N) if owner else (COLL_CS, COLL_N)
    if owner:
        assert M.owner_verifies(stream, A.word(a, cs, n)) and not M.owner_verifies(stream, A.word(b, cs, n))
    else:
        assert O.Ctx(stream).verify(A.word(b, cs, n)) == 0
    # one launch on one device, so batches and workgroups count from `start` (dprf_doc.cpp policy / plan_chunk:
    # K_PDF_R24's first chunk is 2^24, halved for the owner kernels)
    assert _lib.plan_chunk("pdf_r24_owner" if owner else "pdf_r24", 0.0, count, count, 1) == count
    want_rel = {"both-survive": ("same-batch",), "odd-start": ("batch-before", "batch-after"),
                "partial-last-batch": ("other-workgroup",)}.get(rel, (rel,))
    assert relation(a, b, start) in want_rel, (a, b, start)
    if rel == "odd-start":
        assert start % 64 != 0 and relation(a, b, 0) == "same-batch"
    if rel == "partial-last-batch":
        assert count % 64 != 0 and (b - start) // 64 == (count - 1) // 64 and (a - start) // 64 != (b - start) // 64


@pytest.mark.gpu
@pytest.mark.parametrize("inst,rel,owner", COLL_PARAMS, ids=COLL_IDS)
def test_gpu_redo_rejects_the_survivor(dprf, inst, rel, owner):
    """A wrong candidate whose first two bytes equal U[0:2] sends its wave through the full 16-byte pass, which must
    throw it out and keep the password (in the same batch, the next, the previous, another workgroup)."""
    stream, a, b, start, count = coll_doc(inst, rel, owner)
    exp = coll_want(inst, rel, owner)
    assert exp == ([] if rel == "both-survive" else [a])
    cs, n = (OWN_CS, OWN_N) if owner else (COLL_CS, COLL_N)
    for devs in ([0], [0, 0]):
        with dprf.Context(O.split_stream(stream), devices=devs, pdf_password="owner" if owner else "user") as ctx:
            hits, nh, st = ctx.search_range(cs, n, start, count)
            assert hits == exp and nh == len(exp) and st["candidates"] == count, (devs, hits, exp, b)
            first, _, _ = ctx.search_range(cs, n, start, count, stop_on_first=True, cap=1)
            assert first == exp[:1], (devs, first)


# ---------------------------------------------------------------- B: the 32-bit gates of R2 and R5, mirrored
def gate_only_stream(R):
    """U tampered in the gated bytes alone -- R2: U[0:4] (the first keystream word), R5: U[28:32] (the digest word the
    round-61 exit looks at) -- one bit in each of the four bytes, the rest of U kept"""
    case = next(c for c in CASES if c.id == ("pdf-r2-user" if R == 2 else "pdf-r5-user"))
    f = O.split_stream(case.doc("short")[None])
    u = bytes.fromhex(f[9])
    for k in range(4) if R == 2 else range(28, 32):
        u = tamper(u, k)
    f[9] = u.hex()
    return "gate.pdf:$pdf$*" + "*".join(f[1:]), u


@pytest.mark.parametrize("R", [2, 5])
def test_gate_only_streams_on_the_oracle(R):
    stream, u = gate_only_stream(R)
    octx = O.Ctx(stream)
    assert octx.flags == 0 and u[0] != 0 and octx.verify(U_PW) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 5])
def test_gpu_gate_only_tamper(dprf, R):
    stream, _ = gate_only_stream(R)
    for cs in ("$8Tqz", "$8Tqzabcdefghijkl"):
        idx = A.index_of(U_PW, cs)
        start = max(0, idx - 150)
        exp = O.Ctx(stream).search_range(cs, 5, start, 300, nthreads=NT)[0]
        assert exp == []
        with dprf.Context(O.split_stream(stream), device=0) as ctx:
            hits, n, st = ctx.search_range(cs, 5, start, 300)
            assert hits == [] and n == 0 and st["candidates"] == 300, (R, cs, hits)
            assert ctx.verify_list(_near(U_PW))[0] == []


# ---------------------------------------------------------------- C: the oracle against the reference executables
GOLDEN_CASES = ["office-hash", "office-verifier", "odt-checksum", "pdf-r2-user", "pdf-r3-40-user", "pdf-r3-128-user",
                "pdf-r4-user", "pdf-r4-nometa-user", "pdf-r5-user", "pdf-r6-user"]


def golden_entries():
    """(name, stream, password) of the streams whose reference verdict tests/golden/make_tamper.py records: per
    family every fourth byte position, both ends of the compared width and the first byte outside it; the Office
    hash_size gate streams; the ODF 2-byte and coverage streams."""
    out = []
    for case in CASES:
        if case.id not in GOLDEN_CASES:
            continue
        ks = set(range(0, case.n, 4)) | {0, max(case.miss), case.n - 1}
        if max(case.miss) + 1 < case.n:
            ks.add(max(case.miss) + 1)
        doc = case.doc("short")
        out += [("%s-%s" % (case.id, "base" if k is None else k), doc[k], case.pws["short"])
                for k in [None] + sorted(ks)]
    for hs in OFFICE_HASH_SIZES:
        out.append(("office-gate-%d" % hs, office_gate_stream(hs)[0], "Ux7"))
    out += [("odt-" + name, make(), "Lk9") for name, make, _ in ODT_EXTRA]
    out += [("pdf-r%d-gate-only" % R, gate_only_stream(R)[0], U_PW) for R in (2, 5)]
    return out


def test_oracle_agrees_with_the_reference_on_tampered_streams():
    gold = load_golden("tamper_verdicts.json")
    mine = {name: (stream, pw) for name, stream, pw in golden_entries()}
    assert sorted(gold) == sorted(mine)
    codes = collections.Counter()
    for name, e in gold.items():
        assert (e["stream"], e["password"]) == mine[name], name       # the fixture records part A's own streams
        assert O.Ctx(e["stream"]).verify(e["password"]) == e["code"], name
        codes[e["code"]] += 1
    assert set(codes) == {0, 1} and codes[0] > 40 and codes[1] > 20
