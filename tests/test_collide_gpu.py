"""The password search for a known 40-bit key on the device (dprf_ctx_set_key40: k_collide_pdf, k_collide_oldoffice)
against tests/key40_model.key_of_password, the Python statement of the key derivation, which tests/test_collide_model.py
and tests/test_key40_model.py tie to the oracle, the Office model and the public hashcat pairs on the CPU.  A candidate
verifies exactly when key_of_password(document, candidate) is the key that is set; expected hit sets always come from
the model over the same candidates.  The shapes are the smallest at which these kernels can go wrong.

  (a) the public and golden pairs in list mode, a neighbour on either side
  (b) range windows on all four families: odd starts, counts around a wave and a block, the key of the first, the last
      and of a candidate one outside; planted range lengths 1..32
  (c) message-shape edges in list mode: one / two hash blocks, a full slot, the PDF cut at 32 bytes
  (d) every lane and every seam of two full workgroups plus a partial one; a list of one password three workgroups long
  (e) the compare in the rejecting direction: the 40 keys one bit away
  (f) a full 2^16 window per family against the model, both directions
  (g) symbols, mask, hybrid, rules and list with a key set; stop_on_first; two lanes on one device
  (h) round trip: set the recorded key, find the recorded password, clear, and the document check is back
  (i) refusals, after each of which the context still serves; owner mode in both orders; a never-matching context
  (j) end to end from generated documents: --key40 FROM-TO, then --key with a mask, one run with --checkpoint"""
import contextlib
import functools
import io
import itertools
import json

import pytest

import doc_layer
import key40_model as km
from conftest import load_golden

pytestmark = pytest.mark.gpu

FAMILIES = ["pdf_r2", "pdf_r34", "office_md5", "office_sha1"]
NAMES = {"pdf_r2": ("pdf_r24", "pdf_r24_collide"), "pdf_r34": ("pdf_r24", "pdf_r24_collide"),
         "office_md5": ("office_rc4_md5", "office_rc4_md5_collide"),
         "office_sha1": ("office_rc4_sha1", "office_rc4_sha1_collide")}
# candidates per workgroup: 256 threads x the candidates per thread of the family's kernel (dprf_kernels.hip
# COLLIDE_R2_PER 8, COLLIDE_R3_PER 2; dprf_kernels_oldoffice.hip COLLIDE_OO_PER 4)
WG = {"pdf_r2": 256 * 8, "pdf_r34": 256 * 2, "office_md5": 256 * 4, "office_sha1": 256 * 4}
LOWER = "abcdefghijklmnopqrstuvwxyz"


@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _doc(fam):
    return tuple(km.base_documents()[fam])


def _word(index, n, charset=LOWER):
    """Candidate `index` of charset^n in itertools.product order: the leftmost character is the most significant."""
    out = []
    for _ in range(n):
        index, r = divmod(index, len(charset))
        out.append(charset[r])
    return "".join(reversed(out))


def _key(fam_or_fields, pw):
    fields = _doc(fam_or_fields) if isinstance(fam_or_fields, str) else fam_or_fields
    return km.key_of_password(list(fields), pw)


def _key_of_raw(fields, raw):
    """The model's key of a candidate given as the bytes the device verifies: UTF-16LE for Office, else the bytes."""
    if fields[0] == "oldoffice":
        return km.key_of_password(list(fields), raw.decode("utf-16-le", "surrogatepass"))
    return km.key_of_password(list(fields), raw.decode("utf-8"))


@functools.lru_cache(maxsize=None)
def _window_keys(fam, n, start, count):
    return tuple(_key(fam, _word(i, n)) for i in range(start, start + count))


def _collider(dprf, fam, key=None):
    ctx = dprf.Context(list(_doc(fam)), device=0, key40=key)
    return ctx


# ---------------------------------------------------------------- (a)
def _pairs():
    vec = load_golden("collide_vectors.json")
    streams = load_golden("streams.json")
    out = [(n, streams[n]["stream"], e["key"], e["password"]) for n, e in sorted(vec["streams"].items())]
    out += [(n, e["stream"], e["key"], e["password"]) for n, e in sorted(vec["public"].items())]
    return out


@pytest.mark.parametrize("name", [c[0] for c in _pairs()])
def test_a_public_and_golden_pairs(dprf, name):
    _, stream, key, pw = [c for c in _pairs() if c[0] == name][0]
    fields = km.fields_of(stream)
    assert km.key_of_password(fields, pw).hex() == key
    below, above = pw[:-1], pw[:-1] + chr(ord(pw[-1]) + 1)          # hashca, hashcat, hashcau
    with dprf.Context(fields, device=0, key40=key) as ctx:
        assert ctx.key40() == bytes.fromhex(key)
        hits, n, st = ctx.verify_list([below, pw, above])
        assert (hits, n, st["candidates"]) == ([1], 1, 3)
        ctx.set_key40(bytes.fromhex(key))                            # bytes as well as hex digits
        assert ctx.verify_list([above, below, pw, pw])[0] == [2, 3]


# ---------------------------------------------------------------- (b)
@pytest.mark.parametrize("fam", FAMILIES)
def test_b_range_window_edges(dprf, fam):
    n, start = 6, 0x0a7f12c5 % 26 ** 6 | 1                         # no multiple of anything
    with _collider(dprf, fam) as ctx:
        assert ctx.kernel == NAMES[fam][0] and ctx.key40() is None
        for count in (1, 63, 65, 257, 513):
            keys = _window_keys(fam, n, start - 1, 515 + 1)          # index start - 1 .. start + 514
            for idx in sorted({start, start + count - 1}):
                ctx.set_key40(keys[idx - start + 1])
                assert ctx.kernel == NAMES[fam][1]
                hits, nh, st = ctx.search_range(LOWER, n, start, count)
                assert (hits, nh, st["candidates"]) == ([idx], 1, count), (count, idx)
            # the key of the candidate one below and one above the window: no hit
            for outside in (start - 1, start + count):
                ctx.set_key40(keys[outside - start + 1])
                assert ctx.search_range(LOWER, n, start, count)[0] == [], (count, outside)


@pytest.mark.parametrize("fam", FAMILIES)
def test_b_planted_lengths_1_to_32(dprf, fam):
    """One search per range length: PDF bytes, Office UTF-16 units.  Lengths 28 and up are two MD5 blocks for types
    0 / 1, 20 and up two SHA-1 blocks for type 3; 32 fills the PDF's padded password and the Office slot."""
    with _collider(dprf, fam) as ctx:
        for n in range(1, 33):
            space = 26 ** n
            start = 3 if n == 1 else (0x9e3779b97f4a7c15 % (space - 70) if space < 1 << 62 else 0x1e3779b97f4a7c15)
            count = 20 if n == 1 else 65
            idx = start + (7 * n) % count
            ctx.set_key40(_key(fam, _word(idx, n)))
            hits, nh, st = ctx.search_range(LOWER, n, start, count)
            assert (hits, nh, st["candidates"]) == ([idx], 1, count), n


# ---------------------------------------------------------------- (c)
def _of_length(n, salt):
    return "".join(LOWER[(salt + 5 * k) % 26] for k in range(n))


@pytest.mark.parametrize("fam,lengths", [("office_md5", (26, 27, 28, 29, 31, 32)),
                                         ("office_sha1", (18, 19, 20, 21, 31, 32))])
def test_c_office_message_shape_edges(dprf, fam, lengths):
    """Types 0 / 1: MD5(pw16) is one block up to 27 units and two from 28; type 3: SHA1(salt || pw16) is one block up
    to 19 units and two from 20; 32 units fill the slot (the terminator moves to the next word).  Planted on both sides
    of each edge; 33 units are refused as in the password search."""
    pws = [_of_length(n, n) for n in lengths]
    with _collider(dprf, fam) as ctx:
        for k, pw in enumerate(pws):
            ctx.set_key40(_key(fam, pw))
            hits, nh, st = ctx.verify_list(pws)
            assert (hits, nh, st["candidates"]) == ([k], 1, len(pws)), len(pw)
        with pytest.raises(dprf.DprfError) as ei:
            ctx.verify_list(pws + [_of_length(33, 1)])
        assert ei.value.code == dprf.E_PWLEN
        assert ctx.verify_list(pws)[0] == [len(pws) - 1]            # the context still serves, the key is kept


@pytest.mark.parametrize("fam", ["pdf_r2", "pdf_r34"])
def test_c_pdf_cut_at_32_bytes(dprf, fam):
    """31 bytes take one byte of PAD, 32 none, and a longer candidate is cut at 32: two candidates sharing 32 leading
    bytes both verify, as in the password search."""
    p32 = _of_length(32, 3)
    pws = [p32[:30], p32[:31], p32, p32 + "tail-of-8", p32[:31] + "#", p32 + "x" * 8, "q" * 40]
    assert len(pws[3]) == 41 and len(pws[5]) == 40
    with _collider(dprf, fam) as ctx:
        for k, want in ((0, [0]), (1, [1]), (2, [2, 3, 5]), (4, [4]), (6, [6])):
            ctx.set_key40(_key(fam, pws[k]))
            hits, nh, st = ctx.verify_list(pws)
            assert (hits, nh, st["candidates"]) == (want, len(want), len(pws)), k
        assert _key(fam, pws[3]) == _key(fam, p32) == _key(fam, pws[5])   # the model cuts alike


# ---------------------------------------------------------------- (d)
@pytest.mark.parametrize("fam", FAMILIES)
def test_d_every_lane_and_seam(dprf, fam):
    wg = WG[fam]
    n, start, count = 7, 0x5100123 | 1, 2 * wg + 37                 # two full workgroups and a partial one
    # every index of the first 130, and each index at and either side of every wave (64) boundary -- the 256-thread
    # strides and the workgroup boundaries are among them -- and the window's last
    offsets = set(range(130)) | {count - 1}
    for b in range(64, count, 64):
        offsets |= {b - 1, b, b + 1}
    offsets = sorted(o for o in offsets if o < count)
    keys = _window_keys(fam, n, start, count + 1)
    with _collider(dprf, fam) as ctx:
        for off in offsets:
            ctx.set_key40(keys[off])
            hits, nh, st = ctx.search_range(LOWER, n, start, count)
            assert (hits, nh, st["candidates"]) == ([start + off], 1, count), off
        ctx.set_key40(keys[count])                                  # the first candidate past the partial workgroup
        assert ctx.search_range(LOWER, n, start, count)[0] == []


@pytest.mark.parametrize("fam", FAMILIES)
def test_d_a_list_of_one_password_returns_every_index(dprf, fam):
    count = 3 * WG[fam] + 1
    with _collider(dprf, fam, _key(fam, "Ux7")) as ctx:
        hits, nh, st = ctx.verify_list(["Ux7"] * count, cap=count)
        assert hits == list(range(count)) and nh == count and st["candidates"] == count
        hits, nh, _ = ctx.verify_list(["Ux8"] * count, cap=count)
        assert (hits, nh) == ([], 0)


# ---------------------------------------------------------------- (e)
@pytest.mark.parametrize("fam", FAMILIES)
def test_e_keys_one_bit_away_reject(dprf, fam):
    n, start, count = 5, 0x31d05 | 1, 300
    idx = start + 211
    key = _key(fam, _word(idx, n))
    with _collider(dprf, fam, key) as ctx:
        assert ctx.search_range(LOWER, n, start, count)[0] == [idx]
        for bit in range(40):
            bad = bytearray(key)
            bad[bit // 8] ^= 1 << (bit % 8)
            ctx.set_key40(bytes(bad))
            hits, nh, st = ctx.search_range(LOWER, n, start, count)
            assert (hits, nh, st["candidates"]) == ([], 0, count), bit
        assert ctx.verify_list([_word(idx, n)])[0] == []            # list mode compares the same 40 bits
        ctx.set_key40(key)
        assert ctx.verify_list([_word(idx, n)])[0] == [0]


# ---------------------------------------------------------------- (f)
@pytest.mark.parametrize("fam", FAMILIES)
def test_f_a_full_window_against_the_model(dprf, fam):
    """2^16 candidates: the device's hit set equals the model's, in both directions, for the key of a candidate inside
    and for the key of one outside."""
    n, start, count = 7, 0x2b00f11 | 1, 1 << 16
    keys = _window_keys(fam, n, start, count + 1)
    with _collider(dprf, fam) as ctx:
        for k in (keys[40961], keys[count]):
            want = [start + i for i in range(count) if keys[i] == k]
            ctx.set_key40(k)
            hits, nh, st = ctx.search_range(LOWER, n, start, count)
            assert hits == want and nh == len(want) and st["candidates"] == count
        assert [start + i for i in range(count) if keys[i] == keys[40961]] == [start + 40961]


# ---------------------------------------------------------------- (g)
def _hits_of(fields, candidates, key, base=0):
    return [base + i for i, raw in enumerate(candidates) if _key_of_raw(fields, raw) == key]


def _enc(fields, text):
    return text.encode("utf-16-le") if fields[0] == "oldoffice" else text.encode("utf-8")


@pytest.mark.parametrize("fam", FAMILIES)
def test_g_every_mode_with_a_key_set(dprf, fam):
    from dprf_amd import hybrid, mask, rules
    fields = list(_doc(fam))
    count = 1 << 12
    with dprf.Context(fields, devices=[0, 0]) as two, dprf.Context(fields, device=0) as ctx:
        # symbols with a 2-byte character: 4^7 candidates, a window of 2^12 at an odd start
        charset, n, start = "aézQ", 7, 4099
        cands = [_enc(fields, _word(i, n, charset)) for i in range(start, start + count)]
        key = _key_of_raw(fields, cands[1234])
        want = _hits_of(fields, cands, key, start)
        ctx.set_key40(key)
        assert ctx.search_symbols(charset, n, start, count)[0] == want == [start + 1234]

        # mask: ?l?d?u?l, 67,600 candidates
        positions = mask.parse_mask("?l?d?u?l")
        start = 31337
        cands = [_enc(fields, mask.word(positions, i)) for i in range(start, start + count)]
        key = _key_of_raw(fields, cands[count - 1])
        ctx.set_key40(key)
        hits, nh, st = ctx.search_mask(positions, start, count)
        assert (hits, nh, st["candidates"]) == (_hits_of(fields, cands, key, start), 1, count)
        assert hits == [start + count - 1]

        # hybrid: words x ?d?d, a word listed twice so that two candidates verify
        words = [b"alpha", b"Bravo7", b"charlie", b"alpha"] + [("w%03d" % k).encode() for k in range(508)]
        positions, word_at = hybrid.parse_hybrid("?w?d?d")
        cands = [_enc(fields, hybrid.candidate(words, positions, word_at, i).decode()) for i in range(count)]
        key = _key_of_raw(fields, cands[37])                        # alpha37: words 0 and 3
        want = _hits_of(fields, cands, key)
        assert want == [37, 337]
        for c in (ctx, two):
            c.set_words(words)
            c.set_key40(key)
            hits, nh, st = c.search_hybrid(positions, word_at, 0, count)
            assert (hits, nh, st["candidates"]) == (want, 2, count)
            assert c.search_hybrid(positions, word_at, 0, count, stop_on_first=True, cap=1)[0] == [37]
            assert c.search_hybrid(positions, word_at, 38, count - 38, stop_on_first=True, cap=1)[0] == [337]
        assert two.last_call_devices()[0]["launches"] >= 1 and len(two.last_call_devices()) == 2

        # rules: the candidate bytes are the device's own spelling (spell_rules is unaffected by the key)
        table = [rules.parse_rule(r) for r in (":", "u", "c", "$1", "^x", "r", "d", "sa4")]
        nrule = len(table)
        total = len(words) * nrule                                  # 2^12
        cands = ctx.spell_rules(table, 0, total)
        assert cands[1 * nrule + 1] == _enc(fields, "BRAVO7")
        key = _key_of_raw(fields, cands[0 * nrule + 2])             # "Alpha": words 0 and 3 under "c"
        want = _hits_of(fields, cands, key)
        assert want == [2, 3 * nrule + 2]
        for c in (ctx, two):
            c.set_key40(key)
            hits, nh, st = c.search_rules(table, 0, total)
            assert (hits, nh, st["candidates"]) == (want, 2, total)
            assert c.search_rules(table, 0, total, stop_on_first=True, cap=1)[0] == [2]
        assert ctx.spell_rules(table, 0, total) == cands

        # list: 2^12 passwords, three of them alike
        pws = [_word(7919 * i, 6) for i in range(count)]
        pws[17] = pws[2222] = pws[count - 1] = "Ux7"
        for c in (ctx, two):
            c.set_key40(_key(fam, "Ux7"))
            hits, nh, st = c.verify_list(pws)
            assert (hits, nh, st["candidates"]) == ([17, 2222, count - 1], 3, count)
            assert c.verify_list(pws, stop_on_first=True, cap=1)[0] == [17]
        lanes = two.last_call_devices()
        assert len(lanes) == 2


# ---------------------------------------------------------------- (h)
@pytest.mark.parametrize("name", [c[0] for c in _pairs()])
def test_h_round_trip(dprf, name):
    _, stream, key, pw = [c for c in _pairs() if c[0] == name][0]
    fields = km.fields_of(stream)
    family = NAMES[km.family(fields)]
    idx = km.key_index(key)
    others = [pw[:-1], pw + "x", "Ux7"]
    with dprf.Context(fields, device=0) as fresh, dprf.Context(fields, device=0) as ctx:
        assert ctx.kernel == family[0]
        before = ctx.search_range(LOWER, 3, 100, 3000)[:2]
        ctx.set_key40(key)
        assert ctx.kernel == family[1] and ctx.key40().hex() == key
        assert ctx.verify_list(others + [pw])[0] == [3]
        assert ctx.search_key40(idx - 50, 100)[0] == [idx]          # the key search is unaffected by the selection
        ctx.set_key40(None)
        assert ctx.kernel == family[0] and ctx.key40() is None
        assert ctx.verify_list(others + [pw])[0] == [3]             # the document check again: the password verifies
        assert ctx.search_key40(idx - 50, 100)[0] == [idx]
        assert ctx.search_range(LOWER, 3, 100, 3000)[:2] == before == fresh.search_range(LOWER, 3, 100, 3000)[:2]
    # with a wrong key set the document's password does not verify: the check really is the key's
    wrong = "%010x" % (idx ^ 1)
    with dprf.Context(fields, device=0, key40=wrong) as ctx:
        assert ctx.verify_list([pw])[0] == []
        ctx.set_key40(None)
        assert ctx.verify_list([pw])[0] == [0]


# ---------------------------------------------------------------- (i)
@pytest.mark.parametrize("label", ["pdf_r3_128", "pdf_r4_meta0", "pdf_r5", "pdf_r6", "oldoffice_4", "office_2007",
                                   "agile_2010", "agile_2013", "odt", "odf"])
def test_i_refused_documents_still_serve(dprf, label):
    fields, pw, family, _ = doc_layer.case(label)
    with pytest.raises(dprf.DprfError) as ei:
        dprf.Context(fields, device=0, key40="0102030405")
    assert ei.value.code == dprf.E_DOMAIN
    with dprf.Context(fields, device=0) as ctx:
        with pytest.raises(dprf.DprfError) as ei:
            ctx.set_key40("0102030405")
        assert ei.value.code == dprf.E_DOMAIN and "not a 40-bit document" in str(ei.value)
        assert ctx.kernel == family and ctx.key40() is None
        ctx.set_key40(None)                                         # clearing is never refused
        assert ctx.verify_list(["no", pw, "nope"])[0] == [1]


@pytest.mark.parametrize("fam", ["pdf_r2", "pdf_r34"])
def test_i_owner_mode_and_a_key_exclude_each_other(dprf, fam):
    key = _key(fam, "Ux7")
    with _collider(dprf, fam) as ctx:
        ctx.set_pdf_password("owner")
        with pytest.raises(dprf.DprfError) as ei:
            ctx.set_key40(key)
        assert ei.value.code == dprf.E_INVALID and "owner" in str(ei.value)
        assert ctx.kernel == "pdf_r24_owner" and ctx.key40() is None and ctx.pdf_password == "owner"
        ctx.set_pdf_password("user")
        ctx.set_key40(key)
        with pytest.raises(dprf.DprfError) as ei:
            ctx.set_pdf_password("owner")
        assert ei.value.code == dprf.E_INVALID and "key" in str(ei.value)
        assert ctx.kernel == "pdf_r24_collide" and ctx.key40() == key and ctx.pdf_password == "user"
        assert ctx.verify_list(["no", "Ux7"])[0] == [1]
        ctx.set_pdf_password("user")                                # selecting the user password again is fine
        assert ctx.verify_list(["no", "Ux7"])[0] == [1]
    with pytest.raises(dprf.DprfError) as ei:
        dprf.Context(list(_doc(fam)), device=0, pdf_password="owner", key40=key)
    assert ei.value.code == dprf.E_INVALID


def test_i_never_matching_context_accepts_a_key_and_launches_nothing(dprf):
    fields = list(_doc("pdf_r2"))
    fields[2] = "3"                                                 # V 1 with R 3: the reference's verdict is constant
    with dprf.Context(fields, device=0) as ctx:
        assert ctx.flags & dprf.FLAG_NEVER_MATCHES
        ctx.set_key40(_key("pdf_r2", "Ux7"))
        assert ctx.kernel == "none" and ctx.key40() is not None
        hits, nh, st = ctx.search_range(LOWER, 4, 0, 26 ** 4)
        assert (hits, nh) == ([], 0) and st["launches"] == 0 and st["candidates"] == 26 ** 4
        assert ctx.verify_list(["Ux7"])[0] == []


# ---------------------------------------------------------------- (j)
def _write(kind, path):
    import docgen
    import oldoffice_docgen
    pw = "Ux7"
    if kind == "pdf_r2":
        docgen.write_pdf(path, pw, seed=412, R=2, length=40)
        return "3", pw
    if kind == "pdf_r3_40":
        docgen.write_pdf(path, pw, seed=413, R=3, length=40)
        return "3", pw
    if kind == "doc_type1":
        oldoffice_docgen.write_doc(path, pw, 1, seed=411)
        return "1", pw
    oldoffice_docgen.write_xls(path, pw, 3, seed=414)
    return "1", pw


def _cli(argv):
    from dprf_amd import brute_force
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ret = brute_force.main(argv)
    return ret, out.getvalue()


def _document(kind, tmp_path):
    from dprf_amd import brute_force
    path = str(tmp_path / {"pdf_r2": "a.pdf", "pdf_r3_40": "b.pdf", "doc_type1": "c.doc", "xls_type3": "d.xls"}[kind])
    doc_type, pw = _write(kind, path)
    with contextlib.redirect_stdout(io.StringIO()):
        fields = list(brute_force.parse_verification_data(brute_force.get_verification_data(doc_type, path)))
    idx = km.key_index(km.key_of_password(fields, pw))
    lo = min(max(0, idx - 2048), km.SPACE - 4096)
    return doc_type, path, fields, pw, "%010x-%010x" % (lo, lo + 4095)


@pytest.mark.parametrize("kind", ["pdf_r2", "pdf_r3_40", "doc_type1", "xls_type3"])
def test_j_key_search_then_password_for_the_key(dprf, kind, tmp_path):
    doc_type, path, fields, pw, window = _document(kind, tmp_path)
    (found, key), text = _cli([doc_type, path, "--key40", window, "--devices", "0"])
    assert found == 1 and "--key %s" % key in text                  # the hint names the flag and the key
    (found, got), text = _cli([doc_type, path, "--key", key, "--mask", "?u?l?d", "--devices", "0"])
    assert found == 1 and "Correct password is '%s'" % got in text
    assert "not necessarily" in text and key in text
    assert km.key_of_password(fields, got).hex() == key
    # the plain password mode accepts what the collider printed
    with dprf.Context(fields, device=0) as ctx:
        assert ctx.verify_list(["nope", got])[0] == [1]
    assert got == pw                                                # 6,760 candidates: a second preimage is not expected
    # a mask that cannot spell it finds nothing, and says nothing of a key
    (found, _), text = _cli([doc_type, path, "--key", key, "--mask", "?d?d?d", "--devices", "0"])
    assert found == 0 and "not necessarily" not in text


def test_j_range_and_checkpoint(tmp_path, monkeypatch):
    from dprf_amd import brute_force
    doc_type, path, fields, pw, _ = _document("doc_type1", tmp_path)
    key = km.key_of_password(fields, pw).hex()
    cursor = str(tmp_path / "cursor.json")
    charset = "7xUa"
    argv = [doc_type, path, "--key", key, "-pr", "3", "--charset", charset, "--devices", "0", "--checkpoint", cursor]
    # rounds of 16 candidates until a rate is known; the run is interrupted after its first round ("Ux7" is index 36)
    monkeypatch.setattr(brute_force, "FIRST_ROUND", 16)

    def stop(*a):
        raise KeyboardInterrupt
    monkeypatch.setattr(brute_force, "progress", stop)
    with pytest.raises(SystemExit) as ei:
        _cli(argv)
    assert ei.value.code == 0
    rec = json.load(open(cursor))
    assert rec["target"] == "key40:" + key and rec["next_index"] == 16 and rec["found"] is None
    monkeypatch.undo()
    ret, text = _cli(argv)
    assert ret == (1, pw) and "resuming at index 16" in text and "not necessarily" in text
    ret, text = _cli(argv)                                          # answered from the finished checkpoint
    assert ret == (1, pw) and "already finished" in text
    # the same file without the key, or under another key, is refused
    for other in (argv[:2] + argv[4:], argv[:3] + ["%010x" % (int(key, 16) ^ 1)] + argv[4:]):
        with pytest.raises(ValueError, match="different search"):
            _cli(other)
    assert list(itertools.product(charset, repeat=3))[36] == tuple(pw)
