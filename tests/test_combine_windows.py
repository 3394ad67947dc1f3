"""Device-spelled combinator windows (dprf_search_combine: k_spell_combine + the list kernels) against the oracle: the
hit set of a whole window equals the set pyoracle (or the family's model) finds over the same window spelled by this
file's own speller (divmod by N2, the two words concatenated; the oracle does its own UTF-16LE conversion and
truncation), on one, two and four device lanes, with stop_on_first returning the oracle's lowest.

  (a) a PDF R5 window of 2^16 against list mode over the host-spelled window (a self-comparison)
  (b) ODF `-e` (2-byte check): false positives besides the planted password
  (c) PDF R5 (one SHA-256 per candidate), one planted document per case, windows of at most 1024: the password at
      R = N2 - 1 and at R = 0, the two sides of a wrap inside one block, for N2 = 1, 255, 256, 257 and 600; the
      keyspace's last candidate; count = 1; a window across 2^32; a chunk start with r0 != 0
  (d) PDF R4: the 32-byte cut inside either word and between them
  (e) Office 2007: a whole small keyspace
  (f) PDF R2 and R6: mixed-width windows of 2^12 whose start is no multiple of 64
  (g) Office Agile (both hashes), Office 97-2003, ODF 1.0 / 1.1, owner mode (PDF R3) and a set key40, each against
      its model
  (h) the right table's life cycle, (i) the refusals, (j) a never-matching context, (k) the CLI end to end

Every oracle case has a CPU test of its preconditions on the oracle or the model alone, so no GPU comparison passes
vacuously.  Word tables come from fixed seeds; the expected set is computed once per case and shared."""
import functools
import json

import pytest

import test_hybrid_windows as hw
from test_hybrid_windows import table
from test_mask_windows import DEVICE_LISTS, DIGITS, LOWER, R2, R4, R5, R6, SEED, _fields, _stream_of

ORACLE_THREADS = 16
R3 = {"R": 3, "length": 128}
WIDE = hw.ALPHA + "\U0001D11E"

WORDS = hw.WORDS                                           # > 2500 distinct words of 3..12 characters, at most 36 bytes
NW = len(WORDS)
RT = {n: hw.distinct(table(2 * n + 8, 0xC200 + n, 1, 4))[:n] for n in (1, 255, 256, 257, 600)}   # distinct right words
MIXED = hw.distinct(table(90, 0xC2F0, 1, 3, "ab\u00e9\u00df\u20ac\u03b1\U0001D11E\U00020000xyz"))[:60]   # (f): 1-4 byte characters
ODF_LEFT = hw.ODF_WORDS                                    # (b): 6000 words x "-00" .. "-99": hybrid mode's candidates
ODF_RIGHT = [b"-%02d" % d for d in range(100)]
BIG_LEFT = [b"w%x" % k for k in range((1 << 17) + 3)]      # (c): N1 * N2 = 2^34 and a bit; "-" makes the split unique
BIG_RIGHT = [b"-%x" % k for k in range((1 << 17) + 5)]
NB = len(BIG_RIGHT)
CUT_LEFT = [b"a" * 31, ("x" * 30 + "€").encode(), b"b", ("x" * 30 + "₭").encode(), b"c" * 32, b"d" * 30, b"z" * 70]
CUT_RIGHT = [b"1", "€1".encode(), "₭2".encode(), b"q" * 64, "é".encode()]
OFFICE_LEFT = ["a€".encode(), "é\U0001D11E".encode(), "P\U00020000b".encode(), b"zz"]
OFFICE_RIGHT = [b"7", "€x".encode(), "\U0001D11E".encode(), "ß9".encode(), b"-"]
SMALL_LEFT = OFFICE_LEFT + [b"summer", b"Anna"]
SMALL_RIGHT = OFFICE_RIGHT + [b"2024", b"Maria"]
DUP_LEFT = [b"moon", b"su", b"sun", b"star", b"sun"]       # key40: "sun7" is spelled five times over
DUP_RIGHT = [b"7", b"x", b"n7", b"7"]


def spell(left, right, i):
    """Left word i // N2 followed by right word i % N2."""
    l, r = divmod(i, len(right))
    return left[l] + right[r]


def _case(kind, kw, left, right, idx, start, count, **more):
    return dict({"kind": kind, "kw": kw, "left": left, "right": right, "idx": idx, "start": start, "count": count},
                **more)


def _r5(left, right, idx, start, count):
    return _case("pdf", R5, left, right, idx, start, count)


def _wrap(n2, w, first):
    """Planted at the last right word of left word w or at the first of w + 1; the window starts 300 below the seam,
    so the seam and both plants lie inside the second block of 256."""
    seam = (w + 1) * n2
    return _r5(WORDS, RT[n2], seam if first else seam - 1, seam - 300, 1000)


CASES = {
    "b-odf-e-false-positives": _case("odt_e", {}, ODF_LEFT, ODF_RIGHT, hw.ODF_PW_IDX, hw.ODF_WINDOW[0],
                                     hw.ODF_WINDOW[1], planted_outside=True),
    "b-odf-e-planted": _case("odt_e", {}, ODF_LEFT, ODF_RIGHT, hw.ODF_PW_IDX, hw.ODF_PW_IDX - 20001, 1 << 15),
    "c-n1": _r5(WORDS, RT[1], 1255, 1000, 1000),
    "c-n255-last": _wrap(255, 7, False),
    "c-n255-first": _wrap(255, 7, True),
    "c-n256-last": _wrap(256, 9, False),
    "c-n256-first": _wrap(256, 9, True),
    "c-n257-last": _wrap(257, 11, False),
    "c-n257-first": _wrap(257, 11, True),
    "c-n600-last": _wrap(600, 13, False),
    "c-n600-first": _wrap(600, 13, True),
    "c-keyspace-last": _r5(WORDS, RT[600], NW * 600 - 1, NW * 600 - 777, 777),
    "c-count-1": _r5(WORDS, RT[257], 257 * 16 + 130, 257 * 16 + 130, 1),
    "c-across-2^32": _r5(BIG_LEFT, BIG_RIGHT, (1 << 32) + 5, (1 << 32) - 100, 1000),
    "c-r0-nonzero": _r5(WORDS, RT[600], 600 * 5 + 123 + 700, 600 * 5 + 123, 1000),
    "d-r4-cut": _case("pdf", R4, CUT_LEFT, CUT_RIGHT, 1 * 5 + 0, 0, 35),
    "e-office": _case("docx", {}, OFFICE_LEFT, OFFICE_RIGHT, 2 * 5 + 3, 0, 20),
    "f-pdf-r2": _case("pdf", R2, WORDS, MIXED, 60 * 700 + 31, 60 * 700 - 2001, 1 << 12),
    "f-pdf-r6": _case("pdf", R6, WORDS, MIXED, 60 * 900 + 59, 60 * 900 - 3003, 1 << 12),
    "g-owner-r3": _case("pdf", R3, WORDS, RT[257], 257 * 150 + 7, 257 * 150 - 1001, 1 << 11, owner=True),
}
B_CASES = [k for k in CASES if k.startswith("b-")]
C_CASES = [k for k in CASES if k.startswith("c-")]
F_CASES = [k for k in CASES if k.startswith("f-")]


def _password(name):
    c = CASES[name]
    return spell(c["left"], c["right"], c["idx"]).decode()


def _window(c):
    return [spell(c["left"], c["right"], i) for i in range(c["start"], c["start"] + c["count"])]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(stream, the oracle's sorted hit indices of the case's window): once per case, for every test that needs it."""
    import pyoracle
    c = CASES[name]
    kw = dict(c["kw"], owner=_password(name)) if c.get("owner") else c["kw"]
    pw = "user" if c.get("owner") else _password(name)
    stream = _stream_of(c["kind"], tuple(sorted(kw.items())), pw)
    window = _window(c)
    if c.get("owner"):
        import owner_model
        return stream, [c["start"] + k for k, w in enumerate(window) if owner_model.owner_verifies(stream, w)]
    verdicts = pyoracle.Ctx(stream).verify_list(window, nthreads=ORACLE_THREADS)
    return stream, [c["start"] + k for k, v in enumerate(verdicts) if v]


def _spelled_like_the_password(name):
    c = CASES[name]
    pw = spell(c["left"], c["right"], c["idx"])
    return [c["start"] + k for k, w in enumerate(_window(c)) if w == pw]


def _search_equals(fields, left, right, start, count, want, what, **ctx_kw):
    """The window on every device list: all hits, the candidate count, and stop_on_first's lowest."""
    from dprf_amd import _lib
    assert want, what                                                       # never a vacuous comparison
    for devs in DEVICE_LISTS:
        with _lib.Context(fields, devices=devs, **ctx_kw) as ctx:
            ctx.set_words(left)
            ctx.set_right_words(right)
            assert (ctx.words, ctx.right_words) == (len(left), len(right))
            hits, nh, st = ctx.search_combine(start, count)
            assert hits == want and nh == len(want), (what, devs, hits[:8], want[:8], nh, len(want))
            assert st["candidates"] == count and st["devices"] == len(devs), (what, devs, st)
            recs = ctx.last_call_devices()
            assert len(recs) == len(devs) and sum(r["candidates"] for r in recs) == count, (what, devs, recs)
            first, _, _ = ctx.search_combine(start, count, stop_on_first=True, cap=1)
            assert first == want[:1], (what, devs, first, want[:1])


def _gpu_equals_oracle(name):
    c = CASES[name]
    stream, want = expected(name)
    _search_equals(_fields(stream), c["left"], c["right"], c["start"], c["count"], want, name,
                   pdf_password="owner" if c.get("owner") else "user")


def test_cases_lie_inside_their_keyspaces():
    for name, c in CASES.items():
        n = len(c["left"]) * len(c["right"])
        assert 0 <= c["start"] and c["start"] + c["count"] <= n, name
        assert c.get("planted_outside") or c["start"] <= c["idx"] < c["start"] + c["count"], name
        assert c["count"] <= (1024 if name in C_CASES else 1 << 15), name
    assert NW >= 2500 and all(len(RT[n]) == n == len(set(RT[n])) for n in RT) and len(MIXED) == 60
    for n2 in (255, 256, 257, 600):
        last, first = CASES["c-n%d-last" % n2], CASES["c-n%d-first" % n2]
        assert last["idx"] % n2 == n2 - 1 and first["idx"] % n2 == 0 and first["idx"] == last["idx"] + 1
        assert last["start"] == first["start"] and last["start"] % n2                     # r0 != 0
        assert (last["idx"] - last["start"]) // 256 == (first["idx"] - first["start"]) // 256 == 1   # one block
    assert len(RT[1]) == 1 and CASES["c-n1"]["idx"] - CASES["c-n1"]["start"] == 255
    assert CASES["c-keyspace-last"]["idx"] == NW * 600 - 1 and CASES["c-count-1"]["count"] == 1
    c = CASES["c-across-2^32"]
    assert c["start"] < 1 << 32 < c["idx"] < c["start"] + c["count"] and len(BIG_LEFT) * NB > 1 << 34
    assert (1 << 17) <= len(BIG_LEFT) and (1 << 17) <= NB and c["start"] % NB
    assert CASES["c-r0-nonzero"]["start"] % 600 == 123 and CASES["c-r0-nonzero"]["start"] % 64
    for name in F_CASES:
        assert CASES[name]["start"] % 64 and CASES[name]["count"] == 1 << 12, name
    assert {len(ch.encode()) for w in MIXED for ch in w.decode()} == {1, 2, 3, 4}
    assert ODF_LEFT is hw.ODF_WORDS and all(hw.spell(ODF_LEFT, hw.ODF_POS, 0, i) == spell(ODF_LEFT, ODF_RIGHT, i)
                                            for i in (0, 99, 100, hw.ODF_PW_IDX, 599999))
    assert [len(ch.encode("utf-16-le")) for ch in _password("e-office")] == [2, 4, 2, 2, 2]


# ------------------------------------------------------------------ (a) self-comparison
@pytest.mark.gpu
def test_combine_window_equals_list_mode_of_the_spelled_window():
    from dprf_amd import _lib
    left, right = WORDS, RT[257]
    start, count = 257 * 1111 + 17, 1 << 16
    idx = start + 40000
    stream = _stream_of("pdf", tuple(sorted(R5.items())), spell(left, right, idx).decode())
    window = [spell(left, right, i) for i in range(start, start + count)]
    same = [start + k for k, w in enumerate(window) if w == window[40000]]
    for devs in DEVICE_LISTS:
        with _lib.Context(_fields(stream), devices=devs) as ctx:
            ctx.set_words(left)
            ctx.set_right_words(right)
            a = ctx.search_combine(start, count)
            b = ctx.verify_list(window)
            assert a[0] == [start + h for h in b[0]] == same and idx in same and a[1] == b[1], (devs, a[:2], b[:2])
            assert a[2]["candidates"] == b[2]["candidates"] == count
            assert ctx.search_combine(start, count, stop_on_first=True, cap=1)[0] == same[:1]


# ------------------------------------------------------------------ (b) ODF -e: false positives
def test_odf_e_windows_on_the_oracle():
    lo, n = hw.ODF_WINDOW
    want = [h for h in hw.ODF_ALL if lo <= h < lo + n]
    assert want == [465380, 476425, 491283] and hw.ODF_PW_IDX not in want
    assert expected("b-odf-e-false-positives")[1] == want and lo % 100 and lo % 64
    assert expected("b-odf-e-planted")[1] == [hw.ODF_PW_IDX, 432447]


@pytest.mark.gpu
@pytest.mark.parametrize("name", B_CASES)
def test_odf_e_window_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ (c) PDF R5: one document per edge
@pytest.mark.parametrize("name", C_CASES)
def test_pdf_r5_plant_is_what_the_oracle_finds(name):
    """The oracle's hits are exactly the indices that spell the planted password (one, unless two pairs concatenate to
    the same bytes), the planted index among them."""
    want = expected(name)[1]
    assert want == _spelled_like_the_password(name) and CASES[name]["idx"] in want and len(want) <= 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", C_CASES)
def test_pdf_r5_planted_edge_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ (d) PDF R4: the 32-byte cut
def test_pdf_r4_cut_on_the_oracle():
    """The password is x * 30 + € + 1, of which R4 hashes x * 30 E2 82: so does every pair whose first 32 bytes are
    those -- left words 1 and 3 with any right word -- and nothing else."""
    want = expected("d-r4-cut")[1]
    assert want == list(range(5, 10)) + list(range(15, 20))
    c = CASES["d-r4-cut"]
    assert {spell(c["left"], c["right"], i)[:32] for i in want} == {b"x" * 30 + b"\xe2\x82"}
    cut = [spell(c["left"], c["right"], i) for i in range(c["count"])]
    assert any(len(w) > 64 for w in cut) and max(len(w) for w in c["left"] + c["right"]) > 64
    # the cut inside the left word, exactly between the words, and inside a character of the right word
    assert len(c["left"][1]) == 33 and len(c["left"][4]) == 32 and len(c["left"][0] + c["right"][1]) == 35


@pytest.mark.gpu
def test_pdf_r4_cut_equals_oracle():
    _gpu_equals_oracle("d-r4-cut")


CUT_PLANTS = [(0, 1), (4, 0), (5, 2), (6, 3)]


@functools.lru_cache(maxsize=None)
def cut_plant(left, right):
    """(stream, the oracle's hits over the 35 pairs, the planted index) of one more planted R4 document per place of
    the cut: inside the right word's first character (31 + E2 | 82 AC), exactly between the words, inside the right's
    character behind 30 bytes (E2 82 | AD), and both words over 32 bytes."""
    import pyoracle
    idx = left * len(CUT_RIGHT) + right
    pw = spell(CUT_LEFT, CUT_RIGHT, idx)
    stream = _stream_of("pdf", tuple(sorted(R4.items())), pw.decode())
    window = [spell(CUT_LEFT, CUT_RIGHT, i) for i in range(35)]
    return stream, [k for k, v in enumerate(pyoracle.Ctx(stream).verify_list(window, nthreads=ORACLE_THREADS)) if v], idx


@pytest.mark.parametrize("left,right", CUT_PLANTS)
def test_pdf_r4_cut_plants_on_the_oracle(left, right):
    """The oracle finds the planted pair and exactly the pairs that share its first 32 bytes."""
    _, want, idx = cut_plant(left, right)
    pw = spell(CUT_LEFT, CUT_RIGHT, idx)
    assert idx in want and want == [k for k in range(35) if spell(CUT_LEFT, CUT_RIGHT, k)[:32] == pw[:32]]
    assert len(pw) > 32 and len(want) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("left,right", CUT_PLANTS)
def test_pdf_r4_cut_planted_on_either_side_of_the_cut(left, right):
    stream, want, _ = cut_plant(left, right)
    _search_equals(_fields(stream), CUT_LEFT, CUT_RIGHT, 0, 35, want, (left, right))


# ------------------------------------------------------------------ (e) Office 2007
def test_office_keyspace_has_one_hit_on_the_oracle():
    assert expected("e-office")[1] == [CASES["e-office"]["idx"]]


@pytest.mark.gpu
def test_office_whole_keyspace_equals_oracle():
    _gpu_equals_oracle("e-office")


# ------------------------------------------------------------------ (f) PDF R2 and R6
@pytest.mark.parametrize("name", F_CASES)
def test_mixed_width_window_on_the_oracle(name):
    want = expected(name)[1]
    assert want == _spelled_like_the_password(name) and CASES[name]["idx"] in want


@pytest.mark.gpu
@pytest.mark.parametrize("name", F_CASES)
def test_mixed_width_window_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ (g) the families with a model of their own
MODEL_IDX = 1 * 7 + 1                                      # "é\U0001D11E" + "€x"
MODEL_START, MODEL_COUNT = 2, 38
MODEL_CASES = [("agile", "2010", 128), ("agile", "2013", 256), ("oldoffice", 0), ("oldoffice", 1), ("oldoffice", 3),
               ("oldoffice", 4), ("odf",)]
MODEL_IDS = ["-".join(str(x) for x in c) for c in MODEL_CASES]
KEY40_FAMILIES = ["pdf_r2", "pdf_r34", "office_md5", "office_sha1"]


@functools.lru_cache(maxsize=None)
def model_expected(case):
    """(fields, the model's sorted hit indices over the window of SMALL_LEFT x SMALL_RIGHT) for one family with a
    Python model of its own, the document made for the pair at MODEL_IDX."""
    window = [spell(SMALL_LEFT, SMALL_RIGHT, i).decode() for i in range(MODEL_START, MODEL_START + MODEL_COUNT)]
    pw = window[MODEL_IDX - MODEL_START]
    if case[0] == "agile":
        import agile_model
        stream = agile_model.make_stream(pw, case[1], case[2], 1000, seed=0xC61 + case[2])
        fields, verifies = agile_model.fields_of(stream), agile_model.verifies
    elif case[0] == "oldoffice":
        import oldoffice_model
        stream = oldoffice_model.make_stream(pw, case[1], seed=0xC70 + case[1])
        fields, verifies = _fields(stream), oldoffice_model.verifies
    else:
        import odf_legacy_model
        stream = odf_legacy_model.make_stream(pw, 1024, seed=0xC80)
        fields, verifies = _fields(stream), odf_legacy_model.verifies
    return fields, [MODEL_START + k for k, w in enumerate(window) if verifies(stream, w)]


@pytest.mark.parametrize("case", MODEL_CASES, ids=MODEL_IDS)
def test_model_window_has_the_planted_hit_on_the_model(case):
    assert model_expected(case)[1] == [MODEL_IDX]
    assert MODEL_START < MODEL_IDX < MODEL_START + MODEL_COUNT <= len(SMALL_LEFT) * len(SMALL_RIGHT)
    pw = spell(SMALL_LEFT, SMALL_RIGHT, MODEL_IDX).decode()
    assert [len(ch.encode("utf-16-le")) for ch in pw] == [2, 4, 2, 2]      # BMP and a surrogate pair, both sides


@pytest.mark.gpu
@pytest.mark.parametrize("case", MODEL_CASES, ids=MODEL_IDS)
def test_model_window_equals_the_model(case):
    """Office Agile (SHA-1 and SHA-512, spinCount 1000), Office 97-2003 (types 0, 1, 3, 4) and ODF 1.0 / 1.1."""
    fields, want = model_expected(case)
    _search_equals(fields, SMALL_LEFT, SMALL_RIGHT, MODEL_START, MODEL_COUNT, want, case)


def test_owner_window_on_the_model():
    want = expected("g-owner-r3")[1]
    assert want == _spelled_like_the_password("g-owner-r3") and CASES["g-owner-r3"]["idx"] in want


@pytest.mark.gpu
def test_owner_window_equals_the_model():
    _gpu_equals_oracle("g-owner-r3")


@functools.lru_cache(maxsize=None)
def key40_expected(fam):
    """(fields, the key of "sun7", the model's hits over DUP_LEFT x DUP_RIGHT from index 1 on)."""
    import key40_model as km
    fields = list(km.base_documents()[fam])
    key = km.key_of_password(fields, "sun7")
    n = len(DUP_LEFT) * len(DUP_RIGHT)
    return fields, key, [i for i in range(1, n)
                         if km.key_of_password(fields, spell(DUP_LEFT, DUP_RIGHT, i).decode()) == key]


@pytest.mark.parametrize("fam", KEY40_FAMILIES)
def test_set_key40_window_has_several_hits_on_the_model(fam):
    want = key40_expected(fam)[2]
    assert want == [6, 8, 11, 16, 19] and [spell(DUP_LEFT, DUP_RIGHT, i) for i in want] == [b"sun7"] * 5


@pytest.mark.gpu
@pytest.mark.parametrize("fam", KEY40_FAMILIES)
def test_set_key40_window_equals_the_model_with_several_hits(fam):
    """A collider context: every pair that spells "sun7" derives the key, and all of them are reported."""
    fields, key, want = key40_expected(fam)
    _search_equals(fields, DUP_LEFT, DUP_RIGHT, 1, len(DUP_LEFT) * len(DUP_RIGHT) - 1, want, fam, key40=key)


# ------------------------------------------------------------------ (h) the right table's life cycle
@pytest.mark.gpu
def test_right_table_life_cycle():
    from dprf_amd import _lib, rules
    stream = _stream_of("pdf", tuple(sorted(R5.items())), "sun7")
    left, first, second = [b"sun", b"moon", b"star"], [b"1", b"7", b"x"], [b"x", b"7", b"y", b"7"]
    rule = [rules.parse_rule("$7"), rules.parse_rule("c")]
    with _lib.Context(_fields(stream), devices=[0, 0]) as ctx, _lib.Context(_fields(stream), device=0) as other:
        def others():
            return (ctx.search_mask([LOWER, LOWER, LOWER, DIGITS], 0, 26 ** 3 * 10)[:2],
                    ctx.search_range(LOWER + DIGITS, 4, 0, 36 ** 4)[:2], ctx.verify_list(["sun7", "moon7", "sun7"])[:2],
                    ctx.search_hybrid([DIGITS], 0, 0, 30)[:2], ctx.search_rules(rule, 0, 6)[:2])
        ctx.set_words(left)
        before = others()
        assert before[0][1] == before[1][1] == 1 and before[2][0] == [0, 2] and before[3][0] == [7] and before[4][0] == [0]
        assert ctx.right_words == 0 and ctx.words == 3
        ctx.set_right_words(first)                                          # set
        other.set_words([b"su", b"s"])
        other.set_right_words([b"un7", b"n7"])
        assert (ctx.words, ctx.right_words, other.words, other.right_words) == (3, 3, 2, 2)
        assert ctx.search_combine(0, 9)[0] == [1]
        assert other.search_combine(0, 4)[0] == [1, 2]                      # su + n7, s + un7
        assert ctx.search_combine(0, 9)[0] == [1]                           # two contexts, one device: no mixing
        ctx.set_right_words(second)                                         # replaced: the results follow
        assert ctx.right_words == 4 and ctx.words == 3 and ctx.search_combine(0, 12)[0] == [1, 3]
        assert ctx.search_combine(0, 12, stop_on_first=True, cap=1)[0] == [1]
        with pytest.raises(_lib.DprfError) as ei:                           # a refused table keeps the old one
            ctx.set_right_words([b"7", b"", b"x"])
        assert ei.value.code == _lib.E_DOMAIN and "word 1" in str(ei.value)
        assert ctx.right_words == 4 and ctx.search_combine(0, 12)[0] == [1, 3]
        ctx.set_words([b"moon", b"sun"])                                    # the left table changes alone ...
        assert (ctx.words, ctx.right_words) == (2, 4) and ctx.search_combine(0, 8)[0] == [5, 7]
        with pytest.raises(_lib.DprfError):                                 # ... and a refused left keeps both
            ctx.set_words([b"\0"])
        assert (ctx.words, ctx.right_words) == (2, 4) and ctx.search_combine(0, 8)[0] == [5, 7]
        ctx.set_words(left)
        assert others() == before                                           # every other mode as before
        ctx.set_right_words([])                                             # cleared
        assert ctx.right_words == 0 and ctx.words == 3
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_combine(0, 1)
        assert ei.value.code == _lib.E_INVALID and "right" in str(ei.value) and ctx.last_call_devices() == []
        assert others() == before
        assert other.search_combine(0, 4)[0] == [1, 2]


# ------------------------------------------------------------------ (i) refusals
@pytest.mark.gpu
def test_refusals_after_each_of_which_the_context_serves():
    from dprf_amd import _lib
    stream = _stream_of("pdf", tuple(sorted(R5.items())), "sun7")

    def refused(ctx, code, call, serve, word=None):
        with pytest.raises(_lib.DprfError) as ei:
            call()
        assert ei.value.code == code, ei.value
        assert ctx.last_call_devices() == []                                # a refused call leaves no record
        assert serve() == [1]                                               # ... and the context still serves
        assert word is None or word in str(ei.value), ei.value

    with _lib.Context(_fields(stream), device=0) as ctx:                    # PDF R5: candidates cut at 127 bytes
        listed = lambda: ctx.verify_list(["x", "sun7"])[0]
        refused(ctx, _lib.E_INVALID, lambda: ctx.search_combine(0, 1), listed, "left")      # no table at all
        ctx.set_right_words([b"1", b"7"])
        refused(ctx, _lib.E_INVALID, lambda: ctx.search_combine(0, 1), listed, "left")      # the left one missing
        refused(ctx, _lib.E_INVALID, lambda: ctx.spell_combine(0, 1), listed, "left")
        ctx.set_right_words([])
        ctx.set_words([b"sun", b"m" * 60, b"star"])
        refused(ctx, _lib.E_INVALID, lambda: ctx.search_combine(0, 1), listed, "right")     # the right one missing
        refused(ctx, _lib.E_INVALID, lambda: ctx.spell_combine(0, 1), listed, "right")
        ctx.set_right_words([b"1", b"7", b"four"])
        serve = lambda: ctx.search_combine(0, 9)[0]
        assert serve() == [1]
        for start, count in ((0, 10), (9, 1), (8, 2), (1 << 40, 1)):        # start + count over N1 * N2
            refused(ctx, _lib.E_INVALID, lambda: ctx.search_combine(start, count), serve, "keyspace")
            refused(ctx, _lib.E_INVALID, lambda: ctx.spell_combine(start, count), serve, "keyspace")
        refused(ctx, _lib.E_INVALID, lambda: ctx.spell_combine(0, (1 << 20) + 1), serve)
        assert ctx.search_combine(9, 0)[2]["candidates"] == 0 and ctx.spell_combine(9, 0) == []
        assert ctx.search_combine(3, 6)[2]["candidates"] == 6               # 60 + 4 fill the slot
        ctx.set_right_words([b"1", b"7", b"fives"])
        refused(ctx, _lib.E_PWLEN, lambda: ctx.search_combine(0, 1), listed,
                "left word 1 takes 60 bytes, right word 2 takes 5")
        refused(ctx, _lib.E_PWLEN, lambda: ctx.spell_combine(0, 1), listed, "left word 1")
        # the setter's refusals are set_words', and words_status serves both tables
        for table_, k in (([b"a", b""], 1), ([b"a\0b"], 0), ([b"ok", b"ok", b"x\0"], 2)):
            with pytest.raises(_lib.DprfError) as ei:
                ctx.set_right_words(table_)
            assert ei.value.code == _lib.E_DOMAIN and "word %d" % k in str(ei.value), ei.value
            assert [int(x) for x in ctx.words_status(table_)] == [_lib.E_DOMAIN if j == k else 0 for j in range(len(table_))]
            assert ctx.right_words == 3
    r4 = _stream_of("pdf", tuple(sorted(R4.items())), "sun7")
    with _lib.Context(_fields(r4), device=0) as ctx:                        # R2-R4: words of any length
        ctx.set_words([b"x" * 5000, b"sun"])
        ctx.set_right_words([b"y" * 9000, b"7"])
        assert ctx.search_combine(0, 4)[:2] == ([3], 1)
    office = _stream_of("docx", (), "sun7")
    with _lib.Context(_fields(office), device=0) as ctx:                    # Office: UTF-8 in, 32 units in all
        with pytest.raises(_lib.DprfError) as ei:
            ctx.set_right_words([b"ok", b"\xff"])
        assert ei.value.code == _lib.E_DOMAIN and "word 1" in str(ei.value) and ctx.right_words == 0
        ctx.set_words([("€" * 16).encode(), b"sun"])
        ctx.set_right_words([b"7", ("é" * 16).encode()])
        assert ctx.search_combine(0, 4)[:2] == ([2], 1)
        ctx.set_right_words([b"7", ("é" * 17).encode()])
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_combine(0, 4)
        assert ei.value.code == _lib.E_PWLEN and "left word 0 takes 32 bytes, right word 1 takes 34" in str(ei.value)


# ------------------------------------------------------------------ (j) a never-matching context
@pytest.mark.gpu
def test_never_matching_context_counts_the_window():
    from dprf_amd import _lib
    fields = ["pdf", "2", "4", "128", "-4", "1", "16", "11" * 16, "32", "22" * 32, "32", "33" * 32]
    with _lib.Context(fields, device=0) as ctx:
        assert ctx.flags & _lib.FLAG_NEVER_MATCHES
        ctx.set_words([b"sun", b"moon"])
        ctx.set_right_words([b"1", b"2", b"3"])
        hits, nh, st = ctx.search_combine(1, 5)
        assert hits == [] and nh == 0 and st["candidates"] == 5 and (ctx.words, ctx.right_words) == (2, 3)
        for call in (lambda: ctx.search_combine(1, 6), lambda: ctx.spell_combine(0, 1)):
            with pytest.raises(_lib.DprfError) as ei:
                call()
            assert ei.value.code == _lib.E_INVALID


# ------------------------------------------------------------------ (k) the CLI
@pytest.mark.gpu
def test_cli_combine_end_to_end(tmp_path, capsys):
    import docgen
    from dprf_amd import brute_force, combine
    pdf = str(tmp_path / "budget.pdf")
    wl, wr = tmp_path / "left.txt", tmp_path / "right.txt"
    wl.write_bytes(b"spring\r\n\nsummer\nhiver\xe2\x82\xac\n" + b"q" * 50 + b"\nautumn\n")
    wr.write_bytes(b"2023\n2024\n" + b"r" * 40 + b"\n24\n")
    password = "hiver€-24"
    docgen.write_pdf(pdf, password, SEED, **R5)
    argv = ["3", pdf, "--wordlist", str(wl), "--wordlist2", str(wr), "--rule-left", "$-"]
    capsys.readouterr()
    assert brute_force.main(argv) == (1, password)
    out = capsys.readouterr().out
    # 51 + 40 bytes do not share a slot: of the 63 splits, dropping the one long left word keeps the most pairs (4 x 4;
    # dropping the long right word instead keeps 5 x 3)
    left = [b"spring-", b"summer-", "hiver€-".encode(), b"autumn-"]
    right = [b"2023", b"2024", b"r" * 40, b"24"]
    assert combine.fit([7, 7, 9, 51, 7], [4, 4, 40, 2]) == (9, 55)
    assert "Dropped 1 left words over 9 bytes and 0 right words over 55 bytes" in out and "not searched" in out
    idx = combine.index_of(left, right, password)
    assert idx == 2 * 4 + 3 and combine.space(len(left), len(right)) == 16
    # a checkpoint written mid-search resumes at its cursor ...
    cp = str(tmp_path / "cursor.json")
    data = brute_force.parse_verification_data(brute_force.get_verification_data("3", pdf))
    read_l, read_r = brute_force._read_words(str(wl)), brute_force._read_words(str(wr))
    key = brute_force.Checkpoint(cp, data, wordlist=brute_force.wordlist_key(read_l),
                                 wordlist2=brute_force.wordlist_key(read_r), side_rules=("$-", ""))
    key.save(5)
    capsys.readouterr()
    assert brute_force.main(argv + ["--checkpoint", cp]) == (1, password)
    assert "Checkpoint: resuming at index 5" in capsys.readouterr().out
    assert json.load(open(cp))["found"] == password and json.load(open(cp))["next_index"] == 16
    # ... also when the cursor lies past the password: the indices below it are not searched again
    key.save(idx + 1)
    assert brute_force.main(argv + ["--checkpoint", cp]) == (0, brute_force.DEFAULT_PASSWORD)
    # a changed rule and a changed right wordlist are refused by the checkpoint
    with pytest.raises(ValueError):
        brute_force.main(argv[:-2] + ["--rule-left", "$_", "--checkpoint", cp])
    wr.write_bytes(wr.read_bytes() + b"25\n")
    with pytest.raises(ValueError):
        brute_force.main(argv + ["--checkpoint", cp])


@pytest.mark.gpu
def test_cli_stdout_prints_the_window_the_model_spells(tmp_path, capsysbinary):
    """--stdout: the candidates as the device spells them, after the side rules and the format's cut; nothing verified."""
    import docgen
    from dprf_amd import brute_force, combine
    wl, wr = tmp_path / "left.txt", tmp_path / "right.txt"
    wl.write_bytes(b"spring\nhiver\xe2\x82\xac\n\xff\xfe\n" + b"q" * 31 + b"\n")
    wr.write_bytes(b"2024\n\xe2\x82\xac1\n")
    pdf = str(tmp_path / "budget.pdf")
    docgen.write_pdf(pdf, "Hiver€-2024", SEED, **R4)
    argv = ["3", pdf, "--wordlist", str(wl), "--wordlist2", str(wr), "--rule-left", "c", "--rule-right", "^-", "--stdout"]
    left = [b"Spring", "Hiver€".encode(), b"\xff\xfe", b"Q" + b"q" * 30]
    right = [b"-2024", "-€1".encode()]
    capsysbinary.readouterr()
    assert brute_force.main(argv) == (0, 8)
    out = capsysbinary.readouterr().out
    want = b"".join(combine.candidate(left, right, i)[:32] + b"\n" for i in range(8))
    assert out.endswith(want) and b"Correct password" not in out and b"Tried" not in out
    assert b"Hiver\xe2\x82\xac-2024\n" in out and b"\xff\xfe-2024\n" in out and (b"q" * 30 + b"-\n") in out   # cut at 32
