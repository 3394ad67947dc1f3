"""Device-spelled rule windows (dprf_search_rules: k_spell_rules + the list kernels) against the oracle: the hit set of
a whole window equals the set pyoracle finds over the same window spelled by this suite's own implementation of the
rule language (test_rules_model.ref_apply; the oracle does its own UTF-16LE conversion and truncation), on one, two
and four device lanes, with stop_on_first returning the oracle's lowest.

  (a) ODF `-e` (2-byte check): false positives besides the planted password, and without it
  (b) PDF R5 (one SHA-256 per candidate): planted at a run's first and last rule for R = 255, 256, 257; unaligned
      starts, count = 1, the keyspace's last candidate, and a window across index 2^32
  (c) PDF R4: two rules whose results share their first 32 bytes
  (d) Office 2007: a whole small keyspace
  (e) PDF R2 and R6: windows of 2^12 whose start is no multiple of 64
  (f) Office Agile (both hashes) against agile_model.verifies
  (g) owner mode (PDF R3)
  (h) the life cycle, (i) the refusals, (j) the CLI end to end with a checkpoint and --stdout

Every oracle case has a CPU test of its preconditions on the oracle alone, so no GPU comparison passes vacuously.  The
oracle's set is computed once per case and shared."""
import functools
import json

import numpy as np
import pytest

import test_hybrid_windows as hw
import test_rules_model as rm
import test_rules_spell as rs
from test_mask_windows import DEVICE_LISTS, DIGITS, LOWER, R2, R4, R5, R6, SEED, _fields, _stream_of

ORACLE_THREADS = 16
R3 = {"R": 3, "length": 128}


def rules_of(texts):
    """Rule texts without blanks as parameters -> parsed rules, by this suite's own reading of the notation."""
    return [tuple(rm.fn_of(t) for t in text.split(" ")) for text in texts]


BASE = rules_of([
    ":", "l", "u", "c", "C", "t", "r", "d", "f", "{", "}", "q", "k", "K", "[", "]", "E", "$1", "$!", "^1", "c $1",
    "c $1 $2", "$2 $0 $2 $4", "sa@", "so0", "se3", "sa@ so0", "T0", "T1", "T2", "D0", "D1", "D2", "'4", "'5", "'6",
    "x03", "x14", "O12", "i1-", "i3.", "o0X", "o1_", "z1", "z2", "Z1", "Z2", "y2", "Y2", "p1", ".1", ",1", "*01",
    "*12", "@a", "@e", "r c", "u r", "d ]", "c $!", "l $1 $2 $3", "^! $!", "t $7", "E $9"])
MANY = BASE + rm.random_rules(193, 0x2B1, lo=1, hi=3)          # 257 rules; a prefix of R of them is a case's rule list
ODF_WORDS = hw.ODF_WORDS                                       # 6000 words
ODF_PW_IDX = 3210 * 64 + 21                                    # word 3210 under "c $1 $2"
WORDS = hw.WORDS                                               # > 2500 distinct words of 3..12 characters
NW = len(WORDS)
CUT_WORDS = [b"sun", b"a" * 31, ("x" * 30 + "€").encode(), b"moon"]
CUT_RULES = rules_of([":", "$1 $2", "r", "$1 $3", "$2", "d"])
OFFICE_WORDS = ["a€".encode(), "Zé".encode(), b"summer", "Hiver€".encode()]
OFFICE_RULES = BASE[:30]
AGILE_RULES = BASE[:20]
BIG_R = 1 << 20


def _is_text(b):
    try:
        return all(ch.isprintable() for ch in b.decode("utf-8"))
    except UnicodeDecodeError:
        return False


def spell(words, rules, i):
    w, r = divmod(i, len(rules))
    return rm.ref_apply(rules[r], words[w])


def _case(kind, kw, words, rules, idx, start, count, **more):
    return dict({"kind": kind, "kw": kw, "words": words, "rules": rules, "idx": idx, "start": start, "count": count},
                **more)


def _r5(words, rules, idx, start, count):
    return _case("pdf", R5, words, rules, idx, start, count)


def _edge(R, w, last):
    """A planted candidate that is the first or the last rule of a word's run of R: word w, or the first one after it
    whose candidate is text a document can be made with."""
    r = R - 1 if last else 0
    while not _is_text(rm.ref_apply(MANY[r], WORDS[w])):
        w += 1
    idx = w * R + r
    return _r5(WORDS, MANY[:R], idx, idx - 300, 1000)


CASES = {
    "a-odf-e-planted": _case("odt_e", {}, ODF_WORDS, BASE, ODF_PW_IDX, ODF_PW_IDX - 20001, 1 << 15),
    "a-odf-e-false-positives": None,                           # filled below from ODF_WINDOW
    "b-r255-first": _edge(255, 7, False),
    "b-r255-last": _edge(255, 7, True),
    "b-r256-first": _edge(256, 9, False),
    "b-r256-last": _edge(256, 9, True),
    "b-r257-first": _edge(257, 11, False),
    "b-r257-last": _edge(257, 11, True),
    "b-r1": _r5(WORDS, BASE[:1], 1255, 1000, 1000),
    "b-r63-inside-a-run": _r5(WORDS, MANY[:63], 63 * 40 + 17, 63 * 40 + 5, 1000),
    "b-r64-inside-a-run": _r5(WORDS, BASE, 64 * 50 + 20, 64 * 41 + 33, 1000),
    "b-count-1": _r5(WORDS, BASE, 64 * 66 + 21, 64 * 66 + 21, 1),
    "b-keyspace-last": _r5(WORDS, BASE, NW * 64 - 1, NW * 64 - 777, 777),
    "b-across-2^32": _r5(rs.BIG_WORDS, "big", (1 << 32) + 5, (1 << 32) - 100, 1000),
    "c-r4-shared-32-bytes": _case("pdf", R4, CUT_WORDS, CUT_RULES, 1 * 6 + 1, 0, 24),
    "d-office": _case("docx", {}, OFFICE_WORDS, OFFICE_RULES, 3 * 30 + 21, 0, 120),
    "e-pdf-r2": _case("pdf", R2, WORDS, BASE, 64 * 700 + 20, 64 * 700 - 2001, 1 << 12),
    "e-pdf-r6": _case("pdf", R6, WORDS, BASE, 64 * 900 + 59, 64 * 900 - 3003, 1 << 12),
    "g-owner-r3": _case("pdf", R3, WORDS, BASE, 64 * 1500 + 21, 64 * 1500 - 1001, 1 << 11, owner=True),
}
# (a): the oracle over the whole keyspace of ODF_WORDS x BASE on the planted document (found once; the CPU test below
# checks the windows used against the oracle itself)
ODF_ALL = [120936, 130702, 130718, 205461, 254794, 285038, 285664, 340690]
ODF_WINDOW = (120936 - 3333, 1 << 15)                         # three false positives, the planted password outside
CASES["a-odf-e-false-positives"] = _case("odt_e", {}, ODF_WORDS, BASE, ODF_PW_IDX, ODF_WINDOW[0], ODF_WINDOW[1],
                                         planted_outside=True)
A_CASES = [k for k in CASES if k.startswith("a-")]
B_CASES = [k for k in CASES if k.startswith("b-")]
E_CASES = [k for k in CASES if k.startswith("e-")]


@functools.lru_cache(maxsize=None)
def big_rules():
    return rs.big_rule_table()


def _rules_arg(c):
    return big_rules() if c["rules"] == "big" else c["rules"]


def _spell_case(c, i):
    if c["rules"] != "big":
        return spell(c["words"], c["rules"], i)
    from dprf_amd import rules as rulemod                      # only to unpack the encoded word of the one rule
    fns, _ = big_rules()
    w, r = divmod(i, BIG_R)
    return rm.ref_apply(rulemod.decode(fns[r:r + 1], [0, 1])[0], c["words"][w])


def _password(name):
    c = CASES[name]
    b = _spell_case(c, c["idx"])
    return b.decode("utf-8")


@functools.lru_cache(maxsize=None)
def expected(name):
    """(stream, the oracle's sorted hit indices of the case's window): once per case, for every test that needs it."""
    import pyoracle
    c = CASES[name]
    kw = dict(c["kw"], owner=_password(name)) if c.get("owner") else c["kw"]
    pw = "user" if c.get("owner") else _password(name)
    stream = _stream_of(c["kind"], tuple(sorted(kw.items())), pw)
    office = c["kind"] == "docx"
    window = []
    for i in range(c["start"], c["start"] + c["count"]):
        if office:      # the model spells UTF-16 units; the oracle converts UTF-8 itself
            w, r = divmod(i, len(c["rules"]))
            window.append(rm.ref_apply(c["rules"][r], c["words"][w], office=True).decode("utf-16-le").encode())
        else:
            window.append(_spell_case(c, i))
    if c.get("owner"):
        import owner_model
        return stream, [c["start"] + k for k, w in enumerate(window) if owner_model.owner_verifies(stream, w)]
    verdicts = pyoracle.Ctx(stream).verify_list(window, nthreads=ORACLE_THREADS)
    return stream, [c["start"] + k for k, v in enumerate(verdicts) if v]


def _gpu_equals_oracle(name):
    from dprf_amd import _lib
    c = CASES[name]
    stream, want = expected(name)
    assert want, name
    rules = _rules_arg(c)
    for devs in DEVICE_LISTS:
        with _lib.Context(_fields(stream), devices=devs, pdf_password="owner" if c.get("owner") else "user") as ctx:
            ctx.set_words(c["words"])
            hits, nh, st = ctx.search_rules(rules, c["start"], c["count"])
            assert hits == want and nh == len(want), (name, devs, hits[:8], want[:8], nh, len(want))
            assert st["candidates"] == c["count"], (name, devs, st)
            first, _, _ = ctx.search_rules(rules, c["start"], c["count"], stop_on_first=True, cap=1)
            assert first == want[:1], (name, devs, first, want[:1])


def test_cases_lie_inside_their_keyspaces():
    assert len(BASE) == 64 and len(MANY) == 257
    assert {f for r in BASE for f, _, _ in r} == set(rm.ALL_FUNCTIONS)
    for name, c in CASES.items():
        R = BIG_R if c["rules"] == "big" else len(c["rules"])
        n = len(c["words"]) * R
        assert 0 <= c["start"] and c["start"] + c["count"] <= n, name
        assert c.get("planted_outside") or c["start"] <= c["idx"] < c["start"] + c["count"], name
        assert c["count"] <= (1000 if name in B_CASES else 1 << 17), name
        assert all(1 <= len(w) <= 64 for w in c["words"]), name
    assert NW >= 2500 and len(set(WORDS)) == NW
    for R in (255, 256, 257):
        assert CASES["b-r%d-first" % R]["idx"] % R == 0 and CASES["b-r%d-last" % R]["idx"] % R == R - 1
        assert len(CASES["b-r%d-first" % R]["rules"]) == R
    for name in ("b-r63-inside-a-run", "b-r64-inside-a-run", "e-pdf-r2", "e-pdf-r6", "a-odf-e-false-positives"):
        c = CASES[name]
        assert c["start"] % 64 and c["start"] % len(c["rules"]), name
    assert CASES["b-count-1"]["count"] == 1 and CASES["b-keyspace-last"]["idx"] == NW * 64 - 1
    c = CASES["b-across-2^32"]
    assert c["start"] < 1 << 32 < c["start"] + c["count"] and len(c["words"]) * BIG_R > c["start"] + c["count"]
    for name in E_CASES:
        assert CASES[name]["count"] == 1 << 12
    a, b = spell(CUT_WORDS, CUT_RULES, 7), spell(CUT_WORDS, CUT_RULES, 9)
    assert a != b and a[:32] == b[:32] and len(a) == 33
    assert 1 << 15 <= ODF_WINDOW[1] <= 1 << 17 and len(ODF_WORDS) == 6000


# ------------------------------------------------------------------ (a) ODF -e: false positives
def test_odf_e_windows_on_the_oracle():
    lo, n = ODF_WINDOW
    want = [h for h in ODF_ALL if lo <= h < lo + n]
    assert len(want) >= 2 and ODF_PW_IDX not in want and ODF_PW_IDX in ODF_ALL
    assert expected("a-odf-e-false-positives")[1] == want
    c = CASES["a-odf-e-planted"]
    got = expected("a-odf-e-planted")[1]
    assert got == [h for h in ODF_ALL if c["start"] <= h < c["start"] + c["count"]] and ODF_PW_IDX in got
    # a false positive is a candidate other than the password
    pw = _password("a-odf-e-planted").encode()
    assert sum(1 for h in want if spell(ODF_WORDS, BASE, h) != pw) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", A_CASES)
def test_odf_e_window_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ (b) PDF R5: planted edges and window shapes
@pytest.mark.parametrize("name", B_CASES)
def test_pdf_r5_planted_candidate_verifies_on_the_oracle(name):
    c = CASES[name]
    want = expected(name)[1]
    pw = _password(name).encode()
    assert c["idx"] in want and all(_spell_case(c, h) == pw for h in want)  # the password's other spellings only


@pytest.mark.gpu
@pytest.mark.parametrize("name", B_CASES)
def test_pdf_r5_planted_window_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ (c) PDF R4: the 32-byte cut
def test_pdf_r4_shared_prefix_on_the_oracle():
    assert expected("c-r4-shared-32-bytes")[1] == [7, 9]


@pytest.mark.gpu
def test_pdf_r4_shared_prefix_equals_oracle():
    _gpu_equals_oracle("c-r4-shared-32-bytes")


# ------------------------------------------------------------------ (d) Office 2007
def test_office_keyspace_on_the_oracle():
    want = expected("d-office")[1]
    assert CASES["d-office"]["idx"] in want and len(want) <= 4
    assert _password("d-office") == "Hiver€12"


@pytest.mark.gpu
def test_office_whole_keyspace_equals_oracle():
    _gpu_equals_oracle("d-office")


# ------------------------------------------------------------------ (e) PDF R2 and R6
@pytest.mark.parametrize("name", E_CASES)
def test_unaligned_window_on_the_oracle(name):
    assert CASES[name]["idx"] in expected(name)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", E_CASES)
def test_unaligned_window_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ (f) Office Agile
def _agile_case(version, bits):
    import agile_model
    words, rules = OFFICE_WORDS, AGILE_RULES
    start, count = 0, 80
    idx = 3 * 20 + 17                                                       # "Hiver€" under "$1"
    cands = [rm.ref_apply(rules[i % 20], words[i // 20], office=True).decode("utf-16-le") for i in range(count)]
    stream = agile_model.make_stream(cands[idx], version, bits, 1000, seed=0xA71 + bits)
    want = [start + k for k, pw in enumerate(cands) if agile_model.verifies(stream, pw)]
    return stream, words, rules, start, count, idx, want


@pytest.mark.parametrize("version,bits", [("2010", 128), ("2013", 256)])
def test_agile_window_on_the_model(version, bits):
    _, _, _, _, _, idx, want = _agile_case(version, bits)
    assert idx in want and len(want) <= 3


@pytest.mark.gpu
@pytest.mark.parametrize("version,bits", [("2010", 128), ("2013", 256)])
def test_agile_window_equals_the_model(version, bits):
    import agile_model
    from dprf_amd import _lib
    stream, words, rules, start, count, idx, want = _agile_case(version, bits)
    for devs in DEVICE_LISTS:
        with _lib.Context(agile_model.fields_of(stream), devices=devs) as ctx:
            ctx.set_words(words)
            hits, nh, st = ctx.search_rules(rules, start, count)
            assert hits == want and nh == len(want) and st["candidates"] == count, (version, devs, hits, st)
            assert ctx.search_rules(rules, start, count, stop_on_first=True, cap=1)[0] == want[:1]


# ------------------------------------------------------------------ (g) owner mode
def test_owner_window_on_the_model():
    assert CASES["g-owner-r3"]["idx"] in expected("g-owner-r3")[1]


@pytest.mark.gpu
def test_owner_window_equals_the_model():
    _gpu_equals_oracle("g-owner-r3")


# ------------------------------------------------------------------ (h) the life cycle
LIFE_RULES = rules_of([":", "$7", "c $7", "r"])


@pytest.mark.gpu
def test_life_cycle():
    from dprf_amd import _lib
    first, second = [b"sun", b"moon", b"star"], [b"star", b"sun", b"sun", b"moon!"]
    stream = _stream_of("pdf", tuple(sorted(R5.items())), "sun7")
    with _lib.Context(_fields(stream), devices=[0, 0]) as ctx, _lib.Context(_fields(stream), device=0) as other:
        def others():
            return (ctx.search_mask([LOWER, LOWER, LOWER, DIGITS], 0, 26 ** 3 * 10)[:2],
                    ctx.search_range(LOWER + DIGITS, 4, 0, 36 ** 4)[:2], ctx.verify_list(["sun7", "moon7", "sun7"])[:2],
                    ctx.search_hybrid([DIGITS], 0, 0, 10 * ctx.words)[:2] if ctx.words else None)
        before = others()
        assert before[0][1] == before[1][1] == 1 and before[2][0] == [0, 2]
        ctx.set_words(first)
        other.set_words(second)
        with_table = others()
        assert with_table[3] == ([7], 1)
        assert ctx.search_rules(LIFE_RULES, 0, 12)[0] == [1]
        assert other.search_rules(LIFE_RULES, 0, 16)[0] == [5, 9]           # a repeated word is verified twice
        assert ctx.search_rules(LIFE_RULES, 0, 12)[0] == [1]                # two contexts, one device: no mixing
        assert others() == with_table                                       # the other calls are as before
        assert ctx.spell_rules(LIFE_RULES, 0, 4) == [b"sun", b"sun7", b"Sun7", b"nus"]
        assert others() == with_table
        ctx.set_words(second)                                               # the results follow the second table
        assert ctx.search_rules(LIFE_RULES, 0, 16)[0] == [5, 9]
        assert ctx.search_rules(LIFE_RULES, 0, 16, stop_on_first=True, cap=1)[0] == [5]
        assert ctx.search_rules(LIFE_RULES[:1] + LIFE_RULES[2:], 0, 12)[0] == []   # other rules, other results
        ctx.set_words([])
        assert others()[:3] == before[:3]
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_rules(LIFE_RULES, 0, 1)
        assert ei.value.code == _lib.E_INVALID and ctx.last_call_devices() == []
        assert other.search_rules(LIFE_RULES, 0, 16)[0] == [5, 9]


# ------------------------------------------------------------------ (i) refusals
def _enc(rules):
    from dprf_amd import rules as rulemod
    return rulemod.encode(rules)


def _refused(ctx, code, call, serve):
    from dprf_amd import _lib
    with pytest.raises(_lib.DprfError) as ei:
        call()
    assert ei.value.code == code, ei.value
    assert ctx.last_call_devices() == []                                    # a refused call leaves no record
    assert serve() == [1]                                                   # ... and the context still serves
    return str(ei.value)


@pytest.mark.gpu
def test_refusals_after_each_of_which_the_context_serves():
    import ctypes
    from dprf_amd import _lib
    u32 = lambda xs: np.asarray(xs, dtype=np.uint32)
    words = [b"sun", b"moon", b"star"]
    stream = _stream_of("pdf", tuple(sorted(R5.items())), "sun7")
    ok_f, ok_o = _enc(LIFE_RULES)
    with _lib.Context(_fields(stream), device=0) as ctx:
        with pytest.raises(_lib.DprfError) as ei:                           # no word table yet
            ctx.search_rules(LIFE_RULES, 0, 1)
        assert ei.value.code == _lib.E_INVALID and ctx.last_call_devices() == []
        ctx.set_words(words)
        serve = lambda: ctx.search_rules(LIFE_RULES, 0, 12)[0]
        assert serve() == [1]
        both = lambda f, o, s=0, n=1: [lambda: ctx.search_rules((f, o), s, n), lambda: ctx.spell_rules((f, o), s, n)]
        invalid = (both(ok_f, u32([0])) +                                   # nrules = 0
                   both(ok_f, u32([0, 1, 3, 2, 5])) +                       # offsets not ascending
                   both(ok_f, u32([0, 1, 1, 3, 5])) +                       # a rule of 0 functions
                   both(u32([ord(":")] * 33), u32([0, 33])) +               # a rule of 33 functions
                   both(ok_f, ok_o, 0, 13) + both(ok_f, ok_o, 12, 1) + both(ok_f, ok_o, 11, 2) +   # over N * R
                   [lambda: ctx.spell_rules(rs.big_rule_table(), 0, (1 << 20) + 1)])           # spell: over 2^20
        for call in invalid:
            _refused(ctx, _lib.E_INVALID, call, serve)
        L = _lib.lib()                                                      # null arguments, at the export itself
        st, nh, hits = _lib.Stats(), ctypes.c_int64(), (ctypes.c_uint64 * 1)()
        p = ok_f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ok_o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        assert L.dprf_search_rules(ctx._h, None, p[1], 4, 0, 1, 0, hits, 1, ctypes.byref(nh), ctypes.byref(st)) == -1
        assert L.dprf_search_rules(ctx._h, p[0], None, 4, 0, 1, 0, hits, 1, ctypes.byref(nh), ctypes.byref(st)) == -1
        assert L.dprf_spell_rules(ctx._h, p[0], p[1], 4, 0, 1, None, None) == -1
        assert L.dprf_search_rules(None, p[0], p[1], 4, 0, 1, 0, hits, 1, ctypes.byref(nh), ctypes.byref(st)) == -1
        assert ctx.last_call_devices() == [] and serve() == [1]
        too_many = np.full((1 << 20) + 1, ord(":"), dtype=np.uint32)        # nrules over DPRF_MAX_RULES
        _refused(ctx, _lib.E_INVALID, lambda: ctx.search_rules((too_many, np.arange((1 << 20) + 2, dtype=np.uint32)), 0, 1),
                 serve)
        full = np.full((1 << 22) + 8, ord(":"), dtype=np.uint32)            # over DPRF_MAX_RULE_WORDS in all
        _refused(ctx, _lib.E_INVALID, lambda: ctx.search_rules((full, np.arange(0, (1 << 22) + 9, 8, dtype=np.uint32)), 0, 1),
                 serve)
        one = lambda w: (u32([ord(":"), w]), u32([0, 1, 2]))                # rule 1, function 0 is the bad one
        charset = [ord("+"), ord("L") | 1 << 8, 0x01, ord("T") | 36 << 8, ord("x") | 1 << 8 | 36 << 16,
                   ord("$"), ord("s") | 97 << 8, ord("i") | 1 << 8, ord("l") | 1 << 8, ord("T") | 1 << 8 | 1 << 16,
                   ord("$") | 97 << 8 | 1 << 16, ord(":") | 1 << 24]
        for w in charset:
            for call in both(*one(w), 0, 1):
                msg = _refused(ctx, _lib.E_CHARSET, call, serve)
                assert "rule 1" in msg and "function 0" in msg, msg
        assert ctx.search_rules(one(ord("$") | 0xff << 8), 0, 6)[2]["candidates"] == 6    # 0xFF is a unit here
        ctx.set_words([b"ok", b"x" * 65, b"sun"])                           # held; rules refuse the long word
        for call in both(ok_f, ok_o, 0, 1):
            with pytest.raises(_lib.DprfError) as ei:
                call()
            assert ei.value.code == _lib.E_PWLEN and "word 1" in str(ei.value) and ctx.last_call_devices() == []
        ctx.set_words(words)
        assert serve() == [1]
    office, _ = hw.mw.expected("c-office-mixed")
    with _lib.Context(_fields(office), device=0) as ctx:                    # Office: units 0x01..0x7F only
        ctx.set_words([b"ok", ("€" * 32).encode()])
        assert ctx.search_rules(one(ord("$") | 0x7f << 8), 0, 4)[2]["candidates"] == 4
        for w in (ord("$") | 0x80 << 8, ord("s") | 97 << 8 | 0xff << 16, ord("o") | 0x80 << 16):
            with pytest.raises(_lib.DprfError) as ei:
                ctx.search_rules(one(w), 0, 1)
            assert ei.value.code == _lib.E_CHARSET and "rule 1" in str(ei.value) and ctx.last_call_devices() == []
        ctx.set_words([b"ok", ("€" * 33).encode()])                         # 66 bytes of UTF-16LE
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_rules(LIFE_RULES, 0, 1)
        assert ei.value.code == _lib.E_PWLEN and "word 1" in str(ei.value)
    r4, _ = hw.mw.expected("b-pdf-r4-cut")
    with _lib.Context(_fields(r4), device=0) as ctx:                        # R2-R4 too: no clipped copy for rules
        ctx.set_words([b"y", b"x" * 65])
        assert ctx.search_hybrid([], 0, 0, 2)[2]["candidates"] == 2
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_rules(LIFE_RULES, 0, 1)
        assert ei.value.code == _lib.E_PWLEN and "word 1" in str(ei.value) and ctx.last_call_devices() == []


@pytest.mark.gpu
def test_never_matching_context_counts_the_window_and_spells_nothing():
    from dprf_amd import _lib
    fields = ["pdf", "2", "4", "128", "-4", "1", "16", "11" * 16, "32", "22" * 32, "32", "33" * 32]
    with _lib.Context(fields, device=0) as ctx:
        assert ctx.flags & _lib.FLAG_NEVER_MATCHES
        ctx.set_words([b"sun", b"moon"])
        hits, nh, st = ctx.search_rules(LIFE_RULES, 3, 5)
        assert hits == [] and nh == 0 and st["candidates"] == 5
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_rules(LIFE_RULES, 3, 6)
        assert ei.value.code == _lib.E_INVALID
        with pytest.raises(_lib.DprfError) as ei:
            ctx.spell_rules(LIFE_RULES, 0, 1)
        assert ei.value.code == _lib.E_INVALID


def test_binding_refuses_a_window_over_64_bits_and_packs_the_rule_table(monkeypatch):
    """No device: what Context.search_rules hands to the export, and _check_window before it."""
    import ctypes
    from dprf_amd import _lib
    calls = []

    class Lib:
        @staticmethod
        def dprf_search_rules(h, fns, off, n, start, count, stop, hits, cap, nh, st):
            calls.append(([fns[k] for k in range(off[n])], [off[k] for k in range(n + 1)], n, start, count, stop, cap))
            hits[0] = 3
            nh._obj.value = 1
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib)
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._h = ctypes.c_void_p(1)
    try:
        rules = rules_of(["c $1", "sa@ x3Z"])
        want = ([ord("c"), ord("$") | 49 << 8, ord("s") | 97 << 8 | 64 << 16, ord("x") | 3 << 8 | 35 << 16], [0, 2, 4], 2)
        assert ctx.search_rules(rules, 100, 7, stop_on_first=True, cap=2)[:2] == ([103], 1)
        assert ctx.search_rules(_enc(rules), 5, 1)[:2] == ([8], 1)
        assert calls == [want + (100, 7, 1, 2), want + (5, 1, 0, 1 << 16)]
        for start, count in ((-1, 1), (0, 1 << 64), ((1 << 64) - 1, 1)):
            with pytest.raises(_lib.DprfError) as ei:
                ctx.search_rules(rules, start, count)
            assert ei.value.code == _lib.E_INVALID
            with pytest.raises(_lib.DprfError):
                ctx.spell_rules(rules, start, count)
    finally:
        ctx._h = None


# ------------------------------------------------------------------ (j) the CLI
@pytest.mark.gpu
def test_cli_rules_end_to_end_checkpoint_and_stdout(tmp_path, capsys):
    import docgen
    from dprf_amd import brute_force, hybrid
    pdf = str(tmp_path / "budget.pdf")
    wl = tmp_path / "words.txt"
    wl.write_bytes(b"spring\r\n\nsummer\nhiver\xe2\x82\xac\n" + b"q" * 70 + b"\nautumn\n")
    rf = tmp_path / "some.rule"
    rf.write_bytes(b"# season rules\n:\nc\nu +0\n$2 $4\nc $2 $4\nr\n")
    password = "Hiver€24"
    docgen.write_pdf(pdf, password, SEED, **R5)
    argv = ["3", pdf, "--wordlist", str(wl), "--rules", str(rf)]
    capsys.readouterr()
    assert brute_force.main(argv) == (1, password)
    out = capsys.readouterr().out
    assert "Dropped 1 words too long" in out and "Skipped 1 lines" in out
    kept = [b"spring", b"summer", "hiver€".encode(), b"autumn"]
    rules = rules_of([":", "c", "$2 $4", "c $2 $4", "r"])
    idx = 2 * 5 + 3
    assert rm.ref_apply(rules[3], kept[2]).decode() == password
    # a checkpoint written mid-search resumes at its cursor ...
    cp = str(tmp_path / "cursor.json")
    data = brute_force.parse_verification_data(brute_force.get_verification_data("3", pdf))
    read = hybrid.read_wordlist(str(wl))
    key = brute_force.Checkpoint(cp, data, mask="?w", custom=(), wordlist=brute_force.wordlist_key(read),
                                 rules=brute_force.rules_key(rules))
    key.save(5)
    capsys.readouterr()
    assert brute_force.main(argv + ["--checkpoint", cp]) == (1, password)
    assert "Checkpoint: resuming at index 5" in capsys.readouterr().out
    assert json.load(open(cp))["found"] == password and json.load(open(cp))["next_index"] == 20
    # ... also when the cursor lies past the password: the indices below it are not searched again
    key.save(idx + 1)
    assert brute_force.main(argv + ["--checkpoint", cp]) == (0, brute_force.DEFAULT_PASSWORD)
    # a hybrid search of the bare words does not load the rule search's file, nor the other way round
    with pytest.raises(ValueError):
        brute_force.main(["3", pdf, "--wordlist", str(wl), "--checkpoint", cp])
    # a changed rule file is refused by the checkpoint
    rf.write_bytes(rf.read_bytes() + b"d\n")
    with pytest.raises(ValueError):
        brute_force.main(argv + ["--checkpoint", cp])
    # two rule files are multiplied, the first slowest
    r2 = tmp_path / "two.rule"
    r2.write_bytes(b"$2 $4\n$!\n")
    r1 = tmp_path / "one.rule"
    r1.write_bytes(b":\nc\n")
    capsys.readouterr()
    assert brute_force.main(["3", pdf, "--wordlist", str(wl), "--rules", str(r1), "--rules", str(r2)]) == (1, password)
    # --rules needs --wordlist and takes no mask around the word
    for bad in (["3", pdf, "--rules", str(rf)], argv + ["--mask", "?w?d"]):
        with pytest.raises(SystemExit):
            brute_force.main(bad)
    with pytest.raises(ValueError):
        brute_force.init("x:$pdf$1*2", None, None, rules=[str(rf)])


@pytest.mark.gpu
def test_cli_stdout_prints_the_window_the_model_spells(tmp_path, capsysbinary):
    """--stdout: the candidates' bytes, one per line, nothing verified; for Office the units as UTF-8."""
    import docgen
    from dprf_amd import brute_force
    wl = tmp_path / "words.txt"
    wl.write_bytes(b"spring\nhiver\xe2\x82\xac\n" + b"q" * 70 + b"\nautumn\n")
    rf = tmp_path / "some.rule"
    rf.write_bytes(b":\nc $2 $4\nr\n$\xff\n")
    kept = [b"spring", "hiver€".encode(), b"autumn"]
    rules = rules_of([":", "c $2 $4", "r"]) + [(("$", 0xff, 0),)]
    pdf = str(tmp_path / "budget.pdf")
    docgen.write_pdf(pdf, "Hiver€24", SEED, **R4)
    capsysbinary.readouterr()
    assert brute_force.main(["3", pdf, "--wordlist", str(wl), "--rules", str(rf), "--stdout"]) == (0, 12)
    out = capsysbinary.readouterr().out
    want = b"".join(spell(kept, rules, i) + b"\n" for i in range(12))
    assert out.endswith(want) and b"Correct password" not in out and b"Tried" not in out
    assert b"\n\xac\x82\xe2revih\n" in out and b"spring\xff\n" in out        # raw bytes, valid UTF-8 or not
    docx = str(tmp_path / "budget.docx")
    docgen.write_docx(docx, "Hiver€24", SEED)
    capsysbinary.readouterr()
    assert brute_force.main(["1", docx, "--wordlist", str(wl), "--rules", str(rf), "--stdout"]) == (0, 9)
    out = capsysbinary.readouterr().out
    assert b"Dropped 1 rules" in out                                         # 0xFF is no Office unit
    want = b"".join(rm.ref_apply(rules[i % 3], kept[i // 3], office=True).decode("utf-16-le").encode() + b"\n"
                    for i in range(9))
    assert out.endswith(want) and "€revih\n".encode() in out
