"""Device-spelled rule windows (dprf_spell_rules: k_spell_rules alone, no verification) against this suite's own
implementation of the rule language (test_rules_model.ref_units), byte-exact, slot bytes and lengths, every candidate:

  (a) the matrix -- one word of every length 1..64 and a dozen multi-byte words times every parameterless function,
      every position function at every N, x / O / * at every (N, M) and the unit functions over a few units -- on PDF
      R6 (no cut), PDF R4 (the 32-byte cut) and Office 2007 (2-byte units, LIMIT 32)
  (b) 4,096 random rules of 1..32 functions times the 64 words: all functions mixed within every wave
  (c) window shapes: R = 1, 63, 64, 255, 256, 257, a start inside a word's run of rules, count = 1, the keyspace's
      last candidate, and a window across index 2^32 (2^20 rules x 4,200 words)

A CPU test checks the matrix's preconditions: every function is in it and changes some word, and both global rules
(over LIMIT, empty) fire."""
import functools

import numpy as np
import pytest

import test_rules_model as rm
from test_mask_windows import R4, R6, _fields, _stream_of

WORDS = rm.ascii_words() + rm.MULTIBYTE_WORDS                 # 76 words, bytes
OFFICE_WORDS = rm.BMP_WORDS + [rm.NON_BMP_WORD]               # the non-BMP word stands last
NON_BMP_RULES = [((":", 0, 0),), (("d", 0, 0),), (("$", ord("1"), 0),), (("c", 0, 0),)]
SPELL_MAX = 1 << 20


def _model(words, rules, start, count, office=False, trunc=None):
    """(slots, lens) as the device must write them: candidate i is rule i % R applied to word i // R."""
    limit = 32 if office else 64
    units = [rm.to_units(w, office) for w in words]
    R = len(rules)
    parts, lens = [], np.zeros(count, dtype=np.uint8)
    for k in range(count):
        w, r = divmod(start + k, R)
        u = rm.ref_units(rules[r], units[w], limit)
        b = u.encode("utf-16-le", "surrogatepass") if office else u.encode("latin-1")
        if trunc is not None:
            b = b[:trunc]
        lens[k] = len(b)
        parts.append(b.ljust(64, b"\0"))
    return np.frombuffer(b"".join(parts), dtype=np.uint8).reshape(count, 64), lens


def _same(got, want, what):
    (gs, gl), (ws, wl) = got, want
    assert gs.shape == ws.shape and gl.shape == wl.shape, what
    bad = np.flatnonzero((gl != wl) | (gs != ws).any(axis=1))
    assert bad.size == 0, (what, "%d candidates differ, the first at %d" % (bad.size, bad[0]),
                           bytes(gs[bad[0]][:int(gl[bad[0]])]), bytes(ws[bad[0]][:int(wl[bad[0]])]))


@functools.lru_cache(maxsize=None)
def matrix_model(office):
    if office:
        return _model(OFFICE_WORDS[:-1], rm.matrix_rules(True), 0, (len(OFFICE_WORDS) - 1) * len(rm.matrix_rules(True)),
                      office=True)
    return _model(WORDS, rm.matrix_rules(), 0, len(WORDS) * len(rm.matrix_rules()))


def _ctx(kind, kw=None):
    from dprf_amd import _lib
    return _lib.Context(_fields(_stream_of(kind, tuple(sorted((kw or {}).items())), "Hiver€24")), device=0)


# ------------------------------------------------------------------ preconditions (CPU)
def test_the_matrix_holds_every_function_and_both_global_rules():
    rules = rm.matrix_rules()
    assert {r[0][0] for r in rules} == set(rm.ALL_FUNCTIONS) and all(len(r) == 1 for r in rules)
    assert len(rules) >= 4500 and 300000 <= len(rules) * len(WORDS) <= SPELL_MAX
    assert sorted(len(w) for w in WORDS[:64]) == list(range(1, 65))
    assert sum(1 for w in WORDS if len(w.decode()) != len(w)) >= 12
    assert {len(ch.encode()) for w in rm.MULTIBYTE_WORDS for ch in w.decode()} == {1, 2, 3, 4}
    slots, lens = matrix_model(False)
    R = len(rules)
    changed, over, empty = set(), set(), set()
    for w, word in enumerate(WORDS):
        u = rm.to_units(word)
        for r, rule in enumerate(rules):
            fn, a, b = rule[0]
            raw = rm._TABLE[fn](u, a, b)
            got = bytes(slots[w * R + r][:int(lens[w * R + r])])
            if got != word:
                changed.add(fn)
            if raw is not None and len(raw) > 64:
                over.add(fn)
                assert got == word
            if raw is not None and len(raw) == 0:
                empty.add(fn)
                assert got == word
    assert changed == set(rm.ALL_FUNCTIONS) - {":"}
    assert over >= set("dpfqzZyY$^i") and empty >= set("[]D@xO'")
    # the 32-byte cut falls inside a multi-byte character for some result
    assert ((lens > 32) & (slots[:, 31] >= 0x80) & ((slots[:, 32] & 0xC0) == 0x80)).any()
    # Office: BMP words (a unit is a character), LIMIT 32 met and exceeded
    oslots, olens = matrix_model(True)
    assert all(len(w.decode()) * 2 == len(w.decode().encode("utf-16-le")) for w in OFFICE_WORDS[:-1])
    assert len(rm.NON_BMP_WORD.decode().encode("utf-16-le")) == 8
    assert int(olens.max()) == 64 and {len(rm.to_units(w, True)) for w in OFFICE_WORDS} >= {1, 16, 17, 31, 32}
    assert {r[0][0] for r in rm.matrix_rules(True)} == set(rm.ALL_FUNCTIONS)


# ------------------------------------------------------------------ (a) the matrix
@pytest.mark.gpu
@pytest.mark.parametrize("kw,trunc", [(R6, None), (R4, 32)], ids=["pdf-r6", "pdf-r4-cut"])
def test_matrix_on_pdf_equals_the_model(kw, trunc):
    rules = rm.matrix_rules()
    slots, lens = matrix_model(False)
    if trunc is not None:
        slots = slots.copy()
        slots[:, trunc:] = 0
        lens = np.minimum(lens, trunc).astype(np.uint8)
    with _ctx("pdf", kw) as ctx:
        ctx.set_words(WORDS)
        _same(ctx.spell_rules_raw(rules, 0, len(lens)), (slots, lens), kw)
        # the list form is the same bytes
        got = ctx.spell_rules(rules, 1000, 500)
        assert got == [bytes(slots[k][:int(lens[k])]) for k in range(1000, 1500)]
        assert ctx.last_call_devices() == []                                 # nothing was verified


@pytest.mark.gpu
def test_matrix_on_office_equals_the_model():
    rules = rm.matrix_rules(True)
    with _ctx("docx") as ctx:
        ctx.set_words(OFFICE_WORDS[:-1])
        want = matrix_model(True)
        _same(ctx.spell_rules_raw(rules, 0, len(want[1])), want, "office")
        ctx.set_words(OFFICE_WORDS)                                          # the non-BMP word: units, not characters
        base = (len(OFFICE_WORDS) - 1) * len(NON_BMP_RULES)
        _same(ctx.spell_rules_raw(NON_BMP_RULES, base, len(NON_BMP_RULES)),
              _model(OFFICE_WORDS, NON_BMP_RULES, base, len(NON_BMP_RULES), office=True), "office non-BMP")
        got = ctx.spell_rules(NON_BMP_RULES, base, len(NON_BMP_RULES))
        assert got[0] == "a\U0001D11Eb".encode("utf-16-le") and got[3] == "A\U0001D11Eb".encode("utf-16-le")


# ------------------------------------------------------------------ (b) random rule chains
@pytest.mark.gpu
def test_random_rule_chains_equal_the_model():
    rules = rm.random_rules(4096, 0xC4A1)
    assert {len(r) for r in rules} == set(range(1, 33))
    words = WORDS[:64]
    count = len(rules) * len(words)
    with _ctx("pdf", R6) as ctx:
        ctx.set_words(words)
        _same(ctx.spell_rules_raw(rules, 0, count), _model(words, rules, 0, count), "random chains")
    orules = rm.random_rules(2048, 0xC4A2, office=True)
    with _ctx("docx") as ctx:
        ctx.set_words(OFFICE_WORDS)
        n = len(orules) * len(OFFICE_WORDS)
        _same(ctx.spell_rules_raw(orules, 0, n), _model(OFFICE_WORDS, orules, 0, n, office=True), "random, office")


# ------------------------------------------------------------------ (c) window shapes
SHAPE_WORDS = [w for _ in range(5) for w in WORDS]            # 380 words: a block of 256 lanes spans many of them
SHAPE_RULES = rm.random_rules(257, 0x5A9E, lo=1, hi=3)


def shape_windows(R):
    n = len(SHAPE_WORDS) * R
    inside = 37 * R + R // 2 + (1 if (37 * R + R // 2) % 64 == 0 else 0)     # inside word 37's run (R = 1: at it)
    return [(inside, min(3000, n - inside)), (n // 2 + 1, 1), (n - 1, 1), (max(0, n - 700), min(n, 700)), (0, min(n, 600))]


def test_window_shapes_are_what_they_claim():
    for R in (1, 63, 64, 255, 256, 257):
        (s0, c0), (s1, c1), (s2, c2), (s3, c3), _ = shape_windows(R)
        assert s0 % 64 and (R == 1 or s0 % R) and c1 == 1 and s2 + c2 == len(SHAPE_WORDS) * R == s3 + c3
        assert c0 > 256 and s0 // R != (s0 + c0 - 1) // R
    assert len(BIG_WORDS) * (1 << 20) > (1 << 32) + 500 and BIG_START < 1 << 32 < BIG_START + 1000


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 63, 64, 255, 256, 257])
def test_window_shapes_equal_the_model(R):
    rules = SHAPE_RULES[:R]
    with _ctx("pdf", R6) as ctx:
        ctx.set_words(SHAPE_WORDS)
        for start, count in shape_windows(R):
            _same(ctx.spell_rules_raw(rules, start, count), _model(SHAPE_WORDS, rules, start, count), (R, start, count))


BIG_WORDS = [WORDS[(k * 7) % 58] + b"%d" % k for k in range(4200)]   # at most 58 + 4 bytes
BIG_START = (1 << 32) - 500


def big_rule_table():
    """2^20 one-function rules, encoded directly: rule k is one of eight functions with a parameter from k."""
    k = np.arange(1 << 20, dtype=np.uint32)
    which, par = k % 8, (k // 8) % 36
    unit = 0x21 + (k // 8) % 0x5e
    fns = np.select(
        [which == 0, which == 1, which == 2, which == 3, which == 4, which == 5, which == 6, which == 7],
        [ord(":") + 0 * k, ord("$") | unit << 8, ord("^") | unit << 8, ord("T") | par << 8, ord("r") + 0 * k,
         ord("D") | par << 8, ord("i") | par << 8 | unit << 16, ord("z") | (par % 4) << 8]).astype(np.uint32)
    return fns, np.arange((1 << 20) + 1, dtype=np.uint32)


@pytest.mark.gpu
def test_window_across_2_to_the_32_equals_the_model():
    from dprf_amd import rules as rulemod
    fns, off = big_rule_table()
    R = 1 << 20
    assert len(BIG_WORDS) >= 4100
    with _ctx("pdf", R6) as ctx:
        ctx.set_words(BIG_WORDS)
        got = ctx.spell_rules_raw((fns, off), BIG_START, 1000)
        parts, lens = [], []
        for i in range(BIG_START, BIG_START + 1000):
            w, r = divmod(i, R)
            rule = rulemod.decode(fns[r:r + 1], [0, 1])[0]
            b = rm.ref_apply(rule, BIG_WORDS[w])
            parts.append(b.ljust(64, b"\0"))
            lens.append(len(b))
        want = (np.frombuffer(b"".join(parts), dtype=np.uint8).reshape(1000, 64), np.array(lens, dtype=np.uint8))
        _same(got, want, "across 2^32")
        assert {i // R for i in (BIG_START, BIG_START + 999)} == {4095, 4096}
