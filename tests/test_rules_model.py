"""The rule language (dprf_amd/rules.py, include/dprf.h "rule mode") without a device: the pinned examples of
tests/golden/rule_examples.json, and rules.apply against this file's own plain implementation of the language's table
(`ref_apply`, written from the table alone) over the matrix the device test spells (test_rules_spell.py imports it
from here) and over 20,000 random rules.  Also the text form (blanks, "$ ", '#' lines, unsupported functions counted),
rules.product with its 32-function drop, and encode round trips."""
import json
import os
import random

import pytest

from conftest import REPO

POS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
NOPARAM = ":lucCtErdf{}qkK[]"
ONEPOS = "TpD'zZyY.,"
TWOPOS = "*xO"
ONEUNIT = "$^@"
POSUNIT = "io"
ALL_FUNCTIONS = NOPARAM + ONEPOS + TWOPOS + ONEUNIT + POSUNIT + "s"


# ------------------------------------------------------------------ this file's own implementation of the table
# A candidate is a str with one character per unit (chr of the byte, or of the UTF-16 code unit: a lone surrogate is a
# character like any other), so the table's slices are str slices.  Case goes through ASCII-only translation tables.
_LOW = {c: c + 32 for c in range(65, 91)}
_UP = {c: c - 32 for c in range(97, 123)}
_TOG = {**_LOW, **_UP}


def _title(w, a, b):
    out, up = [], True
    for ch in w.translate(_LOW):
        out.append(ch.translate(_UP) if up else ch)
        up = ch == " "
    return "".join(out)


def _swap(w, i, j):
    u = list(w)
    u[i], u[j] = u[j], u[i]
    return "".join(u)


# fn -> (w, a, b) -> the table's result, or None where the row's condition does not hold
_TABLE = {
    ":": lambda w, a, b: w,
    "l": lambda w, a, b: w.translate(_LOW),
    "u": lambda w, a, b: w.translate(_UP),
    "c": lambda w, a, b: w[:1].translate(_UP) + w[1:].translate(_LOW),
    "C": lambda w, a, b: w[:1].translate(_LOW) + w[1:].translate(_UP),
    "t": lambda w, a, b: w.translate(_TOG),
    "T": lambda w, a, b: w[:a] + w[a].translate(_TOG) + w[a + 1:] if a < len(w) else None,
    "E": _title,
    "r": lambda w, a, b: w[::-1],
    "d": lambda w, a, b: w + w,
    "p": lambda w, a, b: w * (a + 1),
    "f": lambda w, a, b: w + w[::-1],
    "{": lambda w, a, b: w[1:] + w[0],
    "}": lambda w, a, b: w[-1] + w[:-1],
    "q": lambda w, a, b: "".join(ch + ch for ch in w),
    "k": lambda w, a, b: _swap(w, 0, 1) if len(w) >= 2 else None,
    "K": lambda w, a, b: _swap(w, len(w) - 2, len(w) - 1) if len(w) >= 2 else None,
    "*": lambda w, a, b: _swap(w, a, b) if a < len(w) and b < len(w) else None,
    "$": lambda w, a, b: w + chr(a),
    "^": lambda w, a, b: chr(a) + w,
    "[": lambda w, a, b: w[1:],
    "]": lambda w, a, b: w[:-1],
    "D": lambda w, a, b: w[:a] + w[a + 1:] if a < len(w) else None,
    "x": lambda w, a, b: w[a:a + b] if a + b <= len(w) else None,
    "O": lambda w, a, b: w[:a] + w[a + b:] if a + b <= len(w) else None,
    "i": lambda w, a, b: w[:a] + chr(b) + w[a:] if a <= len(w) else None,
    "o": lambda w, a, b: w[:a] + chr(b) + w[a + 1:] if a < len(w) else None,
    "'": lambda w, a, b: w[:a] if a < len(w) else None,
    "z": lambda w, a, b: w[0] * a + w,
    "Z": lambda w, a, b: w + w[-1] * a,
    "y": lambda w, a, b: w[:a] + w if a <= len(w) else None,
    "Y": lambda w, a, b: w + w[len(w) - a:] if a <= len(w) else None,
    "s": lambda w, a, b: w.replace(chr(a), chr(b)),
    "@": lambda w, a, b: w.replace(chr(a), ""),
    ".": lambda w, a, b: w[:a] + w[a + 1] + w[a + 1:] if a + 1 < len(w) else None,
    ",": lambda w, a, b: w[:a] + w[a - 1] + w[a + 1:] if 1 <= a < len(w) else None,
}


def to_units(word, office=False):
    if not office:
        return word.decode("latin-1")
    raw = word.decode("utf-8").encode("utf-16-le")
    return "".join(chr(raw[k] + 256 * raw[k + 1]) for k in range(0, len(raw), 2))


def ref_units(rule, w, limit):
    """`rule` (a sequence of (fn, p1, p2)) on the unit string w, with the two global rules."""
    for fn, a, b in rule:
        got = _TABLE[fn](w, a, b)
        if got is not None and 1 <= len(got) <= limit:
            w = got
    return w


def ref_apply(rule, word, office=False, trunc=None):
    """`rule` applied to `word` (bytes) -> bytes; Office: over UTF-16 code units, returned as UTF-16LE."""
    w = to_units(word, office)
    assert 1 <= len(w) <= (32 if office else 64)
    w = ref_units(rule, w, 32 if office else 64)
    out = w.encode("utf-16-le", "surrogatepass") if office else w.encode("latin-1")
    return out if trunc is None else out[:trunc]


def fn_of(text):
    """One function in text form -> (fn, p1, p2), by this file's reading of the notation."""
    fn, ps = text[0], text[1:]
    if fn in NOPARAM:
        assert ps == ""
        return (fn, 0, 0)
    if fn in ONEPOS:
        return (fn, POS.index(ps), 0)
    if fn in TWOPOS:
        return (fn, POS.index(ps[0]), POS.index(ps[1]))
    raw = ps.encode("latin-1")
    if fn in ONEUNIT:
        return (fn, raw[0], 0)
    if fn in POSUNIT:
        return (fn, POS.index(ps[0]), raw[1])
    assert fn == "s"
    return (fn, raw[0], raw[1])


# ------------------------------------------------------------------ the matrix (shared with test_rules_spell.py)
_FILL = "aB3 dEf9gHH1 jKl  mN0pQrsT7uVwXyZz"


def ascii_words():
    """One word of every length 1..64: mixed case, digits, blanks and repeated characters (never a blank at either
    end of the pattern's period, so a blank also stands inside words)."""
    out = []
    for n in range(1, 65):
        s = (_FILL[(n - 1) % 7:] + _FILL) * 3
        out.append(s[:n].encode())
    return out


MULTIBYTE_WORDS = [w.encode() for w in (
    "é", "€", "\U0001D11E", "aé", "Zß€", "x\U0001D11Ey", "ééé€€€", "Hiver€", "ÀbcÉ d", "€uro Sign€", "αβγ δ",
    "q\U00020000Q\U0001F600")]
BMP_WORDS = [w.encode() for w in (
    "a", "Zé", "aB3 dEf9", "Hiver€", "αβγ δεζ", "€€€€€€€€€€€€€€€€", "x" * 31, "Yz" * 16, "p@ssW0rd w0rld", "é" * 17,
    "A€b" * 5 + "q", "mN0pQrsT7uVwXyZz aB3 dEf9gHH1 j")]
NON_BMP_WORD = "a\U0001D11Eb".encode()
UNITS = [ord("a"), ord(" "), ord("H"), ord("#"), 0xFF]       # '#' is in no word; 0xFF only as a byte unit
UNITS_OFFICE = [ord("a"), ord(" "), ord("H"), ord("#"), 0x7F]


def matrix_rules(office=False):
    """Every parameterless function, every one-position function at every N, x / O / * at every (N, M), and the unit
    functions over a few units: one function per rule."""
    units = UNITS_OFFICE if office else UNITS
    out = [((f, 0, 0),) for f in NOPARAM]
    out += [((f, n, 0),) for f in ONEPOS for n in range(36)]
    out += [((f, n, m),) for f in TWOPOS for n in range(36) for m in range(36)]
    out += [((f, x, 0),) for f in ONEUNIT for x in units]
    out += [((f, n, x),) for f in POSUNIT for n in range(36) for x in units]
    out += [(("s", x, y),) for x in units for y in units if x != y]
    return out


def random_rules(count, seed, office=False, lo=1, hi=32):
    rng = random.Random(seed)
    top = 0x7F if office else 0xFF
    out = []
    for _ in range(count):
        rule = []
        for _ in range(rng.randint(lo, hi)):
            f = rng.choice(ALL_FUNCTIONS)
            n, m = rng.choice((0, 1, 2, 3, 5, 8, rng.randrange(36))), rng.choice((0, 1, 2, 4, rng.randrange(36)))
            x = rng.choice((97, 101, 32, 72, 48, rng.randint(1, top)))
            y = rng.choice((64, 65, 51, rng.randint(1, top)))
            if f in NOPARAM:
                rule.append((f, 0, 0))
            elif f in ONEPOS:
                rule.append((f, n, 0))
            elif f in TWOPOS:
                rule.append((f, n, m))
            elif f in ONEUNIT:
                rule.append((f, x, 0))
            elif f in POSUNIT:
                rule.append((f, n, x))
            else:
                rule.append((f, x, y))
        out.append(tuple(rule))
    return out


# ------------------------------------------------------------------ tests
def _examples():
    with open(os.path.join(REPO, "tests", "golden", "rule_examples.json"), encoding="utf-8") as f:
        return json.load(f)["rows"]


def _want(row):
    return row["result"].encode("utf-16-le" if row["office"] else "utf-8")


def test_pinned_examples_hold_for_the_module_and_for_this_files_implementation():
    from dprf_amd import rules
    rows = _examples()
    assert len([r for r in rows if r["group"] == "documented"]) == 70 and len(rows) >= 190
    assert {r["rule"][0] for r in rows} == set(ALL_FUNCTIONS) - {":"}
    for row in rows:
        rule = rules.parse_rule(row["rule"])
        assert len(rule) == 1 and rule[0] == fn_of(row["rule"]), row
        word = row["word"].encode()
        assert rules.apply(rule, word, office=row["office"]) == _want(row), row
        assert ref_apply(rule, word, office=row["office"]) == _want(row), row


def test_edge_rows_meet_and_exceed_the_limit():
    rows = [r for r in _examples() if r["group"] == "LIMIT"]
    for office, limit in ((False, 64), (True, 32)):
        mine = [r for r in rows if r["office"] == office]
        grown = [r for r in mine if r["result"] != r["word"]]
        kept = [r for r in mine if r["result"] == r["word"]]
        assert {len(r["result"]) for r in grown} >= {limit} and max(len(r["result"]) for r in grown) == limit
        for f in ("d", "p1", "q", "$!", "z1", "i0!"):
            assert any(r["rule"] == f and len(r["result"]) == limit for r in grown), (office, f)
            assert any(r["rule"] == f for r in kept), (office, f)


def test_apply_equals_this_files_implementation_over_the_matrix():
    from dprf_amd import rules
    words = ascii_words() + MULTIBYTE_WORDS
    for rule in matrix_rules():
        for w in words:
            assert rules.apply(rule, w) == ref_apply(rule, w), (rule, w)
    for rule in matrix_rules(office=True):
        for w in BMP_WORDS + [NON_BMP_WORD]:
            assert rules.apply(rule, w, office=True) == ref_apply(rule, w, office=True), (rule, w)


def test_apply_equals_this_files_implementation_over_random_rules():
    from dprf_amd import rules
    words = ascii_words() + MULTIBYTE_WORDS
    rng = random.Random(0x2017)
    for k, rule in enumerate(random_rules(20000, 0x2016)):
        assert 1 <= len(rule) <= 32
        w = rng.choice(words)
        got = rules.apply(rule, w)
        assert got == ref_apply(rule, w), (rule, w)
        assert 1 <= len(got) <= 64 and 0 not in got
    for rule in random_rules(4000, 0x2018, office=True):
        w = rng.choice(BMP_WORDS + [NON_BMP_WORD])
        got = rules.apply(rule, w, office=True)
        assert got == ref_apply(rule, w, office=True), (rule, w)
        assert 2 <= len(got) <= 64 and len(got) % 2 == 0


def test_parser_text_form():
    from dprf_amd import rules
    assert rules.parse_rule("c $1") == (("c", 0, 0), ("$", ord("1"), 0))
    assert rules.parse_rule("  c\t$1  ") == rules.parse_rule("c$1")
    assert rules.parse_rule("$ ") == (("$", 32, 0),)                        # the parameter is the next character
    assert rules.parse_rule("$ $ ") == (("$", 32, 0), ("$", 32, 0))
    assert rules.parse_rule("s a") == (("s", 32, ord("a")),)
    assert rules.parse_rule("xAZ *09 i1 ") == (("x", 10, 35, ), ("*", 0, 9), ("i", 1, 32))
    assert rules.parse_rule(b"$\xff o0\x80") == (("$", 255, 0), ("o", 0, 128))
    assert rules.parse_rule("sa@ so0 r\r\n") == (("s", 97, 64), ("s", 111, 48), ("r", 0, 0))
    assert rules.parse_rule(":" * 32) == ((":", 0, 0),) * 32
    for text, fn, col in (("c +0", "+", 2), ("l L1", "L", 2), ("<5", "<", 0), ("u M", "M", 2), ("r -2", "-", 2),
                          ("$1 R0", "R", 3), ("Ta", "T", 0), ("x1", "x", 0), ("c $", "$", 2), ("i5", "i", 0)):
        with pytest.raises(rules.RuleError) as ei:
            rules.parse_rule(text)
        assert ei.value.fn == fn and ei.value.column == col, (text, ei.value)
        assert repr(fn) in str(ei.value) and "column %d" % col in str(ei.value)
    for text in ("", "   ", ":" * 33):
        with pytest.raises(rules.RuleError):
            rules.parse_rule(text)
    for rule in matrix_rules() + random_rules(300, 5):
        assert rules.parse_rule(rules.format_rule(rule)) == rule


def test_rule_files(tmp_path):
    from dprf_amd import rules
    path = tmp_path / "some.rule"
    path.write_bytes(b"# a comment\n:\n\nc $1\r\n   \n#l\nu +0\n$ \nsa@ so0\n<8 l\nM\nr")
    got, skipped = rules.read_rules(str(path))
    assert skipped == 3                                                     # "u +0", "<8 l" and "M"
    assert got == [rules.parse_rule(t) for t in (":", "c $1", "$ ", "sa@ so0", "r")]
    assert rules.parse_rules([]) == ([], 0)


def test_product_and_its_drop():
    from dprf_amd import rules
    a = [rules.parse_rule(t) for t in ("c", "u $1", ":" * 30)]
    b = [rules.parse_rule(t) for t in ("$1 $2", "r", "l l l")]
    got, dropped = rules.product(a, b)
    assert dropped == 1                                                     # 30 + 3 functions
    assert got == [a[0] + b[0], a[0] + b[1], a[0] + b[2], a[1] + b[0], a[1] + b[1], a[1] + b[2], a[2] + b[0],
                   a[2] + b[1]]
    assert max(len(r) for r in got) == 32
    for w in (b"hello", b"X"):
        for x in a:
            for y in b:
                if len(x) + len(y) <= 32:
                    assert rules.apply(x + y, w) == rules.apply(y, rules.apply(x, w))


def test_encode_round_trips():
    import numpy as np
    from dprf_amd import rules
    rs = matrix_rules() + random_rules(500, 9)
    fns, off = rules.encode(rs)
    assert fns.dtype == np.uint32 and off.dtype == np.uint32 and len(off) == len(rs) + 1
    assert int(off[0]) == 0 and int(off[-1]) == len(fns) == sum(len(r) for r in rs)
    assert rules.decode(fns, off) == rs
    one, o = rules.encode([rules.parse_rule("sa@ x3Z $\xff".encode("latin-1"))])
    assert [int(v) for v in one] == [ord("s") | 97 << 8 | 64 << 16, ord("x") | 3 << 8 | 35 << 16, ord("$") | 255 << 8]
    assert [int(v) for v in o] == [0, 3]
    assert int(fns.max()) < 1 << 24


def test_keyspace_model():
    from dprf_amd import rules
    words = [b"sun", b"moon", "Hiver€".encode()]
    rs = [rules.parse_rule(t) for t in (":", "c $1", "r", "$2 $4")]
    assert rules.space(len(words), len(rs)) == 12
    got = [rules.candidate(words, rs, i) for i in range(12)]
    assert got[:5] == [b"sun", b"Sun1", b"nus", b"sun24", b"moon"]          # the word is the slowest digit
    assert got[11] == "Hiver€24".encode() and rules.index_of(words, rs, "Hiver€24") == 11
    assert rules.candidate(words, rs, 11, office=True) == "Hiver€24".encode("utf-16-le")
    assert rules.index_of(words, rs, "Moon1", office=True) == 5
    assert rules.candidate(words, rs, 11, trunc=6) == "Hiver€24".encode()[:6]
    with pytest.raises(IndexError):
        rules.candidate(words, rs, 12)
    with pytest.raises(ValueError):
        rules.index_of(words, rs, "nothing")
