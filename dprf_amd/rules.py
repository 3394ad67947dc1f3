"""Rule search: a wordlist with word-mangling rules ("c $1", "sa@ so0", "r").

Pure Python, no device work: the rule language, its text and compiled forms, and the model of what the device spells
(``_lib.Context.search_rules`` / ``spell_rules``, include/dprf.h "rule mode").

A rule is 1..32 functions applied left to right to a word.  A word is a sequence of *units*: a byte of the word as
given (ODF, PDF), or a UTF-16 code unit of the converted word (Office).  ``LIMIT`` is 64 units (32 for Office): the
64-byte list slot.  Two rules hold for every function: one whose result would be longer than ``LIMIT`` leaves the
candidate unchanged, and so does one whose result would be empty -- every candidate keeps 1..LIMIT units and no NUL.
Case functions touch ASCII letters only.  The functions are hashcat's of the same names (``: l u c C t TN E r d pN f {
} q k K *NM $X ^X [ ] DN xNM ONM iNX oNX 'N zN ZN yN YN sXY @X .N ,N``); reject, memory and arithmetic functions are
not part of the language.

Candidate ``i`` of the keyspace N * R is rule ``i % R`` applied to word ``i // R``: the word is the slowest digit.
"""
import itertools

MAX_RULES = 1 << 20
MAX_RULE_FNS = 32
MAX_RULE_WORDS = 1 << 22
LIMIT, LIMIT_OFFICE = 64, 32

POSITIONS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
# function -> its parameters: N / M positions, X / Y units
SIGNATURE = {}
for _f in ":lucCtErdf{}qkK[]":
    SIGNATURE[_f] = ""
for _f in "TpD'zZyY.,":
    SIGNATURE[_f] = "N"
for _f in "*xO":
    SIGNATURE[_f] = "NM"
for _f in "$^@":
    SIGNATURE[_f] = "X"
for _f in "io":
    SIGNATURE[_f] = "NX"
SIGNATURE["s"] = "XY"
del _f


class RuleError(ValueError):
    """A rule the language does not hold: `fn` the function (or None), `column` where it stands in the line."""

    def __init__(self, msg, fn=None, column=None):
        super().__init__(msg)
        self.fn, self.column = fn, column


def _line_bytes(line):
    if isinstance(line, str):
        return line.encode("utf-8", "surrogateescape")
    return bytes(line)


def parse_rule(line):
    """One line of rule text -> a tuple of functions (fn, p1, p2): fn the function's character, positions as their
    values 0..35, units as ints 1..255, absent parameters 0.  Blanks between functions are skipped; a parameter is the
    character right after its function ("$ " appends a space).  Raises RuleError naming the function and its column
    for anything outside the language, an empty rule or one of more than 32 functions."""
    raw = _line_bytes(line).rstrip(b"\r\n")
    out, i = [], 0
    while i < len(raw):
        ch = raw[i:i + 1]
        if ch in b" \t":
            i += 1
            continue
        fn = ch.decode("latin-1")
        sig = SIGNATURE.get(fn)
        if sig is None:
            raise RuleError("function %r at column %d is not part of the rule language" % (fn, i), fn, i)
        if i + 1 + len(sig) > len(raw):
            raise RuleError("function %r at column %d lacks a parameter" % (fn, i), fn, i)
        ps = [0, 0]
        for k, kind in enumerate(sig):
            b = raw[i + 1 + k]
            if kind in "NM":
                v = POSITIONS.find(chr(b)) if b < 0x80 else -1
                if v < 0:
                    raise RuleError("function %r at column %d: position %r is not one of 0-9A-Z" % (fn, i, chr(b)), fn, i)
                ps[k] = v
            else:
                if b == 0:
                    raise RuleError("function %r at column %d: NUL cannot be a unit" % (fn, i), fn, i)
                ps[k] = b
        out.append((fn, ps[0], ps[1]))
        i += 1 + len(sig)
    if not out:
        raise RuleError("an empty rule")
    if len(out) > MAX_RULE_FNS:
        raise RuleError("a rule of %d functions (at most %d)" % (len(out), MAX_RULE_FNS))
    return tuple(out)


def format_rule(rule):
    """The text form of a parsed rule, as bytes (a unit may be any byte)."""
    out = []
    for fn, p1, p2 in rule:
        ps = (p1, p2)
        out.append(fn.encode("latin-1") + b"".join(
            POSITIONS[ps[k]].encode() if kind in "NM" else bytes([ps[k]]) for k, kind in enumerate(SIGNATURE[fn])))
    return b" ".join(out)


def parse_rules(lines):
    """Lines of rule text -> (rules, skipped): lines that are empty or start with '#' are passed over, lines the
    language does not hold are counted in `skipped`."""
    rules, skipped = [], 0
    for line in lines:
        raw = _line_bytes(line).rstrip(b"\r\n")
        if not raw.strip(b" \t") or raw.startswith(b"#"):
            continue
        try:
            rules.append(parse_rule(raw))
        except RuleError:
            skipped += 1
    return rules, skipped


def read_rules(path):
    """The rules of a rule file and the number of lines skipped as unsupported."""
    with open(path, "rb") as f:
        return parse_rules(f.read().split(b"\n"))


def product(a, b):
    """Every rule of `a` followed by every rule of `b`, `a` slowest -> (rules, dropped): products of more than 32
    functions are dropped and counted."""
    out, dropped = [], 0
    for x, y in itertools.product(a, b):
        if len(x) + len(y) > MAX_RULE_FNS:
            dropped += 1
        else:
            out.append(tuple(x) + tuple(y))
    return out, dropped


def encode(rules):
    """Parsed rules -> (fns, rule_off): numpy uint32 arrays, one word per function (the function's ASCII character in
    bits 0-7, the first parameter in bits 8-15, the second in bits 16-23) and len(rules) + 1 offsets into them."""
    import numpy as np
    fns, off = [], [0]
    for r in rules:
        for fn, p1, p2 in r:
            fns.append(ord(fn) | (int(p1) & 0xff) << 8 | (int(p2) & 0xff) << 16)
        off.append(len(fns))
    return np.asarray(fns, dtype=np.uint32), np.asarray(off, dtype=np.uint32)


def decode(fns, rule_off):
    """The inverse of :func:`encode`."""
    fns = [int(x) for x in fns]
    off = [int(x) for x in rule_off]
    return [tuple((chr(w & 0xff), (w >> 8) & 0xff, (w >> 16) & 0xff) for w in fns[off[k]:off[k + 1]])
            for k in range(len(off) - 1)]


def _letter(v):
    return 0x41 <= v <= 0x5a or 0x61 <= v <= 0x7a


def _lower(v):
    return v | 0x20 if 0x41 <= v <= 0x5a else v


def _upper(v):
    return v & ~0x20 if 0x61 <= v <= 0x7a else v


def _toggle(v):
    return v ^ 0x20 if _letter(v) else v


def _apply_fn(w, fn, a, b):
    """One function on the unit list `w`: the result, before the two global rules."""
    n = len(w)
    if fn == ":":
        return w
    if fn == "l":
        return [_lower(v) for v in w]
    if fn == "u":
        return [_upper(v) for v in w]
    if fn == "c":
        return [_upper(w[0])] + [_lower(v) for v in w[1:]]
    if fn == "C":
        return [_lower(w[0])] + [_upper(v) for v in w[1:]]
    if fn == "t":
        return [_toggle(v) for v in w]
    if fn == "T":
        return w[:a] + [_toggle(w[a])] + w[a + 1:] if a < n else w
    if fn == "E":
        out = [_lower(v) for v in w]
        for j in range(n):
            if j == 0 or out[j - 1] == 0x20:
                out[j] = _upper(out[j])
        return out
    if fn == "r":
        return w[::-1]
    if fn == "d":
        return w + w
    if fn == "p":
        return w * (a + 1)
    if fn == "f":
        return w + w[::-1]
    if fn == "{":
        return w[1:] + w[:1]
    if fn == "}":
        return w[-1:] + w[:-1]
    if fn == "q":
        return [v for v in w for _ in (0, 1)]
    if fn == "k":
        return [w[1], w[0]] + w[2:] if n >= 2 else w
    if fn == "K":
        return w[:-2] + [w[-1], w[-2]] if n >= 2 else w
    if fn == "*":
        if a < n and b < n:
            w = list(w)
            w[a], w[b] = w[b], w[a]
        return w
    if fn == "$":
        return w + [a]
    if fn == "^":
        return [a] + w
    if fn == "[":
        return w[1:]
    if fn == "]":
        return w[:-1]
    if fn == "D":
        return w[:a] + w[a + 1:] if a < n else w
    if fn == "x":
        return w[a:a + b] if a + b <= n else w
    if fn == "O":
        return w[:a] + w[a + b:] if a + b <= n else w
    if fn == "i":
        return w[:a] + [b] + w[a:] if a <= n else w
    if fn == "o":
        return w[:a] + [b] + w[a + 1:] if a < n else w
    if fn == "'":
        return w[:a] if a < n else w
    if fn == "z":
        return w[:1] * a + w
    if fn == "Z":
        return w + w[-1:] * a
    if fn == "y":
        return w[:a] + w if a <= n else w
    if fn == "Y":
        return w + w[n - a:] if a <= n else w
    if fn == "s":
        return [b if v == a else v for v in w]
    if fn == "@":
        return [v for v in w if v != a]
    if fn == ".":
        return w[:a] + [w[a + 1]] + w[a + 1:] if a + 1 < n else w
    if fn == ",":
        return w[:a] + [w[a - 1]] + w[a + 1:] if 1 <= a < n else w
    raise RuleError("function %r is not part of the rule language" % fn, fn)


def _units(word, office):
    if isinstance(word, str):
        word = word.encode("utf-8", "surrogateescape")
    word = bytes(word)
    if not office:
        return list(word)
    u = word.decode("utf-8").encode("utf-16-le")
    return [u[k] | u[k + 1] << 8 for k in range(0, len(u), 2)]


def _pack(units, office):
    if not office:
        return bytes(units)
    return b"".join(bytes((v & 0xff, v >> 8)) for v in units)


def apply(rule, word, office=False, trunc=None):
    """`rule` applied to `word` (bytes; Office: UTF-8, converted first) -> the candidate's bytes (Office: UTF-16LE),
    cut at `trunc` bytes when given (the format's truncation applies to the result).  The word itself must hold
    1..LIMIT units."""
    limit = LIMIT_OFFICE if office else LIMIT
    w = _units(word, office)
    if not 1 <= len(w) <= limit:
        raise ValueError("a word of %d units (1..%d)" % (len(w), limit))
    for fn, a, b in rule:
        if office and ("X" in SIGNATURE[fn] or "Y" in SIGNATURE[fn]):
            for kind, v in zip(SIGNATURE[fn], (a, b)):
                if kind in "XY" and v >= 0x80:
                    raise RuleError("Office takes the units 0x01..0x7F (function %r has 0x%02X)" % (fn, v), fn)
        out = _apply_fn(w, fn, a, b)
        if 1 <= len(out) <= limit:
            w = out
    out = _pack(w, office)
    return out if trunc is None else out[:trunc]


def space(nwords, nrules):
    """The keyspace: words times rules, as an exact int."""
    return int(nwords) * int(nrules)


def candidate(words, rules, index, office=False, trunc=None):
    """Candidate `index` as bytes: rule index % R applied to word index // R."""
    if not 0 <= index < len(words) * len(rules):
        raise IndexError("index %d outside the rule keyspace" % index)
    w, r = divmod(index, len(rules))
    return apply(rules[r], words[w], office, trunc)


def index_of(words, rules, password, office=False, trunc=None):
    """The lowest keyspace index that spells `password` (bytes, or a str: its UTF-8, for Office its UTF-16LE);
    ValueError when none does."""
    if isinstance(password, str):
        password = password.encode("utf-16-le" if office else "utf-8", "surrogateescape" if not office else "strict")
    password = bytes(password) if trunc is None else bytes(password)[:trunc]
    for w, word in enumerate(words):
        for r, rule in enumerate(rules):
            if apply(rule, word, office, trunc) == password:
                return w * len(rules) + r
    raise ValueError("no word and rule spell %r" % (password,))


__all__ = ["MAX_RULES", "MAX_RULE_FNS", "MAX_RULE_WORDS", "LIMIT", "LIMIT_OFFICE", "RuleError", "parse_rule",
           "parse_rules", "read_rules", "format_rule", "product", "encode", "decode", "apply", "space", "candidate",
           "index_of"]
