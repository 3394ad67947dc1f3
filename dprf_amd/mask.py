"""The mask language: a set of characters per password position ("?u?l?l?l?l?l?d?d", "Inv-?d?d?d?d€").

Pure Python, no device work.  :func:`parse_mask` turns a mask into a list of per-position strings, each string that
position's characters in enumeration order; ``_lib.Context.search_mask`` enumerates their product on the device in
``itertools.product`` order, the last position fastest, so a mask with the same set at every position enumerates
exactly as range mode does.

Tokens: ``?l`` a-z, ``?u`` A-Z, ``?d`` 0-9, ``?h`` 0-9a-f, ``?H`` 0-9A-F, ``?s`` the 33 printable ASCII characters that
are neither letters nor digits (space included) in ASCII order, ``?a`` = ``?l?u?d?s``, ``?1`` .. ``?4`` the custom sets,
``??`` a literal ``?``; any other character is a literal.  A custom set is written in the same language and is the
union of its tokens in order (``?l?d_`` is a-z, 0-9 and ``_``); it may not name another custom set.  ``?b`` (all 256
bytes) is refused: it contains NUL, which no argv string can carry to a verifier.
"""
from . import _lib

LOWER = "abcdefghijklmnopqrstuvwxyz"
UPPER = LOWER.upper()
DIGITS = "0123456789"
SPECIAL = " !\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"
BUILTIN = {"l": LOWER, "u": UPPER, "d": DIGITS, "h": DIGITS + "abcdef", "H": DIGITS + "ABCDEF", "s": SPECIAL,
           "a": LOWER + UPPER + DIGITS + SPECIAL}
MAX_CUSTOM = 4


def _refuse(msg):
    raise _lib.DprfError(_lib.E_CHARSET, msg)


def _tokens(text, custom, where):
    """The sets `text` spells, one string per token; `where` names the text in messages ("mask" or "custom set 2").
    custom: the parsed custom sets, or None inside a custom set."""
    if not isinstance(text, str):
        _refuse("%s must be a str (got %s)" % (where, type(text).__name__))
    out, i = [], 0
    while i < len(text):
        ch = text[i]
        at = "%s position %d" % (where, len(out))
        if ch == "\0":
            _refuse("%s: NUL (argv cannot carry it)" % at)
        if ch != "?":
            out.append(ch)
            i += 1
            continue
        if i + 1 == len(text):
            _refuse("%s: trailing '?' (write '??' for a literal question mark)" % at)
        t = text[i + 1]
        i += 2
        if t == "?":
            out.append("?")
        elif t in BUILTIN:
            out.append(BUILTIN[t])
        elif t == "b":
            _refuse("%s: ?b contains NUL, which argv cannot carry" % at)
        elif t in "1234":
            if custom is None:
                _refuse("%s: a custom set may not contain the custom token ?%s" % (at, t))
            if int(t) > len(custom) or custom[int(t) - 1] is None:
                _refuse("%s: custom set ?%s is not defined" % (at, t))
            out.append(custom[int(t) - 1])
        else:
            _refuse("%s: unknown token ?%s" % (at, t))
    return out


def _check_set(chars, where):
    if len(set(chars)) != len(chars):
        dup = next(c for c in chars if chars.count(c) > 1)
        _refuse("%s repeats %r (its candidates would be verified twice)" % (where, dup))
    try:
        chars.encode("utf-8")
    except UnicodeEncodeError as e:   # lone surrogates
        _refuse("%s is not encodable as UTF-8: %s" % (where, e))
    return chars


def parse_mask(mask, custom=()):
    """mask -> list of per-position strings.  custom: up to four custom sets (?1 .. ?4) in the mask language; None or
    "" leaves a set undefined.  Raises DprfError(E_CHARSET) with a message naming the position."""
    custom = list(custom or ())
    if len(custom) > MAX_CUSTOM:
        _refuse("%d custom sets (at most %d: ?1 .. ?%d)" % (len(custom), MAX_CUSTOM, MAX_CUSTOM))
    sets = []
    for k, text in enumerate(custom):
        if not text:
            sets.append(None)
            continue
        where = "custom set %d" % (k + 1)
        sets.append(_check_set("".join(_tokens(text, None, where)), where))
    positions = _tokens(mask, sets, "mask")
    if not positions:
        _refuse("empty mask")
    return [_check_set(p, "mask position %d" % k) for k, p in enumerate(positions)]


def space(positions):
    """The keyspace: the product of the positions' set sizes, as an exact int."""
    n = 1
    for p in positions:
        n *= len(p)
    return n


def word(positions, index):
    """Candidate `index` of the mask, itertools.product order: the last position varies fastest."""
    if not 0 <= index < space(positions):
        raise IndexError("index %d outside the mask's keyspace" % index)
    out = []
    for p in reversed(positions):
        index, r = divmod(index, len(p))
        out.append(p[r])
    return "".join(reversed(out))


def index_of(positions, password):
    """The keyspace index of `password`; ValueError when the mask does not spell it."""
    if len(password) != len(positions):
        raise ValueError("%r has %d characters, the mask %d positions" % (password, len(password), len(positions)))
    i = 0
    for p, ch in zip(positions, password):
        i = i * len(p) + p.index(ch)
    return i
