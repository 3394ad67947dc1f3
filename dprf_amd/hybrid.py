"""Hybrid search: a wordlist with a mask around each word ("?w?d?d", "?d?d?d?d-?w", "Inv-?w-?d?d").

Pure Python, no device work.  The language is the mask language (:mod:`dprf_amd.mask`) plus ``?w``, the word, which
must appear exactly once in the mask and never in a custom set.  :func:`parse_hybrid` returns the mask's positions
without the word and ``word_at``, the number of positions spelled before it (0 prepends the word, ``len(positions)``
appends it).  ``_lib.Context.search_hybrid`` enumerates words x mask on the device: candidate ``i`` is word
``i // M`` with mask index ``i % M`` (``M`` the mask's keyspace, 1 for the bare ``?w``), the mask's last position
fastest and the word the slowest digit wherever it is spelled.

Words are bytes, in file order; duplicates stay (they are verified twice).
"""
from . import mask as masks


def _word_tokens(text):
    """Offsets of the ``?w`` tokens of `text`, read token by token ("??w" is a literal '?' and a literal 'w')."""
    at, i = [], 0
    while i < len(text):
        if text[i] == "?" and i + 1 < len(text):
            if text[i + 1] == "w":
                at.append(i)
            i += 2
        else:
            i += 1
    return at


def parse_hybrid(mask, custom=()):
    """mask with exactly one ``?w`` -> (positions, word_at): the per-position strings of mask.parse_mask for the mask
    without the word, and how many of them are spelled before the word.  Raises DprfError(E_CHARSET)."""
    if not isinstance(mask, str):
        masks._refuse("mask must be a str (got %s)" % type(mask).__name__)
    custom = list(custom or ())
    if len(custom) > masks.MAX_CUSTOM:
        masks._refuse("%d custom sets (at most %d: ?1 .. ?%d)" % (len(custom), masks.MAX_CUSTOM, masks.MAX_CUSTOM))
    sets = []
    for k, text in enumerate(custom):
        if not text:
            sets.append(None)
            continue
        where = "custom set %d" % (k + 1)
        if isinstance(text, str) and _word_tokens(text):
            masks._refuse("%s: ?w is the wordlist's word and cannot be part of a set" % where)
        sets.append(masks._check_set("".join(masks._tokens(text, None, where)), where))
    at = _word_tokens(mask)
    if not at:
        masks._refuse("a hybrid mask needs ?w, the place of the wordlist's word (\"?w?d?d\")")
    if len(at) > 1:
        masks._refuse("?w appears %d times in the mask (exactly once: one word per candidate)" % len(at))
    before = masks._tokens(mask[:at[0]], sets, "mask")
    after = masks._tokens(mask[at[0] + 2:], sets, "mask after ?w")
    positions = [masks._check_set(p, "mask position %d" % k) for k, p in enumerate(before + after)]
    return positions, len(before)


def space(nwords, positions):
    """The keyspace: words times the product of the positions' set sizes, as an exact int."""
    return int(nwords) * masks.space(positions)


def _bytes(word):
    return word.encode("utf-8", "surrogateescape") if isinstance(word, str) else bytes(word)


def candidate(words, positions, word_at, index):
    """Candidate `index` as bytes: word index // M spelled before mask position `word_at` of mask index % M."""
    m = masks.space(positions)
    if not 0 <= index < len(words) * m:
        raise IndexError("index %d outside the hybrid keyspace" % index)
    w, r = divmod(index, m)
    chars = masks.word(positions, r) if positions else ""
    return chars[:word_at].encode("utf-8") + _bytes(words[w]) + chars[word_at:].encode("utf-8")


def index_of(words, positions, word_at, password):
    """The lowest keyspace index that spells `password` (bytes or str); ValueError when none does."""
    pw = _bytes(password).decode("utf-8", "surrogateescape")
    n = len(positions)
    if len(pw) <= n:
        raise ValueError("%r is no longer than the mask's %d positions" % (password, n))
    tail = n - word_at
    chars = pw[:word_at] + (pw[len(pw) - tail:] if tail else "")
    word = pw[word_at:len(pw) - tail].encode("utf-8", "surrogateescape")
    words = [_bytes(w) for w in words]
    return words.index(word) * masks.space(positions) + (masks.index_of(positions, chars) if positions else 0)


def read_wordlist(path):
    """The words of a wordlist file, as bytes in file order: one per line, a trailing CR stripped, empty lines
    skipped.  Duplicates are kept."""
    with open(path, "rb") as f:
        data = f.read()
    out = []
    for line in data.split(b"\n"):
        if line.endswith(b"\r"):
            line = line[:-1]
        if line:
            out.append(line)
    return out


def text(password):
    """A candidate's bytes as the str the CLI reports: UTF-8, undecodable bytes as surrogate escapes."""
    return _bytes(password).decode("utf-8", "surrogateescape")


__all__ = ["parse_hybrid", "space", "candidate", "index_of", "read_wordlist", "text"]
