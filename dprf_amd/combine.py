"""Combinator mode: every word of a left wordlist followed by every word of a right one ("summer" + "2024"), the model
of dprf_search_combine (include/dprf.h "combinator mode") in pure Python -- no device, no library.

With N1 left and N2 right words, candidate i of the keyspace N1 * N2 is left word i // N2 followed by right word
i % N2: the left word is the slowest digit, as the word is in hybrid and rule mode.  Words are bytes as the wordlist
holds them (for Office UTF-8; the library converts a table once).  A rule on either side (hashcat's -j / -k) is applied
once per word while the tables are built (:func:`apply_side_rule`), so the device sees plain tables.  Where a format
cuts its candidates behind more than 64 bytes, two long words cannot share a list slot: :func:`fit` picks the pair of
length limits that keeps the most pairs.
"""
from . import rules as rulemod

SLOT = 64


def _bytes(word):
    return word.encode("utf-8", "surrogateescape") if isinstance(word, str) else bytes(word)


def space(nleft, nright):
    """The keyspace: left words times right words, as an exact int."""
    return int(nleft) * int(nright)


def candidate(left, right, index):
    """Candidate `index` as bytes: left word index // N2 followed by right word index % N2."""
    if not 0 <= index < len(left) * len(right):
        raise IndexError("index %d outside the combinator keyspace" % index)
    l, r = divmod(index, len(right))
    return _bytes(left[l]) + _bytes(right[r])


def index_of(left, right, password):
    """The lowest keyspace index that spells `password` (bytes or str); ValueError when none does."""
    pw = _bytes(password)
    first = {}
    for r, w in enumerate(right):
        first.setdefault(_bytes(w), r)
    for l, w in enumerate(left):
        w = _bytes(w)
        if pw.startswith(w) and pw[len(w):] in first:
            return l * len(right) + first[pw[len(w):]]
    raise ValueError("no left and right word spell %r" % (password,))


def apply_side_rule(rule, words, office=False):
    """One rule (a parsed rule of dprf_amd.rules, or its text; None: no rule) applied to every word of one side, once,
    as rules.apply applies it -> (words, dropped).  The words come back as a table takes them: bytes, for Office UTF-8
    again.  A word the rule does not take (no units, more than the rule limit of 64 bytes / 32 UTF-16 units, for Office
    invalid UTF-8) and an Office result that is no text any more (a rule may split a surrogate pair) are dropped and
    counted; the order of the others stays."""
    words = [_bytes(w) for w in words]
    if rule is None:
        return words, 0
    if isinstance(rule, (str, bytes)):
        rule = rulemod.parse_rule(rule)
    out, dropped = [], 0
    for w in words:
        try:
            got = rulemod.apply(rule, w, office)
            if office:
                got = got.decode("utf-16-le").encode("utf-8")
        except rulemod.RuleError:                            # the rule itself is at fault (Office: a unit over 0x7F)
            raise
        except (ValueError, UnicodeError):
            dropped += 1
            continue
        out.append(got)
    return out, dropped


def fit(left_lengths, right_lengths, limit=SLOT):
    """The length limits (a, b), a + b <= limit and both at least 1, that keep the most pairs when the left words
    longer than a and the right words longer than b are dropped: |left <= a| * |right <= b| over the two sequences of
    (converted) word lengths.  Among equal counts the smallest a wins.  With limit = 64 these are the 63 splits
    (1, 63) .. (63, 1)."""
    if limit < 2:
        raise ValueError("a limit of %d leaves no room for two words" % limit)
    lh, rh = [0] * (limit + 1), [0] * (limit + 1)
    for hist, lengths in ((lh, left_lengths), (rh, right_lengths)):
        for n in lengths:
            if 0 <= n <= limit:
                hist[n] += 1
    for hist in (lh, rh):                                     # cumulative: words of at most k bytes
        for k in range(1, limit + 1):
            hist[k] += hist[k - 1]
    best, kept = (1, limit - 1), -1
    for a in range(1, limit):
        n = lh[a] * rh[limit - a]
        if n > kept:
            best, kept = (a, limit - a), n
    return best


__all__ = ["SLOT", "space", "candidate", "index_of", "apply_side_rule", "fit"]
