"""dprf_amd.combine, the pure-Python model of combinator mode, and the CLI's argument refusals -- no device.

  candidate / index_of / space against itertools.product
  apply_side_rule against rules.apply, word by word
  fit against brute force over all 63 splits of seeded length histograms
  brute_force.main: what --wordlist2, --rule-left and --rule-right refuse before a document is read"""
import itertools
import random

import pytest

from dprf_amd import brute_force, combine, rules
from test_hybrid_windows import table

LEFT = table(23, 0xC0B1, 1, 9) + [b"sun", b"sun", b"su"]
RIGHT = table(11, 0xC0B2, 1, 6) + [b"n7", b"7", b"7"]


def test_candidate_space_and_index_of_follow_itertools_product():
    want = [l + r for l, r in itertools.product(LEFT, RIGHT)]
    assert combine.space(len(LEFT), len(RIGHT)) == len(want) == 26 * 14
    assert [combine.candidate(LEFT, RIGHT, i) for i in range(len(want))] == want
    for i in (-1, len(want)):
        with pytest.raises(IndexError):
            combine.candidate(LEFT, RIGHT, i)
    # the lowest index: "sun" + "7" is spelled by (sun, 7) twice over and by (su, n7)
    assert want.count(b"sun7") == 5
    assert combine.index_of(LEFT, RIGHT, "sun7") == combine.index_of(LEFT, RIGHT, b"sun7") == want.index(b"sun7")
    for pw in set(want):
        assert combine.index_of(LEFT, RIGHT, pw) == want.index(pw)
    with pytest.raises(ValueError):
        combine.index_of(LEFT, RIGHT, b"\x01nowhere")
    assert combine.candidate(["é"], ["€"], 0) == "é€".encode()            # str words are their UTF-8
    assert combine.space(1 << 31, 1 << 40) == 1 << 71                      # an exact int


@pytest.mark.parametrize("office", [False, True])
@pytest.mark.parametrize("text", ["$-", "c", "u $1", "r", "] ]", "^x d", "sa@", "T0"])
def test_apply_side_rule_is_rules_apply_word_by_word(text, office):
    words = table(40, 0xC0B3, 1, 12)
    rule = rules.parse_rule(text)
    got, dropped = combine.apply_side_rule(text, words, office)
    want = [rules.apply(rule, w, office) for w in words]
    if office:
        want = [w.decode("utf-16-le").encode("utf-8") for w in want]
    assert dropped == 0 and got == want
    assert combine.apply_side_rule(rule, words, office) == (want, 0)       # text or parsed, the same
    assert combine.apply_side_rule(None, words, office) == (words, 0)      # no rule: the words as they are


def test_apply_side_rule_drops_what_the_rule_cannot_take():
    words = [b"ok", b"", b"x" * 64, b"y" * 65, "é".encode() * 33, b"\xff", b"end"]
    # bytes: the empty word and the two over 64 bytes go; 64 bytes stay as they are ($! would pass the limit)
    assert combine.apply_side_rule("$!", words, office=False) == ([b"ok!", b"x" * 64, b"\xff!", b"end!"], 3)
    # Office: 32 units at the most, and valid UTF-8
    assert combine.apply_side_rule("$!", words, office=True) == ([b"ok!", b"end!"], 5)
    assert combine.apply_side_rule("$!", ["é" * 32, "é" * 31], office=True) == (["é".encode() * 32, ("é" * 31 + "!").encode()], 0)
    # Office: a rule that splits a surrogate pair leaves no text; such a word is dropped
    pair = "a\U0001D11E".encode()
    assert combine.apply_side_rule("]", [pair, b"ab"], office=True) == ([b"a"], 1)
    assert combine.apply_side_rule("]", [pair, b"ab"], office=False) == ([pair[:-1], b"a"], 0)
    with pytest.raises(rules.RuleError):                                   # the rule's own fault is not a dropped word
        combine.apply_side_rule(b"$\xe9", [b"ab"], office=True)


def _brute_fit(ll, rl, limit=64):
    return max(sum(1 for n in ll if n <= a) * sum(1 for n in rl if n <= limit - a) for a in range(1, limit))


def _kept(ll, rl, ab):
    return sum(1 for n in ll if n <= ab[0]) * sum(1 for n in rl if n <= ab[1])


@pytest.mark.parametrize("seed", range(12))
def test_fit_keeps_as_many_pairs_as_any_of_the_63_splits(seed):
    rng = random.Random(0xF17 + seed)
    shapes = [(1, 20), (1, 64), (10, 90), (30, 64), (1, 5), (50, 64)]
    lo1, hi1 = shapes[seed % 6]
    lo2, hi2 = shapes[(seed // 2 + 3) % 6]
    ll = [rng.randint(lo1, hi1) for _ in range(rng.randint(1, 400))]
    rl = [rng.randint(lo2, hi2) for _ in range(rng.randint(1, 400))]
    a, b = combine.fit(ll, rl)
    assert 1 <= a and 1 <= b and a + b <= 64
    assert _kept(ll, rl, (a, b)) == _brute_fit(ll, rl)
    assert combine.fit(ll, rl) == combine.fit(list(reversed(ll)), sorted(rl))   # a function of the histograms


def test_fit_edge_cases():
    ll, rl = [3, 8, 12, 1], [4, 4, 9]
    a, b = combine.fit(ll, rl)                                             # nothing dropped
    assert a >= 12 and b >= 9 and _kept(ll, rl, (a, b)) == 12
    assert (a, b) == (12, 52)                                              # among equal counts the smallest a
    assert combine.fit([64, 70, 100], [1, 2, 3]) == (1, 63)                # one side all long: no pair can be kept
    assert _brute_fit([64, 70, 100], [1, 2, 3]) == 0
    assert combine.fit([63], [1]) == (63, 1) and combine.fit([1], [63]) == (1, 63) and combine.fit([32], [32]) == (32, 32)
    # many short and a few long words on both sides: the long ones go
    assert combine.fit([8] * 100 + [60] * 2, [4] * 100 + [40] * 3) == (8, 56)
    assert combine.fit([5, 6], [5, 6], limit=10) == (5, 5)
    with pytest.raises(ValueError):
        combine.fit([1], [1], limit=1)


REFUSED = [
    ["--wordlist2", "r.txt"],                                              # no left side
    ["--wordlist", "l.txt", "--wordlist2", "r.txt", "--mask", "?w?d"],
    ["--wordlist", "l.txt", "--wordlist2", "r.txt", "--rules", "x.rule"],
    ["--wordlist", "l.txt", "--wordlist2", "r.txt", "-pr", "3"],
    ["--wordlist", "l.txt", "--wordlist2", "r.txt", "--key40"],
    ["--wordlist", "l.txt", "--rule-left", "$-"],                          # side rules without a right side
    ["--wordlist", "l.txt", "--rule-right", "c"],
    ["--rule-left", "$-", "-pr", "3"],
    ["--wordlist", "l.txt", "--wordlist2", "r.txt", "--rule-left", "$"],    # a rule the language does not hold
    ["--wordlist", "l.txt", "--wordlist2", "r.txt", "--rule-right", "~"],
]


@pytest.mark.parametrize("extra", REFUSED, ids=[" ".join(e) for e in REFUSED])
def test_cli_refuses_before_the_document_is_read(extra, capsys):
    """The document does not exist: a refusal that came after reading it would be another error."""
    with pytest.raises(SystemExit) as ei:
        brute_force.main(["3", "/nonexistent/none.pdf"] + extra)
    assert ei.value.code == 2
    err = capsys.readouterr().err
    assert "wordlist2" in err or "--rule-" in err, err


def test_init_refuses_the_same_combinations():
    for kw in (dict(wordlist2=[b"a"]), dict(wordlist=[b"a"], wordlist2=[b"b"], mask="?w?d"),
               dict(wordlist=[b"a"], wordlist2=[b"b"], rules=[()]), dict(wordlist=[b"a"], rule_left="c"),
               dict(wordlist=[b"a"], wordlist2=[b"b"], passwords=["x"])):
        kw = dict(kw)
        passwords = kw.pop("passwords", None)
        with pytest.raises(ValueError):
            brute_force.init("$pdf$none", None, passwords, **kw)


def test_checkpoint_key_covers_both_wordlists_and_both_rules(tmp_path):
    data = ["pdf", "x"]
    path = str(tmp_path / "cp.json")
    key = lambda l, r, rules_=("", ""): brute_force.Checkpoint(
        path, data, wordlist=brute_force.wordlist_key(l), wordlist2=brute_force.wordlist_key(r), side_rules=rules_)
    key([b"a", b"b"], [b"c"]).save(7)
    assert key([b"a", b"b"], [b"c"]).load() == (7, None)
    for other in (key([b"a", b"b"], [b"c", b"d"]), key([b"a"], [b"c"]), key([b"a", b"b"], [b"c"], ("$-", "")),
                  key([b"a", b"b"], [b"c"], ("", "c")),
                  brute_force.Checkpoint(path, data, mask="?w", wordlist=brute_force.wordlist_key([b"a", b"b"]))):
        with pytest.raises(ValueError):
            other.load()
    # ... and a hybrid search's file is not a combinator search's
    brute_force.Checkpoint(path, data, mask="?w", wordlist=brute_force.wordlist_key([b"a", b"b"])).save(3)
    with pytest.raises(ValueError):
        key([b"a", b"b"], [b"c"]).load()
