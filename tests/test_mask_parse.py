"""The mask language (dprf_amd/mask.py) and the host logic of mask mode that needs no device: tokens and refusals,
space / word / index_of, the checkpoint key, the CLI's argument conflicts, the 64-bit window guard of
Context.search_mask, and init_mask_brute_force's rounds over an oracle-backed stand-in for the context."""
import itertools
import json

import pytest

from dprf_amd import _lib, brute_force as bf
from dprf_amd import mask as M

LOWER = "abcdefghijklmnopqrstuvwxyz"
SPECIAL = " !\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"


def refused(mask, custom=(), naming=None):
    with pytest.raises(_lib.DprfError) as ei:
        M.parse_mask(mask, custom)
    assert ei.value.code == _lib.E_CHARSET, (mask, custom)
    if naming is not None:
        assert naming in str(ei.value), (naming, str(ei.value))


# ------------------------------------------------------------------ tokens
def test_builtin_tokens():
    assert M.parse_mask("?l") == [LOWER] and M.parse_mask("?u") == [LOWER.upper()]
    assert M.parse_mask("?d") == ["0123456789"]
    assert M.parse_mask("?h") == ["0123456789abcdef"] and M.parse_mask("?H") == ["0123456789ABCDEF"]
    assert M.parse_mask("?s") == [SPECIAL]
    # ?s: every printable ASCII character that is neither a letter nor a digit, the space too, in ASCII order
    assert len(SPECIAL) == 33 and list(SPECIAL) == sorted(SPECIAL)
    assert set(SPECIAL) == {chr(c) for c in range(0x20, 0x7f) if not chr(c).isalnum()}
    assert M.parse_mask("?a") == [LOWER + LOWER.upper() + "0123456789" + SPECIAL]
    assert len(M.parse_mask("?a")[0]) == 95


def test_literals_and_the_question_mark():
    assert M.parse_mask("Inv-?d?d€") == ["I", "n", "v", "-", "0123456789", "0123456789", "€"]
    assert M.parse_mask("??") == ["?"] and M.parse_mask("a???d") == ["a", "?", "0123456789"]
    assert M.parse_mask("\U0001D11E") == ["\U0001D11E"]
    assert M.parse_mask("?u?l?l?l?l?l?d?d") == [LOWER.upper()] + [LOWER] * 5 + ["0123456789"] * 2


def test_custom_sets():
    assert M.parse_mask("?1?2", ["€é", "xyz"]) == ["€é", "xyz"]
    assert M.parse_mask("a?4", [None, None, None, "?d_"]) == ["a", "0123456789_"]
    assert M.parse_mask("?1", ["?l?d-"]) == [LOWER + "0123456789-"]       # built-in tokens inside a custom set
    assert M.parse_mask("?1", ["x??"]) == ["x?"]                           # ... and a literal '?'
    assert M.parse_mask("?1?1", ["ba"]) == ["ba", "ba"]                    # enumeration order is the set's own order
    assert M.parse_mask("?l", ["xyz"]) == [LOWER]


@pytest.mark.parametrize("mask,custom,naming", [
    ("?b", (), "position 0"),                       # all bytes: holds NUL
    ("ab?b", (), "position 2"),
    ("?x", (), "position 0"),                       # unknown token
    ("?l?L", (), "position 1"),
    ("abc?", (), "position 3"),                     # trailing '?'
    ("?", (), "position 0"),
    ("?l?2", ("abc",), "position 1"),               # undefined custom set
    ("?1", (), "position 0"),
    ("?3", ("a", "b", None), "position 0"),
    ("?5", ("a", "b", "c", "d"), "position 0"),     # no fifth set: an unknown token
    ("?1", ("abca",), "custom set 1"),              # a repeated character inside a set
    ("?1", ("?la",), "custom set 1"),
    ("?1", ("?d?h",), "custom set 1"),
    ("?1", ("????",), "custom set 1"),
    ("?1?2", ("ab", "?1c"), "custom set 2"),        # a custom token inside a custom set
    ("a\0b", (), "position 1"),                     # NUL
    ("?1", ("a\0",), "custom set 1"),
    ("", (), None),                                 # no position at all
])
def test_refusals_name_the_position(mask, custom, naming):
    refused(mask, custom, naming)


def test_refusals_of_other_kinds():
    refused("?1", ("a", "b", "c", "d", "e"))        # five custom sets
    refused(b"?l")                                  # not a str
    refused("\ud800")                               # a lone surrogate cannot be spelled as UTF-8


# ------------------------------------------------------------------ space / word / index_of
def test_space_word_index_of_round_trip():
    pos = M.parse_mask("?1x?d?2", ["αβγ", "€é"])
    assert [len(p) for p in pos] == [3, 1, 10, 2] and M.space(pos) == 60
    ref = ["".join(t) for t in itertools.product(*pos)]
    assert [M.word(pos, i) for i in range(60)] == ref
    assert [M.index_of(pos, w) for w in ref] == list(range(60))
    for bad in (-1, 60):
        with pytest.raises(IndexError):
            M.word(pos, bad)
    for bad in ("αx0", "αy0€", "αx0a"):
        with pytest.raises(ValueError):
            M.index_of(pos, bad)


def test_space_is_an_exact_int_past_64_bits():
    pos = M.parse_mask("?a" * 32)
    assert M.space(pos) == 95 ** 32 and M.space(pos) > 1 << 200
    assert M.index_of(pos, M.word(pos, 95 ** 32 - 12345)) == 95 ** 32 - 12345


def test_uniform_mask_enumerates_as_range_mode():
    charset, n = "abc€é", 4
    pos = M.parse_mask("?1" * n, [charset])
    assert M.space(pos) == len(charset) ** n
    for i in list(range(0, 40)) + [len(charset) ** n - 1, 311]:
        assert M.word(pos, i) == bf._index_to_password(i, charset, n)
    big = M.parse_mask("?l" * 14)
    for i in (0, 26 ** 14 - 1, 1 << 40, (1 << 64) + 3):
        assert M.word(big, i) == bf._index_to_password(i, LOWER, 14)


# ------------------------------------------------------------------ checkpoint key
FIELDS = ["pdf", "1", "2", "3"]


def test_checkpoint_key_separates_masks_and_range_searches(tmp_path):
    path = str(tmp_path / "cursor.json")
    a = bf.Checkpoint(path, FIELDS, mask="?l?d?1", custom=("xy",))
    a.save(1234)
    assert bf.Checkpoint(path, FIELDS, mask="?l?d?1", custom=("xy",)).load() == (1234, None)
    for other in (bf.Checkpoint(path, FIELDS, mask="?l?d?2", custom=("xy",)),          # another mask
                  bf.Checkpoint(path, FIELDS, mask="?l?d?1", custom=("xz",)),          # another custom set
                  bf.Checkpoint(path, FIELDS, mask="?l?d?1", custom=()),
                  bf.Checkpoint(path, FIELDS + ["4"], mask="?l?d?1", custom=("xy",)),  # another document
                  bf.Checkpoint(path, FIELDS, LOWER, 3)):                              # a -pr search
        with pytest.raises(ValueError):
            other.load()
    # and a -pr checkpoint is refused by a mask search
    bf.Checkpoint(path, FIELDS, LOWER, 3).save(99)
    with pytest.raises(ValueError):
        bf.Checkpoint(path, FIELDS, mask="?l?l?l").load()


def test_range_checkpoints_written_before_mask_mode_keep_loading(tmp_path):
    """The -pr key is unchanged: exactly the three entries earlier versions wrote."""
    import hashlib
    path = str(tmp_path / "cursor.json")
    sha = hashlib.sha256("*".join(FIELDS).encode()).hexdigest()
    json.dump({"stream_sha256": sha, "charset": LOWER, "pwlen": 3, "next_index": 4056, "found": None}, open(path, "w"))
    cp = bf.Checkpoint(path, FIELDS, LOWER, 3)
    assert cp.key == {"stream_sha256": sha, "charset": LOWER, "pwlen": 3}
    assert cp.load() == (4056, None)


# ------------------------------------------------------------------ CLI argument conflicts
@pytest.mark.parametrize("argv", [
    ["3", "nosuch.pdf", "--mask", "?l?l", "-pr", "2"],
    ["3", "nosuch.pdf", "--mask", "?l?l", "--passwordrange", "2"],
    ["3", "nosuch.pdf", "--mask", "?l?l", "--charset", "abc"],
    ["3", "nosuch.pdf", "-1", "abc"],                                  # a custom set without a mask
    ["3", "nosuch.pdf", "-pr", "2", "--custom-charset2", "abc"],
])
def test_cli_argument_conflicts_are_argparse_errors(argv, capsys):
    with pytest.raises(SystemExit) as ei:
        bf.main(argv)
    assert ei.value.code == 2                                           # argparse's usage error, before any parsing
    assert "usage:" in capsys.readouterr().err


def test_cli_passes_mask_and_custom_sets_on(monkeypatch):
    seen = {}
    monkeypatch.setattr(bf, "get_verification_data", lambda t, f: "stream")
    monkeypatch.setattr(bf, "init", lambda *a, **k: seen.update(a=a, k=k) or (1, "pw"))
    assert bf.main(["3", "x.pdf", "--mask", "Inv-?d?d?1", "-1", "€é", "--custom-charset3", "?l"]) == (1, "pw")
    assert seen["a"] == ("stream", None, None)
    assert seen["k"]["mask"] == "Inv-?d?d?1" and list(seen["k"]["custom_charsets"]) == ["€é", None, "?l"]
    # without --mask the call is the one the CLI always made
    bf.main(["3", "x.pdf", "-pr", "2"])
    assert seen["a"] == ("stream", 2, None) and seen["k"]["charset"] == LOWER and "mask" not in seen["k"]
    bf.main(["3", "x.pdf", "--charset", "ab"])
    assert seen["a"] == ("stream", 8, None) and seen["k"]["charset"] == "ab"


def test_init_refuses_a_mask_beside_a_range_or_a_list():
    for pr, pws in ((3, None), (None, ["a"])):
        with pytest.raises(ValueError):
            bf.init("x", pr, pws, mask="?l")


# ------------------------------------------------------------------ the 64-bit window guard
def test_binding_refuses_mask_windows_over_64_bits_before_the_library():
    """As tests/test_symbol_windows.py: ctypes would wrap them; no handle, so the library must not be reached."""
    ctx = _lib.Context.__new__(_lib.Context)
    pos = M.parse_mask("?1" * 14, ["αβγδεζηθικλμνξοπρστυφχψω"])
    assert M.space(pos) == 24 ** 14 > 1 << 64
    for start, count in ((0, 24 ** 14), (0, 1 << 64), (1 << 63, 1 << 63), ((1 << 64) - 1, 1), (-1, 4), (0, -1)):
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_mask(pos, start, count)
        assert ei.value.code == _lib.E_INVALID, (start, count)


# ------------------------------------------------------------------ mask mode's rounds, on the oracle
class _OracleMaskCtx:
    """Stand-in for _lib.Context: search_mask by the oracle over the window spelled with itertools-order divmod."""

    def __init__(self, oracle, stream, log, fail_at=None):
        self.c = oracle.Ctx(stream)
        self.log = log
        self.fail_at = fail_at

    def verify_list(self, passwords, stop_on_first=False, cap=1 << 16):
        h = [i for i, p in enumerate(passwords) if self.c.verify(p.encode())]
        return h[:cap], len(h), {"candidates": len(passwords), "wall_ms": 1.0}

    def search_mask(self, positions, start, count, stop_on_first=False, cap=1 << 16):
        if self.fail_at is not None and start >= self.fail_at:
            raise KeyboardInterrupt
        self.log.append((start, count))
        words = ["".join(t) for t in itertools.islice(itertools.product(*positions), start, start + count)]
        h = [start + k for k, v in enumerate(self.c.verify_list([w.encode() for w in words])) if v]
        return h[:cap], len(h), {"candidates": count, "wall_ms": 1.0}

    def close(self):
        pass


def test_mask_mode_rounds_checkpoint_and_lowest_index(streams, oracle, tmp_path, monkeypatch, capsys):
    d = streams["pdf_synth_r5_cat"]
    fields = bf.parse_verification_data(d["stream"])
    monkeypatch.setattr(bf, "FIRST_ROUND", 500)
    monkeypatch.setattr(bf, "ROUND_SECONDS", 0.0)
    cp = str(tmp_path / "cursor.json")
    mask, custom = "?1?l?1", ["?lXY"]
    pos = M.parse_mask(mask, custom)
    want = M.index_of(pos, "cat")
    assert want > 1000
    log1 = []
    monkeypatch.setattr(bf, "_context", lambda inp, dev: _OracleMaskCtx(oracle, d["stream"], log1, fail_at=1000))
    with pytest.raises(KeyboardInterrupt):
        bf.init_mask_brute_force(fields, mask, custom, checkpoint=cp)
    assert log1 == [(0, 500), (500, 500)]
    saved = json.load(open(cp))
    assert saved["next_index"] == 1000 and saved["mask"] == mask and saved["custom"] == custom
    log2 = []
    monkeypatch.setattr(bf, "_context", lambda inp, dev: _OracleMaskCtx(oracle, d["stream"], log2))
    capsys.readouterr()
    assert bf.init_mask_brute_force(fields, mask, custom, checkpoint=cp) == (1, "cat")
    out = capsys.readouterr().out
    assert "Checkpoint: resuming at index 1000" in out and "Queue size: " in out
    assert log2[0] == (1000, 500) and log2[-1][0] <= want < log2[-1][0] + log2[-1][1]
    assert bf.init_mask_brute_force(fields, mask, custom, checkpoint=cp) == (1, "cat")      # answered from the file
    with pytest.raises(ValueError):
        bf.init_mask_brute_force(fields, "?l?l?l", checkpoint=cp)
    with pytest.raises(ValueError):
        bf.init_rangebased_brute_force(fields, 3, checkpoint=cp)
    # a mask that does not spell the password exhausts its keyspace
    assert bf.init_mask_brute_force(fields, "ca?d") == (0, bf.DEFAULT_PASSWORD)
    # a bad mask is refused before any device work
    monkeypatch.setattr(bf, "_context", lambda inp, dev: pytest.fail("a context was created"))
    with pytest.raises(_lib.DprfError) as ei:
        bf.init_mask_brute_force(fields, "?l?b")
    assert ei.value.code == _lib.E_CHARSET
