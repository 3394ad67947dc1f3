"""init_hybrid_brute_force's rounds over an oracle-backed stand-in for the context (no device): the counterpart of
tests/test_mask_parse.py::test_mask_mode_rounds_checkpoint_and_lowest_index.  The stand-in spells a window with its own
speller (word i // M, the mask's characters by itertools.product) and verifies it on the oracle; it records every call,
so the tests pin the calls the driver makes, their order, the printed lines and their order, and the checkpoint."""
import itertools
import json

import pytest

import test_mask_windows as mw
from dprf_amd import brute_force as bf

R5 = tuple(sorted(mw.R5.items()))
LONG = b"k" * 70                                          # over a 64-byte slot: a bare ?w verifies it in list mode


class _OracleHybridCtx:
    """Stand-in for _lib.Context: what init_hybrid_brute_force uses of it, verified by the oracle."""
    kernel = "pdf_r5"

    def __init__(self, oracle, stream, log, fail_at=None):
        self.c = oracle.Ctx(stream)
        self.log = log
        self.fail_at = fail_at
        self.table = None

    def words_status(self, words):
        self.log.append(("words_status", len(words)))
        return [-2 if (not w or b"\0" in w) else 0 for w in words]

    def list_status(self, blob, offsets):
        self.log.append(("list_status", bytes(blob), list(offsets)))
        return [0] * (len(offsets) - 1)

    def set_words(self, words):
        self.log.append(("set_words", list(words)))
        self.table = list(words)

    def verify_list(self, passwords, stop_on_first=False, cap=1 << 16):
        self.log.append(("verify_list", list(passwords)))
        h = [i for i, p in enumerate(passwords) if self.c.verify(p.encode() if isinstance(p, str) else p)]
        return h[:cap], len(h), {"candidates": len(passwords), "wall_ms": 1.0}

    def search_hybrid(self, positions, word_at, start, count, stop_on_first=False, cap=1 << 16):
        if self.fail_at is not None and start >= self.fail_at:
            raise KeyboardInterrupt
        self.log.append(("search_hybrid", start, count))
        assert self.table, "search_hybrid before set_words"
        tails = ["".join(t) for t in itertools.product(*positions)]
        spelled = [t[:word_at].encode() + w + t[word_at:].encode() for w in self.table for t in tails]
        window = spelled[start:start + count]
        assert len(window) == count, "window outside the keyspace"
        h = [start + k for k, v in enumerate(self.c.verify_list(window)) if v]
        return h[:cap], len(h), {"candidates": count, "wall_ms": 1.0}

    def close(self):
        self.log.append(("close",))


TAGS = ("Dropped", "Checkpoint", "Running time", "Speed", "Queue size", "Tried", "Correct")


def _tags(out):
    """The printed lines as their leading words, in order; a line none of TAGS begins fails the test."""
    tags = []
    for line in out.splitlines():
        tag = [t for t in TAGS if line.startswith(t)]
        assert tag, "unexpected line %r" % line
        tags.append(tag[0])
    return tags


ROUND = ["Running time", "Speed", "Queue size"]
WORDS = [b"ant", b"", b"bee", b"cat", b"x" * 64, b"dog", b"eel"]      # word 2 is empty, word 5 too long beside ?d
KEPT = [b"ant", b"bee", b"cat", b"dog", b"eel"]
DROPPED = ["Dropped 1 words no candidate can contain (empty, a NUL byte, or for Office invalid UTF-8), the first is "
           "word 2", "Dropped 1 words too long for a 64-byte candidate with this mask"]


def test_hybrid_mode_rounds_checkpoint_and_lowest_index(oracle, tmp_path, monkeypatch, capsys):
    stream = mw._stream_of("pdf", R5, "cat7")
    fields = mw._fields(stream)
    assert oracle.Ctx(stream).verify(b"cat7") and not oracle.Ctx(stream).verify(b"_dummy")
    monkeypatch.setattr(bf, "FIRST_ROUND", 10)
    monkeypatch.setattr(bf, "ROUND_SECONDS", 0.0)
    cp = str(tmp_path / "cursor.json")
    want = bf.hybrid.index_of(KEPT, ["0123456789"], 0, "cat7")
    assert want == 27
    # 1. interrupted at a round boundary
    log1 = []
    monkeypatch.setattr(bf, "_context", lambda inp, dev: _OracleHybridCtx(oracle, stream, log1, fail_at=20))
    capsys.readouterr()
    with pytest.raises(KeyboardInterrupt):
        bf.init_hybrid_brute_force(fields, WORDS, "?w?d", checkpoint=cp)
    assert log1 == [("words_status", 7), ("verify_list", ["_dummy"]), ("set_words", KEPT), ("search_hybrid", 0, 10),
                    ("search_hybrid", 10, 10), ("close",)]
    out = capsys.readouterr().out
    assert out.splitlines()[:2] == DROPPED and _tags(out) == ["Dropped"] * 2 + ROUND * 2
    assert [ln for ln in out.splitlines() if ln.startswith("Queue")] == ["Queue size: 40", "Queue size: 30"]
    saved = json.load(open(cp))
    assert saved["next_index"] == 20 and saved["found"] is None and saved["hybrid_mask"] == "?w?d"
    assert saved["words"] == 7 and saved["wordlist_sha256"] == bf.wordlist_key(WORDS)[0] and "mask" not in saved
    # 2. resumed from the checkpoint, 3. the lowest index wins
    log2 = []
    monkeypatch.setattr(bf, "_context", lambda inp, dev: _OracleHybridCtx(oracle, stream, log2))
    assert bf.init_hybrid_brute_force(fields, WORDS, "?w?d", checkpoint=cp) == (1, "cat7")
    assert log2 == [("words_status", 7), ("set_words", KEPT), ("search_hybrid", 20, 10), ("close",)]
    out = capsys.readouterr().out
    lines = out.splitlines()
    assert _tags(out) == ["Dropped"] * 2 + ["Checkpoint"] + ROUND + ["Tried", "Correct"]
    assert lines[:3] == DROPPED + ["Checkpoint: resuming at index 20"]
    assert lines[5] == "Queue size: 0" and lines[6].startswith("Tried 10 candidates in ")
    assert lines[7] == "Correct password is 'cat7'"
    saved = json.load(open(cp))
    assert saved["next_index"] == 30 and saved["found"] == "cat7"
    # 4. a finished checkpoint answers without a context
    monkeypatch.setattr(bf, "_context", lambda inp, dev: pytest.fail("a context was created"))
    assert bf.init_hybrid_brute_force(fields, WORDS, "?w?d", checkpoint=cp) == (1, "cat7")
    assert capsys.readouterr().out == "Checkpoint: search already finished, password 'cat7'\n"
    # another wordlist or another mask is another search
    for words, mask in ((KEPT, "?w?d"), (WORDS, "?d?w")):
        with pytest.raises(ValueError):
            bf.init_hybrid_brute_force(fields, words, mask, checkpoint=cp)
    # an unsuccessful search from index 0 verifies "_dummy" first, exhausts the keyspace and closes the context
    log3 = []
    monkeypatch.setattr(bf, "_context", lambda inp, dev: _OracleHybridCtx(oracle, stream, log3))
    assert bf.init_hybrid_brute_force(fields, [b"cat", b"ca"], "?l?w") == (0, bf.DEFAULT_PASSWORD)
    assert log3 == [("words_status", 2), ("verify_list", ["_dummy"]), ("set_words", [b"cat", b"ca"]),
                    ("search_hybrid", 0, 10), ("search_hybrid", 10, 10), ("search_hybrid", 20, 10),
                    ("search_hybrid", 30, 10), ("search_hybrid", 40, 10), ("search_hybrid", 50, 2), ("close",)]
    out = capsys.readouterr().out
    assert _tags(out) == ROUND * 6 + ["Tried"] and out.splitlines()[-1].startswith("Tried 53 candidates in ")


def test_bare_word_mask_verifies_the_long_words_as_a_list_at_the_end(oracle, tmp_path, monkeypatch, capsys):
    stream = mw._stream_of("pdf", R5, LONG.decode())
    fields = mw._fields(stream)
    assert oracle.Ctx(stream).verify(LONG) and not oracle.Ctx(stream).verify(LONG[:64])
    monkeypatch.setattr(bf, "FIRST_ROUND", 10)
    monkeypatch.setattr(bf, "ROUND_SECONDS", 0.0)
    cp = str(tmp_path / "cursor.json")
    log = []
    monkeypatch.setattr(bf, "_context", lambda inp, dev: _OracleHybridCtx(oracle, stream, log))
    capsys.readouterr()
    assert bf.init_hybrid_brute_force(fields, [b"ant", LONG, b"bee"], checkpoint=cp) == (1, LONG.decode())
    assert log == [("words_status", 3), ("verify_list", ["_dummy"]), ("set_words", [b"ant", b"bee"]),
                   ("search_hybrid", 0, 2), ("list_status", LONG, [0, 70]), ("verify_list", [LONG]), ("close",)]
    out = capsys.readouterr().out
    lines = out.splitlines()
    assert _tags(out) == ["Dropped"] + ROUND + ["Tried", "Tried", "Correct"]
    assert lines[0] == ("Dropped 1 words too long for a 64-byte candidate with this mask; they are verified as a list "
                        "at the end")
    assert lines[3] == "Queue size: 0" and lines[4].startswith("Tried 3 candidates in ")
    assert lines[5].startswith("Tried 1 candidates in ") and lines[6] == "Correct password is '%s'" % LONG.decode()
    saved = json.load(open(cp))
    assert saved["next_index"] == 3 and saved["found"] == LONG.decode() and saved["hybrid_mask"] == "?w"
    # resumed behind the table (index 2 = the table's end): no rounds, the list pass alone
    json.dump(dict(saved, next_index=2, found=None), open(cp, "w"))
    del log[:]
    assert bf.init_hybrid_brute_force(fields, [b"ant", LONG, b"bee"], checkpoint=cp) == (1, LONG.decode())
    assert log == [("words_status", 3), ("set_words", [b"ant", b"bee"]), ("list_status", LONG, [0, 70]),
                   ("verify_list", [LONG]), ("close",)]
    assert _tags(capsys.readouterr().out) == ["Dropped", "Checkpoint", "Tried", "Tried", "Correct"]
