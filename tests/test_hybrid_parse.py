"""Hybrid search without a device: the ?w mask language and the keyspace arithmetic of dprf_amd.hybrid, the four new
symbols of the C ABI (header, library, binding), the command line's refusals, and the checkpoint key."""
import ctypes
import itertools
import json
import os
import re

import pytest

from dprf_amd import _lib, brute_force, hybrid, mask

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOWER, DIGITS = mask.LOWER, mask.DIGITS
NEW = ["dprf_ctx_set_words", "dprf_ctx_words", "dprf_words_status", "dprf_search_hybrid"]


def _refused(text, custom=()):
    with pytest.raises(_lib.DprfError) as ei:
        hybrid.parse_hybrid(text, custom)
    assert ei.value.code == _lib.E_CHARSET
    return str(ei.value)


def test_parse_hybrid_places_the_word():
    assert hybrid.parse_hybrid("?w?d?d") == ([DIGITS, DIGITS], 0)
    assert hybrid.parse_hybrid("?d?d-?w") == ([DIGITS, DIGITS, "-"], 3)
    assert hybrid.parse_hybrid("Inv-?w-?1", ["€é"]) == (list("Inv-") + ["-", "€é"], 4)
    assert hybrid.parse_hybrid("?w") == ([], 0)
    assert hybrid.parse_hybrid("???w??w") == (["?", "?", "w"], 1)         # "??" is a literal '?', "?w" the word
    assert hybrid.parse_hybrid("w?w") == (["w"], 1)


def test_parse_hybrid_refusals():
    assert "?w" in _refused("?d?d")                                       # the word is missing
    assert "?w" in _refused("")
    assert "2 times" in _refused("?w-?w")
    assert "custom set 1" in _refused("?w?1", ["ab?w"])
    _refused("?w?b")                                                      # the mask language's own refusals stay
    _refused("?w?2", ["ab"])
    _refused("?w?1", ["aba"])
    with pytest.raises(_lib.DprfError):                                   # the mask parser does not learn ?w
        mask.parse_mask("?w?d")


def test_candidate_and_index_of_round_trip():
    words = [b"sun", "é€".encode(), b"sun", b"x" * 70, b"\xff\xfe"]
    pos = ["ab", "-", DIGITS]
    m = mask.space(pos)
    assert hybrid.space(len(words), pos) == 5 * 20 == len(words) * m and hybrid.space(7, []) == 7
    prod = list(itertools.product(words, itertools.product(*pos)))
    for at in range(4):
        got = [hybrid.candidate(words, pos, at, i) for i in range(len(prod))]
        want = ["".join(t[:at]).encode() + w + "".join(t[at:]).encode() for w, t in prod]
        assert got == want, at
        for i, pw in enumerate(got):
            j = hybrid.index_of(words, pos, at, pw)
            assert j == (i - 2 * m if i // m == 2 else i), (at, i, j)     # the duplicate word: its lowest index
    assert [hybrid.candidate(words, [], 0, i) for i in range(5)] == words
    assert hybrid.index_of(words, [], 0, b"\xff\xfe") == 4
    assert hybrid.text(b"a\xff") == "a\udcff" and hybrid.index_of([b"a\xff"], ["-"], 0, "a\udcff-") == 0
    for bad in (-1, 100):
        with pytest.raises(IndexError):
            hybrid.candidate(words, pos, 0, bad)
    with pytest.raises(ValueError):
        hybrid.index_of(words, pos, 0, b"moon-a-0")


def test_read_wordlist(tmp_path):
    p = tmp_path / "w.txt"
    p.write_bytes(b"sun\r\n\r\nmoon\n\nsun\n\xff\xfe raw\nlast")
    assert hybrid.read_wordlist(str(p)) == [b"sun", b"moon", b"sun", b"\xff\xfe raw", b"last"]


def test_header_library_and_binding_carry_the_new_symbols():
    header = open(os.path.join(REPO, "include", "dprf.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\(dprf_ctx \*ctx|\b%s\(const dprf_ctx \*ctx" % (name, name), header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.dprf_abi_version() == 9 == _lib.ABI_VERSION and "#define DPRF_ABI_VERSION 9" in header
    # null contexts are refused without a device
    assert L.dprf_ctx_set_words(None, None, None, 0) == _lib.E_INVALID
    assert L.dprf_ctx_words(None) == _lib.E_INVALID
    assert L.dprf_words_status(None, None, None, 0, None) == _lib.E_INVALID
    assert L.dprf_search_hybrid(None, None, None, None, 0, 0, 0, 0, 0, None, 0, None, None) == _lib.E_INVALID
    assert b"null context" in L.dprf_last_error()
    assert ctypes.sizeof(_lib.Stats) == 56                                # no struct changed


def test_kernel_is_gated_and_built_into_its_own_object():
    csrc = os.path.join(REPO, "dprf_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    # the four spellers share one source and one object (dprf_kernels_spell.hip); each is an expected kernel of it
    assert "$(OBJDIR)/dprf_kernels_spell.o: EXPECT := k_spell_symbols,k_spell_mask,k_spell_hybrid,k_spell_rules" in mk
    assert re.search(r"KOBJS\s+:=[^#]*dprf_kernels_spell\.o", mk, re.S) and "dprf_kernels_spell.hip $(HDRS)" in mk
    assert re.search(r"BUILD_ID := .*dprf_kernels_spell\.hip", mk)
    assert "dprf_kernels_hybrid" not in mk and "dprf_kernels_rules" not in mk
    gate = {}
    exec(open(os.path.join(csrc, "resource_gate.py")).read().split("def parse")[0], gate)
    assert gate["SCRATCH_LIMIT"]["k_spell_hybrid"] == 0
    params = open(os.path.join(csrc, "dprf_params.h")).read()
    assert "#define DPRF_HYB_RUN 256" in params
    assert "#define DPRF_HYB_RUN_WORDS (DPRF_HYB_RUN * DPRF_SLOT_WORDS + 1)" in params
    assert "k_spell_hybrid(dprf_hybrid_args a" in open(os.path.join(csrc, "dprf_kernels_spell.hip")).read()


STREAM = "x:$pdf$5*5*256*-1028*1*16*" + "0" * 32 + "*127*" + "0" * 254 + "*127*" + "0" * 254 + "*32*" + "0" * 64


def test_cli_refusals_need_no_device(tmp_path, monkeypatch):
    words = tmp_path / "words.txt"
    words.write_bytes(b"sun\nmoon\n")
    doc = str(tmp_path / "missing.pdf")

    def no_parse(*a):
        raise AssertionError("the document was read before the arguments were refused")
    monkeypatch.setattr(brute_force, "get_verification_data", no_parse)
    with pytest.raises(ValueError, match="wordlist"):
        brute_force.main(["3", doc, "--wordlist", str(words), "-pr", "4"])
    with pytest.raises(ValueError, match=r"\?w"):
        brute_force.main(["3", doc, "--wordlist", str(words), "--mask", "?d?d"])
    with pytest.raises(ValueError, match=r"\?w"):
        brute_force.main(["3", doc, "--wordlist", str(words), "--mask", "?w?w"])
    # the module entry: the same refusals before any context is made
    monkeypatch.setattr(brute_force, "_context", no_parse)
    with pytest.raises(ValueError):
        brute_force.init(STREAM, 4, None, wordlist=str(words))
    with pytest.raises(ValueError):
        brute_force.init(STREAM, None, ["a"], wordlist=str(words))
    with pytest.raises(ValueError, match=r"\?w"):
        brute_force.init(STREAM, None, None, wordlist=str(words), mask="?d?d")


def test_checkpoint_key_separates_hybrid_and_mask_searches(tmp_path):
    data = ["pdf", "5", "5"]
    words = [b"sun", b"moon"]
    path = str(tmp_path / "cp.json")
    hy = brute_force.Checkpoint(path, data, mask="?w?d?d", custom=(), wordlist=brute_force.wordlist_key(words))
    assert brute_force.wordlist_key(words)[1] == 2 and len(brute_force.wordlist_key(words)[0]) == 64
    hy.save(1234)
    assert hy.load() == (1234, None)
    saved = json.load(open(path))
    assert saved["words"] == 2 and saved["hybrid_mask"] == "?w?d?d" and "mask" not in saved
    for other in (brute_force.Checkpoint(path, data, mask="?w?d?d", custom=()),           # a mask search
                  brute_force.Checkpoint(path, data, mask="?d?d", custom=()),
                  brute_force.Checkpoint(path, data, LOWER, 4),                            # a range search
                  brute_force.Checkpoint(path, data, mask="?w?d?d", wordlist=brute_force.wordlist_key(words + [b"x"])),
                  brute_force.Checkpoint(path, data, mask="?w?d?d", wordlist=brute_force.wordlist_key([b"moon", b"sun"])),
                  brute_force.Checkpoint(path, data, mask="?w?d", wordlist=brute_force.wordlist_key(words)),
                  brute_force.Checkpoint(path, data, mask="?w?d?d", custom=("ab",),
                                         wordlist=brute_force.wordlist_key(words)),
                  brute_force.Checkpoint(path, data, mask="?w?d?d", target="owner",
                                         wordlist=brute_force.wordlist_key(words))):
        with pytest.raises(ValueError, match="different search"):
            other.load()
    # ... and the reverse: a mask search's file is no hybrid search's
    mk = brute_force.Checkpoint(path, data, mask="?d?d", custom=())
    mk.save(7)
    assert mk.load() == (7, None)
    for other in (hy, brute_force.Checkpoint(path, data, mask="?d?d", wordlist=brute_force.wordlist_key(words))):
        with pytest.raises(ValueError, match="different search"):
            other.load()
