"""k_pdf_r6 / k_pdf_r6_owner on passwords chosen for the path they take, not met by luck.

The R6 hash does not depend on the bytes it is compared with, so tests/r6_plant.py makes any password the password of
one base stream (tests/golden/r6_traces.json) for one CPU hash.  That gives a document per case:

  (1) every user length 0..176: the document of length L hits at [L] among one word of every length -- each launch
      ragged, short slots and long records mixed; 177 bytes stay refused
  (2) every owner length 1..64 the same way; user mode finds none of the owner words
  (3) the fixture's strata -- the exit rule `i >= 64 && i >= last + 32` at its equality edges, one round past them, and
      the longest traces a 2^17 scan found (109 rounds: the 14-bit round field of state[] holds 16,383; 128 rounds are
      about 1e-8 per candidate, out of reach of any scan a fixture can afford) -- in a range window and in a list
  (4) range-mode positions of one 2^19 window (one launch; with 1,024 slots a workgroup and 256 CUs its second half is
      served by refill): first and last candidate, wave, slot-group and workgroup edges

All expectations are exact.  tests/test_r6_trace_model.py checks the helper and the fixture on the CPU.
"""
import pytest

import r6_plant as P

pytestmark = pytest.mark.gpu

O = P.O
FX = P.fixture()
ENTRIES = FX["entries"]
CS16, LOWER = FX["charset"], "abcdefghijklmnopqrstuvwxyz"


@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device: GPU tests need the MI355X box"
    return _lib


# ---------------------------------------------------------------- (1) every length, user
# A launch lasts as long as its longest candidate, and one R6 candidate of 64 (176) bytes takes a slot about 0.2 s
# (0.35 s) whatever else runs: the two calls of one length cost about 0.8 s, so four lengths make a case
USER_GROUPS = [list(range(s, min(s + 4, P.MAX_LEN + 1))) for s in range(0, P.MAX_LEN + 1, 4)]


@pytest.mark.parametrize("lens", USER_GROUPS, ids=["%d-%d" % (g[0], g[-1]) for g in USER_GROUPS])
def test_every_user_length(dprf, lens):
    words, hashes = P.length_words("user")
    base = P.base_fields()
    for L in lens:
        assert len(words[L]) == L
        with dprf.Context(P.plant(base, words[L], "user", hashes[L]), device=0) as ctx:
            hits, n, st = ctx.verify_list(words)
            assert (hits, n) == ([L], 1) and st["candidates"] == len(words), L
            assert ctx.verify_list(words, stop_on_first=True, cap=1)[0] == [L], L


def test_177_bytes_are_still_refused(dprf):
    words, hashes = P.length_words("user")
    with dprf.Context(P.plant(P.base_fields(), words[176], "user", hashes[176]), device=0) as ctx:
        with pytest.raises(dprf.DprfError) as ei:
            ctx.verify_list([words[176], b"x" * 177])
        assert ei.value.code == dprf.E_DOMAIN and "176" in str(ei.value)
        assert ctx.verify_list([b"x" * 176, words[176]])[0] == [1]          # the context still serves


# ---------------------------------------------------------------- (2) every length, owner
# 7/8: the first message pw || O[32:40] || U[0:48] reaches 64 bytes; 47/48: the SHA-256 period reaches 128;
# 63/64: the last two-block first message and the only three-block one
OWNER_GROUPS = ([list(range(1, 4)), list(range(4, 7)), [7, 8]] +
                [list(range(s, min(s + 5, 47))) for s in range(9, 47, 5)] + [[47, 48]] +
                [list(range(s, min(s + 5, 63))) for s in range(49, 63, 5)] + [[63, 64]])
assert sorted(sum(OWNER_GROUPS, [])) == list(range(1, 65))


@pytest.mark.parametrize("lens", OWNER_GROUPS, ids=["%d-%d" % (g[0], g[-1]) for g in OWNER_GROUPS])
def test_every_owner_length(dprf, lens):
    words, hashes = P.length_words("owner")
    base = P.base_fields()
    for L in lens:
        assert len(words[L - 1]) == L
        with dprf.Context(P.plant(base, words[L - 1], "owner", hashes[L - 1]), device=0, pdf_password="owner") as ctx:
            assert ctx.kernel == "pdf_r6_owner"
            hits, n, st = ctx.verify_list(words)
            assert (hits, n) == ([L - 1], 1) and st["candidates"] == len(words), L
            assert ctx.verify_list(words, stop_on_first=True, cap=1)[0] == [L - 1], L
            ctx.set_pdf_password("user")
            assert ctx.verify_list(words)[:2] == ([], 0), L


# ---------------------------------------------------------------- (3) strata
def _decoys(lo, hi):
    """64 printable words of 64 different lengths in lo..hi, without lower-case letters: none is a fixture password."""
    return [bytes(48 + (3 * j + 5 * k + k * k) % 43 for k in range(lo + (41 * j + 5) % (hi - lo + 1)))
            for j in range(64)]


@pytest.mark.parametrize("e", ENTRIES, ids=[e["name"] for e in ENTRIES])
def test_stratum_in_a_range_window(dprf, e):
    idx = e["index"]
    start = max(0, idx - 300)
    with dprf.Context(P.plant(P.base_fields(), e["password"], e["mode"]), device=0, pdf_password=e["mode"]) as ctx:
        hits, n, st = ctx.search_range(CS16, FX["pwlen"], start, idx + 300 - start)
        assert (hits, n) == ([idx], 1) and st["candidates"] == idx + 300 - start
        assert ctx.search_range(CS16, FX["pwlen"], start, idx + 300 - start, stop_on_first=True, cap=1)[0] == [idx]


@pytest.mark.parametrize("e", ENTRIES, ids=[e["name"] for e in ENTRIES])
def test_stratum_in_a_list(dprf, e):
    words = _decoys(0, P.MAX_LEN) if e["mode"] == "user" else _decoys(1, P.OWNER_MAX_LEN)
    assert len(set(map(len, words))) == 64
    at = 5 + e["index"] % 59
    words.insert(at, e["password"].encode())
    assert len(words) == 65 and words.count(words[at]) == 1
    with dprf.Context(P.plant(P.base_fields(), e["password"], e["mode"]), device=0, pdf_password=e["mode"]) as ctx:
        assert ctx.verify_list(words)[:2] == ([at], 1)
        assert ctx.verify_list(words, stop_on_first=True, cap=1)[0] == [at]


# ---------------------------------------------------------------- (4) range-mode positions
WINDOW = 1 << 19
START = 123456789
assert START + WINDOW < 26 ** 6
POSITIONS = [0, 63, 64, 767, 768, 1023, 1024, 262143, 262144, 262207, WINDOW - 1,
             (0x9E3779B1 * 1) % WINDOW, (0x9E3779B1 * 2) % WINDOW, (0x9E3779B1 * 3) % WINDOW]
assert len(set(POSITIONS)) == 14


@pytest.mark.parametrize("p", POSITIONS)
def test_range_position(dprf, p):
    pw = O.index_to_password(START + p, LOWER, 6)
    with dprf.Context(P.plant(P.base_fields(), pw, "user"), device=0) as ctx:
        hits, n, st = ctx.search_range(LOWER, 6, START, WINDOW)
        assert (hits, n) == ([START + p], 1) and st["candidates"] == WINDOW and st["launches"] == 1
        assert ctx.search_range(LOWER, 6, START, WINDOW, stop_on_first=True, cap=1)[0] == [START + p]
