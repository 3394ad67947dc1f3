"""Device-spelled hybrid windows (dprf_search_hybrid: k_spell_hybrid + the list kernels) against the oracle: the hit
set of a whole window equals the set pyoracle finds over the same window spelled by this file's own speller (divmod by
the mask's keyspace, divmod over the positions, bytes concatenated in spelling order; the oracle does its own UTF-16LE
conversion and truncation), on one, two and four device lanes, with stop_on_first returning the oracle's lowest.

  (a) a PDF R5 window of 2^16 against list mode over the host-spelled window (a self-comparison)
  (b) ODF `-e` (2-byte check): false positives besides the planted password
  (c) PDF R5 (one SHA-256 per candidate): one planted document per edge of the spelling
  (d) PDF R4: the 32-byte cut inside a character of the word, inside a symbol behind it, and a word over 64 bytes
  (e) Office 2007: words with BMP and surrogate-pair characters, the whole keyspace
  (f) PDF R2 and R6: mixed-width windows whose start is no multiple of 64
  (g) Office Agile (both hashes) against agile_model.verifies
  (h) owner mode (PDF R3)
  (i) the table's life cycle, (j) the refusals, (k) the CLI end to end with a checkpoint

M = 257 cannot be built (257 is prime, a position holds at most 256 symbols): the shapes around the block size are
M = 255, 256 and 258.  Every oracle case has a CPU test of its preconditions on the oracle alone, so no GPU comparison
passes vacuously.  Word tables come from a fixed seed; the oracle's set is computed once per case and shared."""
import functools
import json
import random

import pytest

import test_mask_windows as mw
from test_mask_windows import DEVICE_LISTS, DIGITS, LOWER, R2, R4, R5, R6, SEED, T, _fields, _stream_of

ORACLE_THREADS = 16
R3 = {"R": 3, "length": 128}
ALPHA = LOWER * 3 + "éß€αAZ"                              # mostly ASCII, some 2- and 3-byte characters


def table(n, seed, lo, hi, alpha=ALPHA):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        k = rng.randint(lo, hi)
        out.append("".join(rng.choice(alpha) for _ in range(k)).encode())
    return out


def distinct(words):
    seen, out = set(), []
    for w in words:
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def space(pos):
    n = 1
    for p in pos:
        n *= len(p)
    return n


def spell(words, pos, at, i):
    """Word i // M before mask position `at` of mask index i % M, the last position fastest."""
    w, r = divmod(i, space(pos))
    chars = []
    for p in reversed(pos):
        r, d = divmod(r, len(p))
        chars.append(p[d])
    chars = "".join(reversed(chars))
    return chars[:at].encode() + words[w] + chars[at:].encode()


ODF_WORDS = table(6000, 0x0DF, 3, 10)                     # (b): 6000 words x "-?d?d"
ODF_POS, ODF_AT = ["-", DIGITS, DIGITS], 0
ODF_PW_IDX = 4321 * 100 + 73
WORDS = distinct(table(2600, 0x5E2, 3, 12))               # (c), (f): distinct words of 3..12 characters
LONGS = [w for w in distinct(table(700, 0x5E3, 1, 60)) if len(w) <= 64]     # 1..64 bytes mixed in every block
BIG = [LOWER] * 7                                         # 26^7 = 8.0e9 > 2^32
M_BIG = 26 ** 7
P255, P256, P258 = [T(2, 255)], [T(2)], ["xy", T(3, 129)]
W64 = [b"abc", ("q" * 61 + "€").encode(), b"de"]           # a word of 64 bytes
W60 = [b"r", b"q" * 60, b"s" * 59]
CUT_WORDS = [b"a" * 31, ("x" * 30 + "€").encode(), b"b", ("x" * 30 + "₭").encode(), ("x" * 30 + "é").encode()]
TAIL_WORDS = [b"y" * 29, b"y" * 30, b"y" * 31]
LONG_WORDS = [b"z" * 31 + b"!", b"z" * 70, b"k", ("z" * 40 + "€" * 20).encode(), b"z" * 32]
OFFICE_WORDS = ["a€".encode(), "é\U0001D11E".encode(), "P\U00020000b".encode(), b"zz"]
OFFICE_POS = [DIGITS, "€x\U0001D11E"]
MIX_POS = ["aé€", DIGITS, "\U0001D11Eb"]                   # M = 60, widths 1-4


def _case(kind, kw, words, pos, at, idx, start, count, **more):
    return dict({"kind": kind, "kw": kw, "words": words, "pos": pos, "at": at, "idx": idx, "start": start,
                 "count": count}, **more)


def _r5(words, pos, at, idx, start, count):
    return _case("pdf", R5, words, pos, at, idx, start, count)


def _edge(pos, w, last):
    """A planted candidate that is the first or the last of word w's block of M."""
    m = space(pos)
    idx = w * m + (m - 1 if last else 0)
    return _r5(WORDS, pos, len(pos), idx, idx - 300, 1000)


NW = len(WORDS)
CASES = {
    "b-odf-e-false-positives": None,                      # filled below from ODF_WINDOW
    "b-odf-e-planted": _case("odt_e", {}, ODF_WORDS, ODF_POS, ODF_AT, ODF_PW_IDX, ODF_PW_IDX - 20001, 1 << 15),
    "c-m1-offset-0": _r5(WORDS, [], 0, 1000, 1000, 1000),
    "c-m1-offset-255": _r5(WORDS, [], 0, 1255, 1000, 1000),
    "c-m1-offset-256": _r5(WORDS, [], 0, 1256, 1000, 1000),
    "c-m1-all-lengths": _r5(LONGS, [], 0, 300, 0, 512),
    "c-m10": _r5(WORDS, [DIGITS], 1, 12347, 12347 - 500, 1000),
    "c-m255-first": _edge(P255, 7, False),
    "c-m255-last": _edge(P255, 7, True),
    "c-m256-first": _edge(P256, 9, False),
    "c-m256-last": _edge(P256, 9, True),
    "c-m258-first": _edge(P258, 11, False),
    "c-m258-last": _edge(P258, 11, True),
    "c-big-across-2^32-in-a-word": _r5(WORDS, BIG, 7, (1 << 32) + 5, (1 << 32) - 100, 1000),
    "c-big-word-boundary": _r5(WORDS, BIG, 0, 5 * M_BIG, 5 * M_BIG - 300, 1000),
    "c-big-boundary-at-the-start": _r5(WORDS, BIG, 3, 5 * M_BIG + 999, 5 * M_BIG, 1000),
    "c-keyspace-last": _r5(WORDS, [DIGITS], 0, NW * 10 - 1, NW * 10 - 777, 777),
    "c-count-1": _r5(WORDS, [DIGITS, "-"], 1, 4242, 4242, 1),
    "c-word-of-64-bytes": _r5(W64, [], 0, 1, 0, 3),
    "c-word-and-mask-of-64-bytes": _r5(W60, ["ab", "-", "cd", "e"], 4, 4 + 3, 0, 8),
    "c-word-first": _r5(WORDS, [DIGITS, "-", LOWER], 0, 777 * 260 + 123, 777 * 260 - 200, 1000),
    "c-word-middle": _r5(WORDS, [DIGITS, "-", LOWER], 1, 777 * 260 + 123, 777 * 260 - 200, 1000),
    "c-word-middle-2": _r5(WORDS, [DIGITS, "-", LOWER], 2, 777 * 260 + 123, 777 * 260 - 200, 1000),
    "c-word-last": _r5(WORDS, [DIGITS, "-", LOWER], 3, 777 * 260 + 123, 777 * 260 - 200, 1000),
    "c-one-word": _r5([b"solo"], [DIGITS, DIGITS], 2, 42, 0, 100),
    "d-r4-cut-in-the-word": _case("pdf", R4, CUT_WORDS, [DIGITS], 0, 10 + 3, 0, 50),
    "d-r4-cut-in-a-symbol": _case("pdf", R4, TAIL_WORDS, ["€₭é", "ab"], 0, 6 + 0, 0, 18),
    "d-r4-word-over-64-bytes": _case("pdf", R4, LONG_WORDS, [DIGITS], 0, 10 + 7, 0, 50),
    "e-office": _case("docx", {}, OFFICE_WORDS, OFFICE_POS, 1, 1 * 30 + 7 * 3 + 2, 0, 120),
    "f-pdf-r2": _case("pdf", R2, WORDS, MIX_POS, 1, 60 * 700 + 31, 60 * 700 - 2001, 1 << 12),
    "f-pdf-r6": _case("pdf", R6, WORDS, MIX_POS, 3, 60 * 900 + 59, 60 * 900 - 3003, 1 << 12),
    "h-owner-r3": _case("pdf", R3, WORDS, [DIGITS, DIGITS], 2, 100 * 1500 + 7, 100 * 1500 - 1001, 1 << 11, owner=True),
}
# (b): the oracle over the whole keyspace of ODF_WORDS x "-?d?d" on the planted document (found once; the CPU test
# below checks the windows used against the oracle itself)
ODF_ALL = [10508, 20261, 146497, 222805, 270050, 345829, 402507, 432173, 432447, 465380, 476425, 491283, 517593]
ODF_WINDOW = (465380 - 3333, 1 << 15)                     # three false positives, the planted password outside
CASES["b-odf-e-false-positives"] = _case("odt_e", {}, ODF_WORDS, ODF_POS, ODF_AT, ODF_PW_IDX, ODF_WINDOW[0],
                                         ODF_WINDOW[1], planted_outside=True)
B_CASES = [k for k in CASES if k.startswith("b-")]
C_CASES = [k for k in CASES if k.startswith("c-")]
D_CASES = [k for k in CASES if k.startswith("d-")]
F_CASES = [k for k in CASES if k.startswith("f-")]


def _password(name):
    c = CASES[name]
    return spell(c["words"], c["pos"], c["at"], c["idx"]).decode()


@functools.lru_cache(maxsize=None)
def expected(name):
    """(stream, the oracle's sorted hit indices of the case's window): once per case, for every test that needs it."""
    import pyoracle
    c = CASES[name]
    kw = dict(c["kw"], owner=_password(name)) if c.get("owner") else c["kw"]
    pw = "user" if c.get("owner") else _password(name)
    stream = _stream_of(c["kind"], tuple(sorted(kw.items())), pw)
    window = [spell(c["words"], c["pos"], c["at"], i) for i in range(c["start"], c["start"] + c["count"])]
    if c.get("owner"):
        import owner_model
        return stream, [c["start"] + k for k, w in enumerate(window) if owner_model.owner_verifies(stream, w)]
    verdicts = pyoracle.Ctx(stream).verify_list(window, nthreads=ORACLE_THREADS)
    return stream, [c["start"] + k for k, v in enumerate(verdicts) if v]


def _gpu_equals_oracle(name):
    from dprf_amd import _lib
    c = CASES[name]
    stream, want = expected(name)
    assert want, name
    for devs in DEVICE_LISTS:
        with _lib.Context(_fields(stream), devices=devs, pdf_password="owner" if c.get("owner") else "user") as ctx:
            ctx.set_words(c["words"])
            assert ctx.words == len(c["words"])
            hits, nh, st = ctx.search_hybrid(c["pos"], c["at"], c["start"], c["count"])
            assert hits == want and nh == len(want), (name, devs, hits[:8], want[:8], nh, len(want))
            assert st["candidates"] == c["count"], (name, devs, st)
            first, _, _ = ctx.search_hybrid(c["pos"], c["at"], c["start"], c["count"], stop_on_first=True, cap=1)
            assert first == want[:1], (name, devs, first, want[:1])


def test_cases_lie_inside_their_keyspaces():
    for name, c in CASES.items():
        n = len(c["words"]) * space(c["pos"])
        assert all(len(set(p)) == len(p) and 1 <= len(p) <= 256 for p in c["pos"]) and len(c["pos"]) <= 32, name
        assert 0 <= c["at"] <= len(c["pos"]) and 0 <= c["start"] and c["start"] + c["count"] <= n, name
        assert c.get("planted_outside") or c["start"] <= c["idx"] < c["start"] + c["count"], name
        assert c["count"] <= (1024 if name in C_CASES else 1 << 15), name
    assert NW >= 2500 and len(set(WORDS)) == NW and len(LONGS) >= 512
    assert len({len(w) for w in LONGS[:256]}) >= 48 and {1, 64} <= {len(w) for w in LONGS[:512]}
    assert any(len(w.decode()) != len(w) for w in WORDS[1000:1256])         # multi-byte characters in the block
    assert [space(p) for p in (P255, P256, P258)] == [255, 256, 258] and M_BIG > 1 << 32
    assert [CASES["c-m1-offset-" + k]["idx"] - 1000 for k in ("0", "255", "256")] == [0, 255, 256]
    for k in ("255", "256", "258"):
        m = int(k)
        assert CASES["c-m%s-first" % k]["idx"] % m == 0 and CASES["c-m%s-last" % k]["idx"] % m == m - 1
    c = CASES["c-big-across-2^32-in-a-word"]
    assert c["start"] < 1 << 32 < c["start"] + c["count"] and (c["start"] + c["count"]) // M_BIG == 0
    assert CASES["c-big-word-boundary"]["idx"] % M_BIG == 0 and CASES["c-big-boundary-at-the-start"]["start"] % M_BIG == 0
    assert CASES["c-keyspace-last"]["idx"] == NW * 10 - 1 and CASES["c-count-1"]["count"] == 1
    assert len(W64[1]) == 64 and len(spell(W60, CASES["c-word-and-mask-of-64-bytes"]["pos"], 4, 7)) == 64
    assert len(CASES["c-one-word"]["words"]) == 1
    assert CUT_WORDS[1][:32] == CUT_WORDS[3][:32] != CUT_WORDS[4][:32] and CUT_WORDS[1][30:32] == b"\xe2\x82"
    assert max(len(w) for w in LONG_WORDS) > 64
    assert ODF_WINDOW[0] % 64 and ODF_WINDOW[0] % 100 and len(ODF_WORDS) == 6000
    for name in F_CASES:
        assert CASES[name]["start"] % 64 and CASES[name]["count"] == 1 << 12, name
    assert [len(ch.encode("utf-16-le")) for ch in _password("e-office")] == [2, 2, 4, 4]


# ------------------------------------------------------------------ (a) self-comparison
@pytest.mark.gpu
def test_hybrid_window_equals_list_mode_of_the_spelled_window():
    from dprf_amd import _lib
    pos, at = [DIGITS, "-", "aé€", DIGITS], 2
    start, count = 300 * 1111 + 17, 1 << 16
    idx = start + 40000
    stream = _stream_of("pdf", tuple(sorted(R5.items())), spell(WORDS, pos, at, idx).decode())
    window = [spell(WORDS, pos, at, i) for i in range(start, start + count)]
    for devs in DEVICE_LISTS:
        with _lib.Context(_fields(stream), devices=devs) as ctx:
            ctx.set_words(WORDS)
            a = ctx.search_hybrid(pos, at, start, count)
            b = ctx.verify_list(window)
            assert a[0] == [start + h for h in b[0]] == [idx] and a[1] == b[1] == 1, (devs, a[:2], b[:2])
            assert a[2]["candidates"] == b[2]["candidates"] == count
            assert ctx.search_hybrid(pos, at, start, count, stop_on_first=True, cap=1)[0] == [idx]


# ------------------------------------------------------------------ (b) ODF -e: false positives
def test_odf_e_windows_on_the_oracle():
    lo, n = ODF_WINDOW
    want = [h for h in ODF_ALL if lo <= h < lo + n]
    assert want == [465380, 476425, 491283] and ODF_PW_IDX not in want and ODF_PW_IDX in ODF_ALL
    assert (lo // 100) * 100 != lo                                          # the start falls inside a word
    assert expected("b-odf-e-false-positives")[1] == want
    c = CASES["b-odf-e-planted"]
    assert expected("b-odf-e-planted")[1] == [h for h in ODF_ALL if c["start"] <= h < c["start"] + c["count"]]
    assert expected("b-odf-e-planted")[1] == [ODF_PW_IDX, 432447]


@pytest.mark.gpu
@pytest.mark.parametrize("name", B_CASES)
def test_odf_e_window_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ (c) PDF R5: one document per edge
@pytest.mark.parametrize("name", C_CASES)
def test_pdf_r5_edge_is_the_only_hit_on_the_oracle(name):
    assert expected(name)[1] == [CASES[name]["idx"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", C_CASES)
def test_pdf_r5_planted_edge_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ (d) PDF R4: the 32-byte cut
def test_pdf_r4_cuts_on_the_oracle():
    """x * 30 + € and x * 30 + ₭ share their first 32 bytes (E2 82 before the cut), whatever follows; so do y * 30 + €
    and y * 30 + ₭; and every word that starts with 32 z."""
    assert expected("d-r4-cut-in-the-word")[1] == list(range(10, 20)) + list(range(30, 40))
    assert expected("d-r4-cut-in-a-symbol")[1] == [6, 7, 8, 9]
    assert expected("d-r4-word-over-64-bytes")[1] == list(range(10, 20)) + list(range(30, 50))


@pytest.mark.gpu
@pytest.mark.parametrize("name", D_CASES)
def test_pdf_r4_cut_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ (e) Office 2007
def test_office_keyspace_has_one_hit_on_the_oracle():
    assert expected("e-office")[1] == [CASES["e-office"]["idx"]]


@pytest.mark.gpu
def test_office_whole_keyspace_equals_oracle():
    _gpu_equals_oracle("e-office")


# ------------------------------------------------------------------ (f) PDF R2 and R6
@pytest.mark.parametrize("name", F_CASES)
def test_mixed_width_window_has_one_hit_on_the_oracle(name):
    assert expected(name)[1] == [CASES[name]["idx"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", F_CASES)
def test_mixed_width_window_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ (g) Office Agile
@pytest.mark.gpu
@pytest.mark.parametrize("version,bits", [("2010", 128), ("2013", 256)])
def test_agile_window_equals_the_model(version, bits):
    import agile_model
    from dprf_amd import _lib
    words, pos, at = OFFICE_WORDS + [b"summer"], [DIGITS, "€x"], 1
    start, count = 13, 80
    idx = 4 * 20 + 11
    pw = spell(words, pos, at, idx).decode()
    stream = agile_model.make_stream(pw, version, bits, 1000, seed=0xA61 + bits)
    want = [i for i in range(start, start + count) if agile_model.verifies(stream, spell(words, pos, at, i).decode())]
    assert want == [idx]
    for devs in DEVICE_LISTS:
        with _lib.Context(agile_model.fields_of(stream), devices=devs) as ctx:
            ctx.set_words(words)
            hits, nh, st = ctx.search_hybrid(pos, at, start, count)
            assert hits == want and nh == 1 and st["candidates"] == count, (version, devs, hits, st)
            assert ctx.search_hybrid(pos, at, start, count, stop_on_first=True, cap=1)[0] == want


# ------------------------------------------------------------------ (h) owner mode
def test_owner_window_has_one_hit_on_the_model():
    assert expected("h-owner-r3")[1] == [CASES["h-owner-r3"]["idx"]]


@pytest.mark.gpu
def test_owner_window_equals_the_model():
    _gpu_equals_oracle("h-owner-r3")


# ------------------------------------------------------------------ (i) the table's life cycle
@pytest.mark.gpu
def test_table_life_cycle():
    from dprf_amd import _lib
    pos = [DIGITS]
    first, second = [b"sun", b"moon", b"star"], [b"star", b"sun", b"sun", b"moon!"]
    stream = _stream_of("pdf", tuple(sorted(R5.items())), "sun7")
    with _lib.Context(_fields(stream), devices=[0, 0]) as ctx, _lib.Context(_fields(stream), device=0) as other:
        before = (ctx.search_mask([LOWER, LOWER, LOWER, DIGITS], 0, 26 ** 3 * 10)[:2],
                  ctx.search_range(LOWER + DIGITS, 4, 0, 36 ** 4)[:2], ctx.verify_list(["sun7", "moon7", "sun7"])[:2])
        assert before[0][1] == before[1][1] == 1 and before[2][0] == [0, 2]
        assert ctx.words == 0
        ctx.set_words(first)
        other.set_words(second)
        assert ctx.words == 3 and other.words == 4
        assert ctx.search_hybrid(pos, 0, 0, 30)[0] == [7]
        assert other.search_hybrid(pos, 0, 0, 40)[0] == [17, 27]            # a repeated word is verified twice
        assert ctx.search_hybrid(pos, 0, 0, 30)[0] == [7]                   # two contexts, one device: no mixing
        ctx.set_words(second)                                               # the results follow the second table
        assert ctx.words == 4 and ctx.search_hybrid(pos, 0, 0, 40)[0] == [17, 27]
        assert ctx.search_hybrid(pos, 0, 0, 40, stop_on_first=True, cap=1)[0] == [17]
        with pytest.raises(_lib.DprfError) as ei:                           # a refused table keeps the old one
            ctx.set_words([b"sun", b"", b"x"])
        assert ei.value.code == _lib.E_DOMAIN and "word 1" in str(ei.value)
        assert ctx.words == 4 and ctx.search_hybrid(pos, 0, 0, 40)[0] == [17, 27]
        after = (ctx.search_mask([LOWER, LOWER, LOWER, DIGITS], 0, 26 ** 3 * 10)[:2],
                 ctx.search_range(LOWER + DIGITS, 4, 0, 36 ** 4)[:2], ctx.verify_list(["sun7", "moon7", "sun7"])[:2])
        assert after == before
        ctx.set_words([])                                                   # cleared
        assert ctx.words == 0
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_hybrid(pos, 0, 0, 1)
        assert ei.value.code == _lib.E_INVALID and ctx.last_call_devices() == []
        assert other.search_hybrid(pos, 0, 0, 40)[0] == [17, 27]


# ------------------------------------------------------------------ (j) refusals
def _refused(ctx, code, pos, at, start, count, serve):
    from dprf_amd import _lib
    with pytest.raises(_lib.DprfError) as ei:
        ctx.search_hybrid(pos, at, start, count)
    assert ei.value.code == code, (ei.value, [len(p) for p in pos], at, start, count)
    assert ctx.last_call_devices() == []                                    # a refused call leaves no record
    assert serve() == [7]                                                   # ... and the context still serves
    return str(ei.value)


@pytest.mark.gpu
def test_refusals_after_each_of_which_the_context_serves():
    from dprf_amd import _lib
    words = [b"sun", b"m" * 60, b"star"]
    stream = _stream_of("pdf", tuple(sorted(R5.items())), "sun7")
    with _lib.Context(_fields(stream), device=0) as ctx:                    # PDF R5: candidates cut at 127 bytes
        with pytest.raises(_lib.DprfError) as ei:                           # no table yet
            ctx.search_hybrid([DIGITS], 0, 0, 1)
        assert ei.value.code == _lib.E_INVALID and ctx.last_call_devices() == []
        ctx.set_words(words)
        serve = lambda: ctx.search_hybrid([DIGITS], 0, 0, 10)[0]
        assert serve() == [7]
        bad = [
            (_lib.E_INVALID, [DIGITS], 2, 0, 1),                            # word_at outside 0..npos
            (_lib.E_INVALID, [DIGITS], -1, 0, 1),
            (_lib.E_INVALID, [], 1, 0, 1),
            (_lib.E_INVALID, [DIGITS], 0, 0, 31),                           # start + count over N * M
            (_lib.E_INVALID, [DIGITS], 0, 30, 1),
            (_lib.E_INVALID, [DIGITS], 0, 29, 2),
            (_lib.E_INVALID, [], 0, 3, 1),
            (_lib.E_PWLEN, ["a"] * 33, 0, 0, 1),                            # 33 positions
            (_lib.E_CHARSET, [DIGITS, ""], 0, 0, 1),                        # the mask's own rules
            (_lib.E_CHARSET, [DIGITS, "aba"], 0, 0, 1),
            (_lib.E_CHARSET, [DIGITS, b"a\0"], 0, 0, 1),
        ]
        for code, pos, at, start, count in bad:
            _refused(ctx, code, pos, at, start, count, serve)
        msg = _refused(ctx, _lib.E_PWLEN, ["-", "€", "a"], 0, 0, 1, serve)  # 60 + 5 bytes: names the word
        assert "word 1" in msg
        assert ctx.search_hybrid(["-", "€"], 0, 0, 3)[2]["candidates"] == 3  # 60 + 4 fill the slot
        # set_words' refusals, and words_status' codes for the same words
        assert ctx.search_hybrid([DIGITS], 1, 0, 0)[2]["candidates"] == 0
        for table_, k in (([b"a", b""], 1), ([b"a\0b"], 0), ([b"ok", b"ok", b"x\0"], 2)):
            with pytest.raises(_lib.DprfError) as ei:
                ctx.set_words(table_)
            assert ei.value.code == _lib.E_DOMAIN and "word %d" % k in str(ei.value), ei.value
            st = ctx.words_status(table_)
            assert [int(x) for x in st] == [_lib.E_DOMAIN if j == k else 0 for j in range(len(table_))]
            assert ctx.words == 3 and serve() == [7]
        assert [int(x) for x in ctx.words_status([b"\xff\xfe", b"x" * 5000])] == [0, 0]   # raw bytes, any length
        ctx.set_words([b"\xff\xfe", b"x" * 5000, b"sun"])                   # held; the search refuses the long word
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_hybrid([DIGITS], 0, 0, 1)
        assert ei.value.code == _lib.E_PWLEN and "word 1" in str(ei.value) and ctx.last_call_devices() == []
    # Office: words are UTF-8; PDF R2-R4: a word of any length fits the 32-byte cut
    office, _ = mw.expected("c-office-mixed")
    with _lib.Context(_fields(office), device=0) as ctx:
        assert [int(x) for x in ctx.words_status([b"ok", b"\xff", b"", "é".encode()])] == [0, _lib.E_DOMAIN,
                                                                                          _lib.E_DOMAIN, 0]
        with pytest.raises(_lib.DprfError) as ei:
            ctx.set_words([b"ok", b"\xff"])
        assert ei.value.code == _lib.E_DOMAIN and "word 1" in str(ei.value) and ctx.words == 0
        ctx.set_words([("€" * 32).encode()])                                # 64 bytes of UTF-16LE
        assert ctx.search_hybrid([], 0, 0, 1)[2]["candidates"] == 1
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_hybrid(["a"], 0, 0, 1)
        assert ei.value.code == _lib.E_PWLEN
    r4, _ = mw.expected("b-pdf-r4-cut")
    with _lib.Context(_fields(r4), device=0) as ctx:
        ctx.set_words([b"x" * 5000, b"y"])
        assert ctx.search_hybrid(["a€"] * 22, 11, 0, 10)[2]["candidates"] == 10
        # a keyspace over 2^64 (N * M = 2 * 256^8): a window below 2^64 is searched, the binding refuses one at 2^64
        cap8 = [T(k) for k in range(8)]
        assert ctx.search_hybrid(cap8, 8, (1 << 64) - 1001, 1000)[2]["candidates"] == 1000
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_hybrid(cap8, 8, 0, 1 << 64)
        assert ei.value.code == _lib.E_INVALID
        with pytest.raises(_lib.DprfError) as ei:                           # N * M = 2 * 26^7: just over it
            ctx.search_hybrid(BIG, 0, 2 * M_BIG - 5, 6)
        assert ei.value.code == _lib.E_INVALID and ctx.last_call_devices() == []
        assert ctx.search_hybrid(BIG, 0, 2 * M_BIG - 6, 6)[2]["candidates"] == 6


@pytest.mark.gpu
def test_never_matching_context_counts_the_window():
    from dprf_amd import _lib
    fields = ["pdf", "2", "4", "128", "-4", "1", "16", "11" * 16, "32", "22" * 32, "32", "33" * 32]
    with _lib.Context(fields, device=0) as ctx:
        assert ctx.flags & _lib.FLAG_NEVER_MATCHES
        ctx.set_words([b"sun", b"moon"])
        hits, nh, st = ctx.search_hybrid([DIGITS], 0, 3, 15)
        assert hits == [] and nh == 0 and st["candidates"] == 15 and ctx.words == 2
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_hybrid([DIGITS], 0, 3, 18)
        assert ei.value.code == _lib.E_INVALID


# ------------------------------------------------------------------ (k) the CLI, with a checkpoint
@pytest.mark.gpu
def test_cli_hybrid_end_to_end_and_checkpoint_resume(tmp_path, capsys):
    import docgen
    from dprf_amd import brute_force, hybrid
    pdf = str(tmp_path / "budget.pdf")
    words = [b"spring", b"", b"summer", "hiver€".encode(), b"q" * 70, b"autumn"]
    wl = tmp_path / "words.txt"
    wl.write_bytes(b"spring\r\n\nsummer\nhiver\xe2\x82\xac\n" + b"q" * 70 + b"\nautumn\n")
    password = "hiver€24"
    docgen.write_pdf(pdf, password, SEED, **R5)
    argv = ["3", pdf, "--wordlist", str(wl), "--mask", "?w?d?d"]
    capsys.readouterr()
    assert brute_force.main(argv) == (1, password)
    assert "Dropped 1 words too long" in capsys.readouterr().out
    kept = [w for w in words if w and len(w) <= 62]
    pos, at = hybrid.parse_hybrid("?w?d?d")
    idx = hybrid.index_of(kept, pos, at, password)
    assert idx == 224 and hybrid.space(len(kept), pos) == 400
    # a checkpoint written mid-search resumes at its cursor ...
    cp = str(tmp_path / "cursor.json")
    data = brute_force.parse_verification_data(brute_force.get_verification_data("3", pdf))
    read = hybrid.read_wordlist(str(wl))
    assert read == [w for w in words if w]
    key = brute_force.Checkpoint(cp, data, mask="?w?d?d", custom=(), wordlist=brute_force.wordlist_key(read))
    key.save(100)
    capsys.readouterr()
    assert brute_force.main(argv + ["--checkpoint", cp]) == (1, password)
    assert "Checkpoint: resuming at index 100" in capsys.readouterr().out
    assert json.load(open(cp))["found"] == password and json.load(open(cp))["next_index"] == 400
    # ... also when the cursor lies past the password: the indices below it are not searched again
    key.save(idx + 1)
    assert brute_force.main(argv + ["--checkpoint", cp]) == (0, brute_force.DEFAULT_PASSWORD)
    # a changed wordlist is refused by the checkpoint
    wl.write_bytes(wl.read_bytes() + b"winter\n")
    with pytest.raises(ValueError):
        brute_force.main(argv + ["--checkpoint", cp])
    # the bare --wordlist: the word over 64 bytes is the password, verified as a list at the end
    long_pdf = str(tmp_path / "long.pdf")
    docgen.write_pdf(long_pdf, "q" * 70, SEED, **R5)
    capsys.readouterr()
    assert brute_force.main(["3", long_pdf, "--wordlist", str(wl)]) == (1, "q" * 70)
    assert "verified as a list at the end" in capsys.readouterr().out
