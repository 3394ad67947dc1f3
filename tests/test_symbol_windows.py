"""Device-spelled symbol windows (dprf_search_symbols, k_spell_symbols + the list kernels) against the oracle, both
directions: the hit set of a whole window equals the set pyoracle finds over the same window spelled by this file's own
speller (divmod digits, "".join(...).encode(); the oracle does its own UTF-16LE conversion and truncation), on one,
two and four device lanes, with stop_on_first returning the oracle's lowest.  tests/test_symbols.py compares the device
spelling with payload.spell_utf8 through the same list kernels and looks for one planted index; here every index of
the window counts, and the windows are chosen where a spelling error would change the set:

  (a) ODF `-e` (2-byte check): false positives besides the planted password, so a window with several hits
  (b) PDF R4: the 32-byte truncation falls inside a 3-byte character; two runs of 64 candidates verify
  (c) Office: ASCII, BMP and surrogate-pair symbols in one table, the whole keyspace
  (d) PDF R5 (one SHA-256 per candidate): one document per edge of the spelling -- window offsets 0 / 255 / 256 /
      count - 1, a carry through 7 positions, the last index of a keyspace, tables of 1, 2, 255 and 256 symbols, 32
      two-byte symbols filling the slot, indices past 2^32
  (e) PDF R2 and R6: mixed-width windows whose start is no multiple of 64

Every case has a CPU test of its preconditions on the oracle alone, so the GPU comparison cannot pass vacuously.  The
oracle's set is computed once per case and shared."""
import contextlib
import functools
import io
import os
import tempfile

import pytest

SEED = 0x5E1
ORACLE_THREADS = 16
DEVICE_LISTS = ([0], [0, 0], [0, 0, 0, 0])

GREEK = "αβγδεζηθικλμνξοπρστυφχψω"                       # 24 two-byte symbols
CUT = "a€é₭"                                              # € = E2 82 AC, ₭ = E2 82 AD
MIXED = "aé€\U0001D11Eb"                                  # 1, 2, 3, 4, 1 UTF-8 bytes
OFFICE = "aé€\U0001D11E\U00020000b"                       # UTF-16 units 1, 1, 1, 2, 2, 1
BMP255 = "".join(chr(0x100 + k) for k in range(255))      # U+0100 .. : every one a valid two-byte character
BMP256 = "".join(chr(0x100 + k) for k in range(256))


def word(i, cs, n):
    """itertools.product order (brute_force.py:205): the last character varies fastest."""
    out = []
    for _ in range(n):
        i, r = divmod(i, len(cs))
        out.append(cs[r])
    return "".join(reversed(out))


def index_of(pw, cs):
    i = 0
    for ch in pw:
        i = i * len(cs) + cs.index(ch)
    return i


def _stream(kind, kw, pw):
    import docgen
    from dprf_amd.parsers import odt2hashes, office2john, pdf2john
    with tempfile.TemporaryDirectory() as t:
        if kind == "docx":
            p = os.path.join(t, "d.docx")
            docgen.write_docx(p, pw, SEED)
            return office2john.get_hash(p)
        if kind == "odt_e":
            p = os.path.join(t, "d.odt")
            docgen.write_odt(p, pw, SEED)
            return odt2hashes.get_hashes(p, True)
        p = os.path.join(t, "d.pdf")
        docgen.write_pdf(p, pw, SEED, **kw)
        return pdf2john.get_hash(p)


def _fields(stream):
    from dprf_amd.brute_force import parse_verification_data
    with contextlib.redirect_stdout(io.StringIO()):
        return parse_verification_data(stream)


R4, R5 = {"R": 4, "length": 128}, {"R": 5, "length": 256}
P10 = index_of("€" * 10, CUT)                             # (b): the candidates "€" * 10 + 4 more are P10 * 256 + ..


def _case(kind, kw, cs, n, idx, start, count):
    return {"kind": kind, "kw": kw, "cs": cs, "n": n, "idx": idx, "start": start, "count": count}


def _r5(cs, n, idx, start, count):
    return _case("pdf", R5, cs, n, idx, start, count)


CASES = {
    "a-odf-e-greek4": _case("odt_e", {}, GREEK, 4, index_of("σμψβ", GREEK), 212992, 1 << 15),
    "b-pdf-r4-cut": _case("pdf", R4, CUT, 14, index_of("€" * 11 + "aaa", CUT), P10 * 256 - (1 << 15), 1 << 16),
    "c-office-mixed": _case("docx", {}, OFFICE, 4, index_of("€\U0001D11Eb\U00020000", OFFICE), 0, 6 ** 4),
    # (e) at length 6: a window of 2^12 does not fit the 5^5 = 3125 indices of length 5
    "e-pdf-r2": _case("pdf", {"R": 2, "length": 40}, MIXED, 6, 7777, 5037, 1 << 12),
    "e-pdf-r6": _case("pdf", {"R": 6, "length": 256}, MIXED, 6, 13000, 5 ** 6 - (1 << 12) - 3, 1 << 12),
    # (d): (charset, length, planted index, window start, window count <= 1024)
    "d-offset-0": _r5(MIXED, 5, 1000, 1000, 1000),
    "d-offset-255": _r5(MIXED, 5, 1255, 1000, 1000),
    "d-offset-256": _r5(MIXED, 5, 1256, 1000, 1000),
    "d-offset-count-1": _r5(MIXED, 5, 1999, 1000, 1000),
    "d-carry-7-positions": _r5(MIXED, 8, 5 ** 7, 5 ** 7 - 3, 600),
    "d-keyspace-last": _r5(MIXED, 5, 5 ** 5 - 1, 5 ** 5 - 777, 777),
    "d-table-1": _r5("é", 32, 0, 0, 1),
    "d-table-2": _r5("a\U0001D11E", 10, 0b1010101011, 0, 1 << 10),
    "d-table-255-len2-last254": _r5(BMP255, 2, 17 * 255 + 254, 17 * 255 + 254 - 300, 700),
    "d-table-255-len3-first254": _r5(BMP255, 3, 254 * 255 ** 2 + 3 * 255 + 254, 254 * 255 ** 2 + 3 * 255 - 2, 1024),
    "d-table-256-len2-both255": _r5(BMP256, 2, 256 ** 2 - 1, 256 ** 2 - 1000, 1000),
    "d-table-256-len3-mid254": _r5(BMP256, 3, 7 * 256 ** 2 + 254 * 256 + 255, 7 * 256 ** 2 + 254 * 256 - 3, 1024),
    "d-table-256-len3-first255": _r5(BMP256, 3, 255 * 256 ** 2 + 255, 255 * 256 ** 2 - 100, 700),
    "d-slot-filled-32x2": _r5("αβ", 32, 0xDEADBEEF, 0xDEADBEEF - 500, 1000),
    "d-slot-filled-last": _r5("αβ", 32, (1 << 32) - 1, (1 << 32) - 333, 333),
    "d-past-2^32": _r5(MIXED, 16, (1 << 32) + 98765, (1 << 32) + 98765 - 321, 1024),
    "d-across-2^32": _r5(MIXED, 16, (1 << 32) + 5, (1 << 32) - 100, 1000),
}
D_CASES = [k for k in CASES if k.startswith("d-")]
E_CASES = [k for k in CASES if k.startswith("e-")]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(stream, the oracle's sorted hit indices of the case's window): once per case, for every test that needs it."""
    import pyoracle
    c = CASES[name]
    stream = _stream(c["kind"], c["kw"], word(c["idx"], c["cs"], c["n"]))
    window = [word(i, c["cs"], c["n"]).encode() for i in range(c["start"], c["start"] + c["count"])]
    verdicts = pyoracle.Ctx(stream).verify_list(window, nthreads=ORACLE_THREADS)
    return stream, [c["start"] + k for k, v in enumerate(verdicts) if v]


def _gpu_equals_oracle(name):
    from dprf_amd import _lib
    c = CASES[name]
    stream, want = expected(name)
    assert want, name
    for devs in DEVICE_LISTS:
        with _lib.Context(_fields(stream), devices=devs) as ctx:
            hits, nh, st = ctx.search_symbols(c["cs"], c["n"], c["start"], c["count"])
            assert hits == want and nh == len(want), (name, devs, hits[:8], want[:8], nh, len(want))
            assert st["candidates"] == c["count"], (name, devs, st)
            first, _, _ = ctx.search_symbols(c["cs"], c["n"], c["start"], c["count"], stop_on_first=True, cap=1)
            assert first == want[:1], (name, devs, first, want[:1])


def test_cases_lie_inside_their_keyspaces():
    assert len(D_CASES) <= 24
    for name, c in CASES.items():
        space = len(c["cs"]) ** c["n"]
        assert len(set(c["cs"])) == len(c["cs"]) and c["count"] <= 1 << 16, name
        assert 0 <= c["start"] <= c["idx"] < c["start"] + c["count"] <= space, name
        if name in D_CASES:
            assert c["count"] <= 1024, name
    for name in E_CASES:
        assert CASES[name]["start"] % 64 and CASES[name]["count"] == 1 << 12, name
    assert [CASES["d-offset-" + k]["idx"] - 1000 for k in ("0", "255", "256", "count-1")] == [0, 255, 256, 999]
    assert word(CASES["d-carry-7-positions"]["start"], MIXED, 8) == "a" + "b" * 6 + "€"   # b is digit nsym - 1
    assert word(CASES["d-carry-7-positions"]["idx"], MIXED, 8) == "é" + "a" * 7
    assert len(word(0, "αβ", 32).encode()) == 64 and CASES["d-past-2^32"]["start"] > 1 << 32
    assert all(len(ch.encode()) == 2 for ch in BMP256) and BMP255 == BMP256[:255]
    for name, pos, dig in (("d-table-255-len2-last254", 1, 254), ("d-table-255-len3-first254", 0, 254),
                           ("d-table-256-len2-both255", 0, 255), ("d-table-256-len3-mid254", 1, 254),
                           ("d-table-256-len3-first255", 0, 255)):
        c = CASES[name]
        assert c["cs"].index(word(c["idx"], c["cs"], c["n"])[pos]) == dig, name


# ------------------------------------------------------------------ (a) ODF -e: false positives
def test_odf_e_window_has_false_positives_on_the_oracle():
    c = CASES["a-odf-e-greek4"]
    assert c["idx"] == 241873
    _, want = expected("a-odf-e-greek4")
    others = [h for h in want if h != c["idx"]]
    assert c["idx"] in want and len(others) >= 2, \
        "the window needs the planted index %d and at least 2 false positives; the oracle found %r" % (c["idx"], others)


@pytest.mark.gpu
def test_odf_e_window_with_false_positives_equals_oracle():
    _gpu_equals_oracle("a-odf-e-greek4")


# ------------------------------------------------------------------ (b) PDF R4: the cut inside a character
def test_pdf_r4_cut_window_has_two_runs_of_64_on_the_oracle():
    """"€" * 10 is 30 bytes: an 11th € or ₭ leaves E2 82 before the cut, so both verify, whatever follows."""
    c = CASES["b-pdf-r4-cut"]
    assert c["idx"] == P10 * 256 + 64 and c["start"] == P10 * 256 - (1 << 15)
    _, want = expected("b-pdf-r4-cut")
    assert want == [P10 * 256 + k for k in list(range(64, 128)) + list(range(192, 256))], (len(want), want[:4])


@pytest.mark.gpu
def test_pdf_r4_cut_inside_a_character_equals_oracle():
    _gpu_equals_oracle("b-pdf-r4-cut")


# ------------------------------------------------------------------ (c) Office: mixed UTF-16 units
def test_office_mixed_keyspace_has_one_hit_on_the_oracle():
    assert CASES["c-office-mixed"]["idx"] == 574
    assert [len(ch.encode("utf-16-le")) for ch in OFFICE] == [2, 2, 2, 4, 4, 2]
    assert expected("c-office-mixed")[1] == [574]


@pytest.mark.gpu
def test_office_mixed_units_whole_keyspace_equals_oracle():
    _gpu_equals_oracle("c-office-mixed")


# ------------------------------------------------------------------ (d) PDF R5: one document per edge
@pytest.mark.parametrize("name", D_CASES)
def test_pdf_r5_edge_is_the_only_hit_on_the_oracle(name):
    assert expected(name)[1] == [CASES[name]["idx"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", D_CASES)
def test_pdf_r5_planted_edge_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ (e) PDF R2 and R6
@pytest.mark.parametrize("name", E_CASES)
def test_mixed_width_window_has_one_hit_on_the_oracle(name):
    assert expected(name)[1] == [CASES[name]["idx"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", E_CASES)
def test_mixed_width_window_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ windows that do not fit 64 bits
def test_binding_refuses_windows_over_64_bits_before_the_library():
    """ctypes would wrap them; the guard stands in front of the call, so no context (and no GPU) is needed to see it."""
    from dprf_amd import _lib
    ctx = _lib.Context.__new__(_lib.Context)              # no handle: the library must not be reached
    for fn, cs in ((ctx.search_symbols, GREEK), (ctx.search_range, "abcdefghijklmnopqrstuvwx")):
        for start, count in ((0, 24 ** 14), (0, 1 << 64), (1 << 63, 1 << 63), ((1 << 64) - 1, 1), (-1, 4), (0, -1)):
            with pytest.raises(_lib.DprfError) as ei:
                fn(cs, 14, start, count)
            assert ei.value.code == _lib.E_INVALID, (start, count)


@pytest.mark.gpu
def test_window_over_64_bits_raises():
    """24^14 > 2^64: once wrapped to 24^14 mod 2^64 the count passed the library's keyspace check and a prefix was
    searched and reported empty."""
    from dprf_amd import _lib
    stream, _ = expected("d-table-1")
    with _lib.Context(_fields(stream), device=0) as ctx:
        assert 24 ** 14 > 1 << 64
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_symbols(GREEK, 14, 0, 24 ** 14)
        assert ei.value.code == _lib.E_INVALID
        with pytest.raises(_lib.DprfError) as ei:
            ctx.search_range("abcdefghijklmnopqrstuvwx", 14, 0, 24 ** 14)
        assert ei.value.code == _lib.E_INVALID
        hits, _, _ = ctx.search_symbols("é", 32, 0, 1)      # the context still serves
        assert hits == [0]
