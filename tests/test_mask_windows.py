"""Device-spelled mask windows (dprf_search_mask, k_spell_mask + the list kernels) against the oracle: the hit set of a
whole window equals the set pyoracle finds over the same window spelled by this file's own speller (divmod digits over
the positions' lists, "".join(...).encode(); the oracle does its own UTF-16LE conversion and truncation), on one, two
and four device lanes, with stop_on_first returning the oracle's lowest.  The windows are the smallest at which the
mixed-radix spelling can go wrong:

  (a) ODF `-e` (2-byte check): false positives besides the planted password, so windows with several hits
  (b) PDF R4: the 32-byte truncation falls inside a 3-byte character behind ten literals
  (c) Office: BMP and surrogate-pair symbols at different positions, the whole keyspace
  (d) PDF R5 (one SHA-256 per candidate): one document per edge of the spelling
  (e) PDF R2 and R6: mixed-width masks, windows whose start is no multiple of 64
  (f) a uniform mask against range mode (a self-comparison, beside the oracle cases)
  (g) the library's refusals, after each of which the context still serves
  (h) the CLI end to end, with a checkpoint

Every oracle case has a CPU test of its preconditions on the oracle alone, so the GPU comparison cannot pass
vacuously.  The oracle's set is computed once per case and shared."""
import contextlib
import functools
import io
import json
import os
import tempfile

import pytest

SEED = 0x5E1
ORACLE_THREADS = 16
DEVICE_LISTS = ([0], [0, 0], [0, 0, 0, 0])

LOWER = "abcdefghijklmnopqrstuvwxyz"
UPPER = LOWER.upper()
DIGITS = "0123456789"
GREEK = "αβγδεζηθικλμνξοπρστυφχψω"                       # 24 two-byte symbols


def T(k, n=256):
    """Table k of n distinct characters from U+0100 + 256 k: two UTF-8 bytes below U+0800, three from there."""
    return "".join(chr(0x100 + 256 * k + j) for j in range(n))


def space(pos):
    n = 1
    for p in pos:
        n *= len(p)
    return n


def word(i, pos):
    """itertools.product order over the positions: the last position varies fastest."""
    out = []
    for p in reversed(pos):
        i, r = divmod(i, len(p))
        out.append(p[r])
    return "".join(reversed(out))


def index_of(pw, pos):
    assert len(pw) == len(pos)
    i = 0
    for p, ch in zip(pos, pw):
        i = i * len(p) + p.index(ch)
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


R2, R4 = {"R": 2, "length": 40}, {"R": 4, "length": 128}
R5, R6 = {"R": 5, "length": 256}, {"R": 6, "length": 256}

ODF = [LOWER, DIGITS, "αβγδ", LOWER, "-", UPPER, "€é"]                           # radices 26 10 4 26 1 26 2
ODF_PW = "q7γm-Z€"
ODF_ALL = [86251, 122547, 148787, 243380, 470715, 472610, 535769, 639233, 672460, 686456, 700646, 906514, 1113824,
           1139271, 1166776, 1311594, 1314168]                                   # the oracle over the whole keyspace
CUT = ["€"] * 10 + ["a€é₭", "ab", "ab", "ab"]                                    # € = E2 82 AC, ₭ = E2 82 AD
OFFICE = ["a€", "é\U0001D11E", "P", DIGITS, "\U00020000b"]
OFFICE_PW = "€\U0001D11EP7\U00020000"
MIX = ["aé€", "-", DIGITS, "\U0001D11Eb", LOWER, "xy"]                           # keyspace 3120, widths 1-4
RIPPLE = ["xy", "a€", "-", T(0, 255), T(1), "pq\U0001D11E"]                      # radices 2 | 2 1 255 256 3
WIDE = [LOWER, LOWER, DIGITS, "a€", "-", LOWER, "éb\U0001D11E", DIGITS, LOWER, LOWER, DIGITS]   # 7.1e10 > 2^33
FILL = ["αβ", "γδ"] * 16                                                         # 32 x 2 bytes: the slot is full
CAP = [T(k) for k in range(8)]                                                   # 8 x 256: the pool at its cap
MIX_E = ["aé€", DIGITS, "\U0001D11Eb", LOWER, "-", "xyz", "€é"]                  # keyspace 9360


def _case(kind, kw, pos, idx, start, count):
    return {"kind": kind, "kw": kw, "pos": pos, "idx": idx, "start": start, "count": count}


def _r5(pos, idx, start, count):
    return _case("pdf", R5, pos, idx, start, count)


RIPPLE_START = index_of("x€-" + T(0, 255)[254] + T(1)[255] + "\U0001D11E", RIPPLE)   # the maximum digit below the first
CAP_IDX = index_of("".join(T(k)[(255, 0, 17, 255, 254, 1, 255, 255)[k]] for k in range(8)), CAP)

CASES = {
    "a-odf-e-three-false-positives": _case("odt_e", {}, ODF, 672460, 671999, 1 << 15),
    "a-odf-e-planted": _case("odt_e", {}, ODF, index_of(ODF_PW, ODF), 894169, 1 << 15),
    "b-pdf-r4-cut": _case("pdf", R4, CUT, index_of("€" * 11 + "aaa", CUT), 0, 32),
    "c-office-mixed": _case("docx", {}, OFFICE, index_of(OFFICE_PW, OFFICE), 0, space(OFFICE)),
    "e-pdf-r2": _case("pdf", R2, MIX_E, 7777, 5037, 1 << 12),
    "e-pdf-r6": _case("pdf", R6, MIX_E, 9000, space(MIX_E) - (1 << 12) - 3, 1 << 12),
    # (d): (positions, planted index, window start, window count <= 1024)
    "d-offset-0": _r5(MIX, 1000, 1000, 1000),
    "d-offset-255": _r5(MIX, 1255, 1000, 1000),
    "d-offset-256": _r5(MIX, 1256, 1000, 1000),
    "d-offset-count-1": _r5(MIX, 1999, 1000, 1000),
    "d-carry-radices-2-1-255-256-3": _r5(RIPPLE, RIPPLE_START + 1, RIPPLE_START, 600),
    "d-keyspace-last": _r5(MIX, space(MIX) - 1, space(MIX) - 777, 777),
    "d-literal-first": _r5(["€", DIGITS, LOWER], 259, 0, 260),
    "d-literal-middle": _r5([DIGITS, "€", LOWER], 137, 0, 260),
    "d-literal-last": _r5([DIGITS, LOWER, "€"], 26, 0, 260),
    "d-all-literal": _r5(list("Inv-€"), 0, 0, 1),
    "d-radix-256-digit-255": _r5(["xy", T(2), "-"], 256 + 255, 0, 512),
    "d-radix-255-digit-254": _r5(["xy", T(2, 255), "-"], 255 + 254, 0, 510),
    "d-slot-filled-32x2": _r5(FILL, 0xDEADBEEF, 0xDEADBEEF - 500, 1000),
    "d-across-2^32": _r5(WIDE, (1 << 32) + 5, (1 << 32) - 100, 1000),
    "d-past-2^32": _r5(WIDE, (1 << 32) + 98765, (1 << 32) + 98765 - 321, 1024),
    "d-pool-at-cap-8x256": _r5(CAP, CAP_IDX, CAP_IDX - 300, 1000),
    # (g): a keyspace of 24^14 > 2^64 whose window [0, 1000) is searched
    "g-keyspace-over-2^64": _r5([GREEK] * 14, 777, 0, 1000),
}
A_CASES = [k for k in CASES if k.startswith("a-")]
D_CASES = [k for k in CASES if k.startswith("d-")]
E_CASES = [k for k in CASES if k.startswith("e-")]


def _password(name):
    return ODF_PW if name in A_CASES else word(CASES[name]["idx"], CASES[name]["pos"])


@functools.lru_cache(maxsize=None)
def _stream_of(kind, kw, pw):
    return _stream(kind, dict(kw), pw)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(stream, the oracle's sorted hit indices of the case's window): once per case, for every test that needs it."""
    import pyoracle
    c = CASES[name]
    stream = _stream_of(c["kind"], tuple(sorted(c["kw"].items())), _password(name))
    window = [word(i, c["pos"]).encode() for i in range(c["start"], c["start"] + c["count"])]
    verdicts = pyoracle.Ctx(stream).verify_list(window, nthreads=ORACLE_THREADS)
    return stream, [c["start"] + k for k, v in enumerate(verdicts) if v]


def _gpu_equals_oracle(name):
    from dprf_amd import _lib
    c = CASES[name]
    stream, want = expected(name)
    assert want, name
    for devs in DEVICE_LISTS:
        with _lib.Context(_fields(stream), devices=devs) as ctx:
            hits, nh, st = ctx.search_mask(c["pos"], c["start"], c["count"])
            assert hits == want and nh == len(want), (name, devs, hits[:8], want[:8], nh, len(want))
            assert st["candidates"] == c["count"], (name, devs, st)
            first, _, _ = ctx.search_mask(c["pos"], c["start"], c["count"], stop_on_first=True, cap=1)
            assert first == want[:1], (name, devs, first, want[:1])


def test_cases_lie_inside_their_keyspaces():
    for name, c in CASES.items():
        assert all(len(set(p)) == len(p) and 1 <= len(p) <= 256 for p in c["pos"]) and len(c["pos"]) <= 32, name
        assert 0 <= c["start"] <= c["idx"] < c["start"] + c["count"] <= space(c["pos"]), name
        assert c["count"] <= (1024 if name in D_CASES else 1 << 15), name
    assert [len(p) for p in ODF] == [26, 10, 4, 26, 1, 26, 2] and space(ODF) == 1406080
    assert index_of(ODF_PW, ODF) == 906514 and 671999 % 64 and 894169 % 64
    for name in E_CASES:
        assert CASES[name]["start"] % 64 and CASES[name]["count"] == 1 << 12, name
    assert [CASES["d-offset-" + k]["idx"] - 1000 for k in ("0", "255", "256", "count-1")] == [0, 255, 256, 999]
    assert [len(p) for p in RIPPLE[1:]] == [2, 1, 255, 256, 3]
    assert [p.index(ch) for p, ch in zip(RIPPLE, word(RIPPLE_START, RIPPLE))] == [0, 1, 0, 254, 255, 2]
    assert [p.index(ch) for p, ch in zip(RIPPLE, word(RIPPLE_START + 1, RIPPLE))] == [1, 0, 0, 0, 0, 0]
    assert len(word(0, FILL).encode()) == 64 and len(FILL) == 32
    assert sum(len(p) for p in CAP) == 2048 and len(set("".join(CAP))) == 2048
    assert space(WIDE) > 1 << 33 and CASES["d-past-2^32"]["start"] > 1 << 32
    assert T(2).index(word(CASES["d-radix-256-digit-255"]["idx"], CASES["d-radix-256-digit-255"]["pos"])[1]) == 255
    assert T(2).index(word(CASES["d-radix-255-digit-254"]["idx"], CASES["d-radix-255-digit-254"]["pos"])[1]) == 254
    assert all(len(p) == 1 for p in CASES["d-all-literal"]["pos"]) and 24 ** 14 > 1 << 64


# ------------------------------------------------------------------ (a) ODF -e: false positives
def test_odf_e_windows_on_the_oracle():
    assert expected("a-odf-e-three-false-positives")[1] == [672460, 686456, 700646]
    assert expected("a-odf-e-planted")[1] == [906514]
    assert [h for h in ODF_ALL if 671999 <= h < 671999 + (1 << 15)] == [672460, 686456, 700646]
    assert [h for h in ODF_ALL if 894169 <= h < 894169 + (1 << 15)] == [906514]


@pytest.mark.gpu
@pytest.mark.parametrize("name", A_CASES)
def test_odf_e_window_equals_oracle(name):
    _gpu_equals_oracle(name)


# ------------------------------------------------------------------ (b) PDF R4: the cut inside a character
def test_pdf_r4_cut_has_sixteen_hits_on_the_oracle():
    """Ten literal € are 30 bytes: an 11th € or ₭ leaves E2 82 before the cut, so both verify, whatever follows."""
    assert CASES["b-pdf-r4-cut"]["idx"] == 8 and space(CUT) == 32
    assert expected("b-pdf-r4-cut")[1] == list(range(8, 16)) + list(range(24, 32))


@pytest.mark.gpu
def test_pdf_r4_cut_inside_a_character_equals_oracle():
    _gpu_equals_oracle("b-pdf-r4-cut")


# ------------------------------------------------------------------ (c) Office: surrogate pairs
def test_office_keyspace_has_one_hit_on_the_oracle():
    assert [len(ch.encode("utf-16-le")) for ch in OFFICE_PW] == [2, 4, 2, 2, 4] and space(OFFICE) == 80
    assert expected("c-office-mixed")[1] == [CASES["c-office-mixed"]["idx"]]


@pytest.mark.gpu
def test_office_whole_keyspace_equals_oracle():
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


# ------------------------------------------------------------------ (f) a uniform mask is range mode
@pytest.mark.gpu
def test_uniform_mask_equals_range_mode():
    from dprf_amd import _lib
    idx, start, count = 7654321, 7654321 - 40000, 1 << 16
    stream = _stream_of("pdf", tuple(sorted(R5.items())), word(idx, [LOWER] * 5))
    for devs in DEVICE_LISTS:
        with _lib.Context(_fields(stream), devices=devs) as ctx:
            a = ctx.search_mask([LOWER] * 5, start, count)
            b = ctx.search_range(LOWER, 5, start, count)
            assert a[0] == b[0] == [idx] and a[1] == b[1] == 1, (devs, a[:2], b[:2])
            assert a[2]["candidates"] == b[2]["candidates"] == count
            a = ctx.search_mask([LOWER] * 5, start, count, stop_on_first=True, cap=1)
            b = ctx.search_range(LOWER, 5, start, count, stop_on_first=True, cap=1)
            assert a[0] == b[0] == [idx]


# ------------------------------------------------------------------ (g) refusals
def test_keyspace_over_64_bits_window_has_one_hit_on_the_oracle():
    assert expected("g-keyspace-over-2^64")[1] == [777]


def _refused(ctx, code, pos, start, count, serve):
    from dprf_amd import _lib
    with pytest.raises(_lib.DprfError) as ei:
        ctx.search_mask(pos, start, count)
    assert ei.value.code == code, (ei.value, [len(p) for p in pos], start, count)
    assert ctx.last_call_devices() == []                               # a refused call leaves no record
    assert serve() == [0]                                              # ... and the context still serves


@pytest.mark.gpu
def test_refusals_and_a_keyspace_over_64_bits():
    from dprf_amd import _lib
    stream, want = expected("g-keyspace-over-2^64")
    with _lib.Context(_fields(stream), device=0) as ctx:               # PDF R5: candidates cut at 127 bytes
        pw = word(777, [GREEK] * 14)
        serve = lambda: ctx.search_mask(list(pw), 0, 1)[0]
        assert serve() == [0]
        bad = [
            (_lib.E_CHARSET, [LOWER, ""], 0, 1),                       # an empty position
            (_lib.E_CHARSET, [T(0) + "~", LOWER], 0, 1),               # 257 symbols
            (_lib.E_CHARSET, [LOWER, "aba"], 0, 1),                    # a repeated symbol within a position
            (_lib.E_CHARSET, CAP + ["-"], 0, 1),                       # 2049 symbols after merging
            (_lib.E_CHARSET, CAP + [T(8)], 0, 1),
            (_lib.E_CHARSET, [LOWER, b"a\0"], 0, 1),                   # NUL
            (_lib.E_PWLEN, [], 0, 0),                                  # no position
            (_lib.E_PWLEN, ["a"] * 33, 0, 1),                          # 33 positions
            (_lib.E_PWLEN, ["a€"] * 22, 0, 1),                         # up to 66 bytes
            (_lib.E_INVALID, [DIGITS, "€", LOWER], 0, 261),            # start + count over the keyspace
            (_lib.E_INVALID, [DIGITS, "€", LOWER], 260, 1),
            (_lib.E_INVALID, [DIGITS, "€", LOWER], 259, 2),
            (_lib.E_INVALID, [T(0, 255)] + CAP[1:], 255 * 256 ** 7 - 5, 6),   # just over a keyspace just under 2^64
            (_lib.E_INVALID, [GREEK] * 13, 24 ** 13 - 1, 2),
        ]
        for code, pos, start, count in bad:
            _refused(ctx, code, pos, start, count, serve)
        # accepted: the same lists merged (a ninth position of a list already in the pool), the keyspace's last index
        assert ctx.search_mask(CAP + [CAP[3]], 0, 10)[2]["candidates"] == 10
        assert ctx.search_mask([T(0, 255)] + CAP[1:], 255 * 256 ** 7 - 6, 6)[2]["candidates"] == 6
        assert ctx.search_mask(["a€"] * 21 + ["a"], 0, 10)[2]["candidates"] == 10    # 64 bytes fill the slot
        # 24^14 > 2^64: the window [0, 1000) is searched, and so is one that ends at 2^64 - 2
        hits, nh, st = ctx.search_mask([GREEK] * 14, 0, 1000)
        assert hits == want == [777] and nh == 1 and st["candidates"] == 1000
        hits, nh, st = ctx.search_mask([GREEK] * 14, (1 << 64) - 1001, 1000)
        assert hits == [] and st["candidates"] == 1000
        with pytest.raises(_lib.DprfError) as ei:                      # the binding's guard, before the library
            ctx.search_mask([GREEK] * 14, 0, 24 ** 14)
        assert ei.value.code == _lib.E_INVALID and serve() == [0]
    # PDF R2-R4 hash 32 bytes, so 66-byte candidates fit there; Office symbols must be characters
    r4, _ = expected("b-pdf-r4-cut")
    with _lib.Context(_fields(r4), device=0) as ctx:
        assert ctx.search_mask(["a€"] * 22, 0, 10)[2]["candidates"] == 10
    office, _ = expected("c-office-mixed")
    with _lib.Context(_fields(office), device=0) as ctx:
        serve = lambda: [h - CASES["c-office-mixed"]["idx"] for h in
                         ctx.search_mask(OFFICE, CASES["c-office-mixed"]["idx"], 1)[0]]
        _refused(ctx, _lib.E_CHARSET, ["ab", b"\xff"], 0, 1, serve)    # not UTF-8
        _refused(ctx, _lib.E_PWLEN, ["a\U0001D11E"] * 17, 0, 1, serve)    # 17 surrogate pairs: 68 bytes


# ------------------------------------------------------------------ (h) the CLI, with a checkpoint
@pytest.mark.gpu
def test_cli_mask_end_to_end_and_checkpoint_resume(tmp_path, capsys):
    import docgen
    from dprf_amd import brute_force, mask
    pdf = str(tmp_path / "invoice.pdf")
    password = "Inv-73€"
    docgen.write_pdf(pdf, password, SEED, **R5)
    argv = ["3", pdf, "--mask", "Inv-?d?d?1", "-1", "€é"]
    assert brute_force.main(argv) == (1, password)
    pos = mask.parse_mask("Inv-?d?d?1", ["€é"])
    idx = mask.index_of(pos, password)
    assert idx == 146 and mask.space(pos) == 200
    # a checkpoint written mid-search (the cursor after a round that ended at 100) resumes at its cursor ...
    cp = str(tmp_path / "cursor.json")
    key = brute_force.Checkpoint(cp, brute_force.parse_verification_data(brute_force.get_verification_data("3", pdf)),
                                 mask="Inv-?d?d?1", custom=("€é",))
    key.save(100)
    capsys.readouterr()
    assert brute_force.main(argv + ["--checkpoint", cp]) == (1, password)
    assert "Checkpoint: resuming at index 100" in capsys.readouterr().out
    assert json.load(open(cp))["found"] == password and json.load(open(cp))["next_index"] == 200
    # ... also when the cursor lies past the password: the indices below it are not searched again
    key.save(idx + 1)
    assert brute_force.main(argv + ["--checkpoint", cp]) == (0, brute_force.DEFAULT_PASSWORD)
    assert json.load(open(cp))["next_index"] == 200
    # another mask's checkpoint is refused
    with pytest.raises(ValueError):
        brute_force.main(["3", pdf, "--mask", "Inv-?d?d?d", "--checkpoint", cp])
