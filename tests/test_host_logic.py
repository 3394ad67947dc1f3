"""Host-side logic of the brute_force counterpart (no GPU): field split, tag regex, argument checks,
enumeration order, parsers."""
import itertools
import json
import os

import pytest

from dprf_amd import brute_force as bf
from dprf_amd.parsers import odt2hashes


def test_parse_verification_data_matches_reference_shapes(streams):
    for name, d in streams.items():
        f = bf.parse_verification_data(d["stream"])
        assert f[0] in ("office", "odt", "pdf")
        assert len(f) == {"office": 8, "odt": 7, "pdf": 12}[f[0]]


@pytest.mark.parametrize("bad", ["x:$office$*2007*20", "garbage", "x:$zip$*1*2*3", "x:$pdf$*1*2"])
def test_unsupported_stream_exits_1(bad):
    with pytest.raises(SystemExit) as ei:
        bf.parse_verification_data(bad)
    assert ei.value.code == 1


def test_init_argument_checks():
    with pytest.raises(ValueError):
        bf.init("x:$pdf$*", 0, None)
    with pytest.raises(ValueError):
        bf.init("x:$pdf$*", 3, ["a"])


@pytest.mark.parametrize("cs,n", [("abc", 3), (bf.LOWERCASE, 2), (bf.ALNUM, 2), ("z", 4)])
def test_index_order_is_itertools_product(cs, n):
    ref = ["".join(t) for t in itertools.product(cs, repeat=n)]
    assert [bf._index_to_password(i, cs, n) for i in range(len(ref))] == ref


def test_odt_parser_matches_golden(streams):
    path = os.path.join(REF_FILES, "odt", "password.odt")
    assert odt2hashes.get_hashes(path, True) == streams["odt_testdoc_e"]["stream"]
    assert odt2hashes.get_hashes(path, False) == streams["odt_testdoc_std"]["stream"]


def _fastdiv(n, d):
    """The u32 division the kernels use (dev_crypto.h fastdiv) with the host magic (dprf_doc.cpp)."""
    if d <= 1:
        return n
    l = (d - 1).bit_length()
    m = ((1 << 32) * ((1 << l) - d)) // d + 1
    t = (n * m) >> 32
    return (t + ((n - t) >> 1)) >> (l - 1)


def test_fastdiv_magic_exact():
    import random
    rng = random.Random(7)
    for d in list(range(1, 257)):
        for n in [0, 1, d - 1, d, d + 1, 2 ** 32 - 1, 2 ** 31, 2 ** 32 - d] + [rng.getrandbits(32) for _ in range(200)]:
            n &= 0xffffffff
            assert _fastdiv(n, d) == n // d, (n, d)


# the reference's test documents, stored as fixtures (tests/golden/ref_docs/README.md)
REF_FILES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_docs")


@pytest.mark.parametrize("name,rel,kind", [("pdf_testdoc_r2", "pdf/password_1.3_v1_r2.pdf", "pdf"),
                                           ("pdf_testdoc_r4", "pdf/password_1.7_v4_r4.pdf", "pdf"),
                                           ("office_testdoc", "ms/password.docx", "office")])
def test_parsers_reproduce_reference_streams(streams, name, rel, kind):
    """The Python-3 parsers print the reference parsers' Python-2 output (PDF streams: SURVEY.md Appendix A,
    including the escaped ')' in the R2 file's U that Python 3 truncates; Office: office2john.py's output)."""
    path = os.path.join(REF_FILES, rel)
    from dprf_amd.parsers import office2john, pdf2john
    mod = pdf2john if kind == "pdf" else office2john
    assert mod.get_hash(path) == streams[name]["stream"]


def test_get_verification_data_uses_engine_parser_modes(streams, capsys):
    """brute_force.get_verification_data: doc type 2 uses the -e stream (brute_force.py:239)."""
    assert bf.get_verification_data("2", REF_FILES + "/odt/password.odt") == streams["odt_testdoc_e"]["stream"]
    assert bf.get_verification_data("3", REF_FILES + "/pdf/password_1.7_v4_r4.pdf") == streams["pdf_testdoc_r4"]["stream"]
    assert bf.get_verification_data("1", REF_FILES + "/ms/password.docx") == streams["office_testdoc"]["stream"]


class _OracleCtx:
    """Stand-in for _lib.Context backed by the oracle (test infrastructure), recording the ranges asked."""

    def __init__(self, oracle, stream, log, fail_at=None):
        self.c = oracle.Ctx(stream)
        self.log = log
        self.fail_at = fail_at

    def verify_list(self, passwords, stop_on_first=False, cap=1 << 16):
        h = [i for i, p in enumerate(passwords) if self.c.verify(p.encode())]
        return h[:cap], len(h), {"candidates": len(passwords), "wall_ms": 1.0}

    def search_range(self, charset, pwlen, start, count, stop_on_first=False, cap=1 << 16):
        if self.fail_at is not None and start >= self.fail_at:
            raise KeyboardInterrupt
        self.log.append((start, count))
        h, n = self.c.search_range(charset, pwlen, start, count)
        return h[:cap], n, {"candidates": count, "wall_ms": 1.0}   # absolute keyspace indices, like _lib.Context

    def close(self):
        pass


def test_range_checkpoint_resumes_where_it_stopped(streams, oracle, tmp_path, monkeypatch):
    d = streams["pdf_synth_r5_cat"]
    fields = bf.parse_verification_data(d["stream"])
    monkeypatch.setattr(bf, "FIRST_ROUND", 1000)
    monkeypatch.setattr(bf, "ROUND_SECONDS", 0.0)
    cp = str(tmp_path / "cursor.json")
    want = bf.LOWERCASE.index("c") * 676 + bf.LOWERCASE.index("a") * 26 + bf.LOWERCASE.index("t")
    log1 = []
    monkeypatch.setattr(bf, "_context", lambda inp, dev: _OracleCtx(oracle, d["stream"], log1, fail_at=1000))
    with pytest.raises(KeyboardInterrupt):
        bf.init_rangebased_brute_force(fields, 3, checkpoint=cp)
    assert log1 == [(0, 1000)]
    assert json.load(open(cp))["next_index"] == 1000
    log2 = []
    monkeypatch.setattr(bf, "_context", lambda inp, dev: _OracleCtx(oracle, d["stream"], log2))
    assert bf.init_rangebased_brute_force(fields, 3, checkpoint=cp) == (1, "cat")
    assert log2[0] == (1000, 1000) and log2[-1][0] <= want < log2[-1][0] + log2[-1][1]
    # finished searches answer from the checkpoint; a different search refuses it
    assert bf.init_rangebased_brute_force(fields, 3, checkpoint=cp) == (1, "cat")
    with pytest.raises(ValueError):
        bf.init_rangebased_brute_force(fields, 4, checkpoint=cp)


def test_range_mode_prints_progress_every_round(streams, oracle, monkeypatch, capsys):
    """The reference prints running time, candidates tried, speed and queue size every 1000 candidates
    (brute_force.py:149-157); range mode here prints the same three lines after every round,
    and the answer is the same as without them."""
    d = streams["pdf_synth_r5_cat"]
    fields = bf.parse_verification_data(d["stream"])
    monkeypatch.setattr(bf, "FIRST_ROUND", 1000)
    monkeypatch.setattr(bf, "ROUND_SECONDS", 0.0)
    log = []
    monkeypatch.setattr(bf, "_context", lambda inp, dev: _OracleCtx(oracle, d["stream"], log))
    capsys.readouterr()
    assert bf.init_rangebased_brute_force(fields, 3) == (1, "cat")
    out = capsys.readouterr().out.splitlines()
    running = [ln for ln in out if ln.startswith("Running time: ")]
    speed = [ln for ln in out if ln.startswith("Speed: ") and ln.endswith(" H/sec")]
    queue = [ln for ln in out if ln.startswith("Queue size: ")]
    assert len(running) == len(speed) == len(queue) == len(log) >= 2
    tried = [int(ln.split("tried since: ")[1].split()[0]) for ln in running]
    assert tried == [1 + sum(c for _, c in log[:k + 1]) for k in range(len(log))]   # + the "_dummy" candidate
    assert int(queue[-1].split(": ")[1]) == 0 and int(queue[0].split(": ")[1]) == 26 ** 3 - 1000


# ---- range mode over a charset with multi-byte characters (VERDICT r5 Weak #2 / Next #1) ----------------------------
# The library's range symbols are bytes; brute_force sizes and decodes the keyspace over characters.  A charset with a
# character of several UTF-8 bytes is therefore spelled on the host by characters (payload.spell_utf8) and verified in
# list mode, so the keyspace, the hit index, the printed password and the checkpoint all count characters.

def test_check_charset_rules():
    from dprf_amd import _lib
    assert bf.check_charset(bf.LOWERCASE) is True and bf.check_charset(bf.ALNUM) is True
    assert bf.check_charset("aé") is False and bf.check_charset("\U0001F600") is False
    for bad in ("", "aba", "a\0", "éé", b"abc", "a\ud800"):
        with pytest.raises(_lib.DprfError) as ei:
            bf.check_charset(bad)
        assert ei.value.code == _lib.E_CHARSET, bad


def test_spell_utf8_parallel_equals_one_thread():
    from dprf_amd.payload import spell_utf8, spell_utf8_parallel
    cs = "abcäöü€\U0001F600"
    for start, count in ((0, 5000), (123457, 40001), (8 ** 5 - 10, 10)):
        b1, o1 = spell_utf8(cs, 6, start, count)
        b2, o2 = spell_utf8_parallel(cs, 6, start, count, workers=4, part=4096)
        assert b1 == b2 and (o1 == o2).all(), (start, count)


@pytest.mark.parametrize("cs,n", [("aé", 3), ("x€y\U0001F600", 2), ("ab", 4), ("é", 2)])
def test_spell_utf8_is_itertools_product(cs, n):
    from dprf_amd.payload import spell_utf8
    ref = ["".join(t).encode("utf-8") for t in itertools.product(cs, repeat=n)]
    for start, count in ((0, len(ref)), (1, len(ref) - 2), (len(ref) - 1, 1)):
        if count <= 0:
            continue
        blob, offs = spell_utf8(cs, n, start, count)
        got = [blob[int(offs[k]):int(offs[k + 1])] for k in range(count)]
        assert got == ref[start:start + count], (cs, n, start)


def test_search_range_refuses_a_multibyte_str_charset():
    """_lib.Context.search_range raises before any library call (self is never touched)."""
    from dprf_amd import _lib
    with pytest.raises(_lib.DprfError) as ei:
        _lib.Context.search_range(object(), "aé", 3, 0, 8)
    assert ei.value.code == _lib.E_CHARSET


class _OracleBlobCtx(_OracleCtx):
    """_OracleCtx plus verify_blob (the list form the host-spelled rounds use), recording the windows asked."""

    def verify_blob(self, blob, offsets, stop_on_first=False, cap=1 << 16):
        words = [bytes(blob[int(offsets[k]):int(offsets[k + 1])]) for k in range(len(offsets) - 1)]
        self.log.append(("blob", len(words)))
        h = [i for i, v in enumerate(self.c.verify_list(words)) if v == 1]
        return h[:cap], len(h), {"candidates": len(words), "wall_ms": 1.0}


def _planted_stream(kind, pw):
    import os
    import tempfile
    import docgen
    from dprf_amd.parsers import odt2hashes, office2john, pdf2john
    with tempfile.TemporaryDirectory() as t:
        if kind == "docx":
            docgen.write_docx(os.path.join(t, "d.docx"), pw, 0xC5)
            return office2john.get_hash(os.path.join(t, "d.docx"))
        if kind == "odt":
            docgen.write_odt(os.path.join(t, "d.odt"), pw, 0xC5)
            return odt2hashes.get_hashes(os.path.join(t, "d.odt"), True)
        docgen.write_pdf(os.path.join(t, "d.pdf"), pw, 0xC5, R=4, length=128)
        return pdf2john.get_hash(os.path.join(t, "d.pdf"))


@pytest.mark.parametrize("kind", ["pdf", "odt", "docx"])
def test_range_mode_finds_a_password_of_multibyte_characters(oracle, monkeypatch, tmp_path, kind):
    """init(stream, 3, None, charset="aé") on a document whose password is "aéa": the answer is that password, its
    index the character-level one, the checkpoint records it (oracle-backed stand-in for the library)."""
    stream = _planted_stream(kind, "aéa")
    fields = bf.parse_verification_data(stream)
    log = []
    monkeypatch.setattr(bf, "_context", lambda inp, dev: _OracleBlobCtx(oracle, stream, log))
    monkeypatch.setattr(bf, "WIDE_ROUND", 3)
    cp = str(tmp_path / "cursor.json")
    assert bf.init_rangebased_brute_force(fields, 3, charset="aé", checkpoint=cp) == (1, "aéa")
    assert all(e[0] == "blob" for e in log) and sum(e[1] for e in log) <= 8
    d = json.load(open(cp))
    assert d["found"] == "aéa" and d["charset"] == "aé"
    # the same search in the library's byte symbols would be {a, 0xC3, 0xA9}^3 -- a different keyspace
    assert bf._index_to_password(0b010, "aé", 3) == "aéa"


class _OracleSymbolCtx(_OracleBlobCtx):
    """... plus search_symbols (ABI 7: the device spells the window by character), restated with the oracle: the
    window spelled by payload.spell_utf8 and verified candidate by candidate.  too_long: answer E_PWLEN as the
    library does when a candidate could exceed a 64-byte slot."""

    def __init__(self, oracle, stream, log, too_long=False):
        super().__init__(oracle, stream, log)
        self.too_long = too_long

    def search_symbols(self, charset, pwlen, start, count, stop_on_first=False, cap=1 << 16):
        from dprf_amd import _lib
        from dprf_amd.payload import spell_utf8
        self.log.append(("symbols", count))
        if self.too_long:
            raise _lib.DprfError(_lib.E_PWLEN, "slot")
        blob, offs = spell_utf8(charset, pwlen, start, count)
        words = [bytes(blob[int(offs[k]):int(offs[k + 1])]) for k in range(count)]
        h = [start + i for i, v in enumerate(self.c.verify_list(words)) if v == 1]
        return h[:cap], len(h), {"candidates": count, "wall_ms": 1.0}


@pytest.mark.parametrize("too_long", [False, True])
def test_multibyte_rounds_spell_on_the_device_or_fall_back_to_the_host(oracle, monkeypatch, too_long):
    """search_round over a multi-byte charset asks the library to spell the window (search_symbols) and returns its
    keyspace index; when the library answers E_PWLEN (a candidate could exceed a list slot) the same round is spelled
    on the host and verified as a list, with the same answer."""
    stream = _planted_stream("pdf", "aéa")
    log = []
    ctx = _OracleSymbolCtx(oracle, stream, log, too_long=too_long)
    monkeypatch.setattr(bf, "WIDE_ROUND", 4)
    found, st = bf.search_round(ctx, "aé", 3, 0, 8)
    assert found == 0b010 and bf._index_to_password(found, "aé", 3) == "aéa"
    assert log[0] == ("symbols", 8)
    if too_long:
        assert [e[0] for e in log[1:]] == ["blob"] and st["candidates"] == 4     # stop_on_first: rounds of 4
    else:
        assert len(log) == 1 and st["candidates"] == 8


def test_range_mode_rejects_a_bad_charset_before_device_work(monkeypatch):
    from dprf_amd import _lib

    def no_device(*a):
        raise AssertionError("a context was created")
    monkeypatch.setattr(bf, "_context", no_device)
    fields = ["pdf"] + ["1"] * 11
    for bad in ("aa", "", "a\0b"):
        with pytest.raises(_lib.DprfError) as ei:
            bf.init_rangebased_brute_force(fields, 2, charset=bad)
        assert ei.value.code == _lib.E_CHARSET
