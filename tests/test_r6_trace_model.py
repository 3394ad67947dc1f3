"""The oracle's R6 trace export, the trace fixture and the planting helper, on the CPU.

  (a) pyoracle.pdf_r6_trace against Ctx.intermediates / work_counts (user) and owner_model.r6_hash (owner)
  (b) tests/golden/r6_traces.json: every entry recomputed and held to its stratum (tests/golden/make_r6_traces.py)
  (c) tests/r6_plant.py: a planted password verifies on the oracle and on the owner model, its neighbours do not
  (d) the every-length words of tests/test_r6_traces.py hash to distinct values
"""
import pytest

import owner_model as M
import r6_plant as P

O = P.O
FX = P.fixture()
ENTRIES = FX["entries"]


def _salts(fields):
    return bytes.fromhex(fields[9]), bytes.fromhex(fields[11])


# ---------------------------------------------------------------- (a) the export
@pytest.mark.parametrize("name", ["pdf_synth_r6_ox", "pdf_synth_r6_long"])
def test_trace_equals_the_verifier(streams, name):
    ctx = O.Ctx(streams[name]["stream"])
    U, _ = _salts(ctx.fields)
    pw = streams[name]["password"].encode()
    for w in (pw, pw[:-1], pw + b"x", b"", b"a" * 55, b"b" * 56, b"c" * 120, b"d" * 176):
        h, tr = O.pdf_r6_trace(w, U[32:40])
        assert h == ctx.intermediates(w)[:32]
        assert len(tr) == ctx.work_counts(w)["aes128_key_exp"] >= 64
        assert (h == U[:32]) == (ctx.verify(w) == 1) == (w == pw)
        n = len(tr)
        assert tr[0][0] == 32 and all(bs in (32, 48, 64) for bs, _ in tr)
        # the loop condition, restated: it ended after n rounds and at no earlier count
        assert tr[n - 1][1] <= n - 32 and all(tr[i - 1][1] > i - 32 for i in range(64, n))
    with pytest.raises(ValueError):
        O.pdf_r6_trace(b"e" * 177, U[32:40])
    assert ctx.verify(b"e" * 177) == -1


def test_trace_owner_form_equals_the_model():
    f = P.base_fields()
    U, Ob = _salts(f)
    assert M.owner_verifies(f, b"owner")
    for w in (b"owner", b"ownes", b"o", b"Q" * 64):
        h, tr = O.pdf_r6_trace(w, Ob[32:40], U[:48])
        assert h == M.r6_hash(w, Ob[32:40], U[:48])
        assert (h == Ob[:32]) == (w == b"owner") and len(tr) >= 64
    # the user form is the owner form with no udata, and the two differ
    assert O.pdf_r6_trace(b"owner", Ob[32:40])[0] != O.pdf_r6_trace(b"owner", Ob[32:40], U[:48])[0]


def test_trace_range_equals_single_traces():
    f = P.base_fields()
    U, Ob = _salts(f)
    cs, n = FX["charset"], FX["pwlen"]
    for salt, udata in ((U[32:40], b""), (Ob[32:40], U[:48])):
        rounds, final, edge = O.pdf_r6_trace_range(salt, cs, n, 4090, 12, udata, nthreads=5)
        for k in range(12):
            tr = O.pdf_r6_trace(O.index_to_password(4090 + k, cs, n), salt, udata)[1]
            assert (rounds[k], final[k]) == (len(tr), tr[-1][1])
            late = [i for i in range(64, len(tr)) if tr[i - 1][1] == i - 31]
            assert edge[k] == (late[0] if late else 0)


# ---------------------------------------------------------------- (b) the fixture
def test_fixture_names_its_scan():
    assert FX["charset"] == "abcdefghijklmnop" and FX["pwlen"] == 6
    assert FX["scan"]["user"][0] == 0 and FX["scan"]["user"][1] >= 1 << 17
    assert FX["max_rounds"]["user"] == max(e["rounds"] for e in ENTRIES if e["mode"] == "user") >= 104
    assert sorted(e["name"] for e in ENTRIES) == sorted(
        ["user-S1", "user-S2", "user-S3", "user-S4", "user-S5", "user-S6a", "user-S6b", "user-S6c", "owner-S1",
         "owner-S4"])
    from conftest import load_golden
    assert FX["stream"] == load_golden("docs.json")["pdf_r6.pdf"]["streams"]["std"]["stream"]


@pytest.mark.parametrize("e", ENTRIES, ids=[e["name"] for e in ENTRIES])
def test_fixture_entry_is_in_its_stratum(e):
    f = P.base_fields()
    pw = O.index_to_password(e["index"], FX["charset"], FX["pwlen"])
    assert pw == e["password"] and e["index"] < FX["scan"][e["mode"]][1]
    tr = P.trace(f, pw, e["mode"])[1]
    n, byte = len(tr), [b for _, b in tr]
    assert (n, byte[-1]) == (e["rounds"], e["final"])
    s = e["stratum"]
    if s == "S1":
        assert n == 64 and byte[63] == 32
    elif s == "S2":
        assert n == 64 and byte[63] == 0
    elif s == "S3":
        assert n == 65 and byte[63] == 33
    elif s == "S4":
        assert n > 64 and byte[-1] == n - 32
    elif s == "S5":
        assert any(byte[i - 1] == i - 31 for i in range(64, n))
        assert e["edge"] == min(i for i in range(64, n) if byte[i - 1] == i - 31)
    else:
        assert s in ("S6a", "S6b", "S6c") and n >= 96


def test_longest_traces_take_every_transition():
    f = P.base_fields()
    seen = set()
    for e in ENTRIES:
        if e["stratum"].startswith("S6"):
            bs = [b for b, _ in P.trace(f, e["password"], "user")[1]]
            seen |= set(zip(bs, bs[1:]))
    assert seen == {(a, b) for a in (32, 48, 64) for b in (32, 48, 64)}
    assert max(e["rounds"] for e in ENTRIES) >= 104


# ---------------------------------------------------------------- (c) planting
@pytest.mark.parametrize("L", [0, 1, 47, 48, 64, 65, 127, 128, 176])
def test_planted_user_password_verifies(L):
    base = P.base_fields()
    pw = P.length_word(L)
    ctx = O.Ctx(P.plant(base, pw, "user"))
    assert ctx.verify(pw) == 1
    assert ctx.verify(pw + b"x") == (0 if L < 176 else -1)
    if L:
        assert ctx.verify(pw[:-1] + bytes([pw[-1] ^ 1])) == 0 and ctx.verify(pw[:-1]) == 0
    assert ctx.verify(b"yak") == 0, "the base stream's own password no longer verifies"
    assert O.Ctx(base).verify(b"yak") == 1
    # only U[0:32] changed
    planted = P.plant(base, pw, "user")
    assert [a == b for a, b in zip(base, planted)].count(False) == 1 and planted[9][64:] == base[9][64:]


@pytest.mark.parametrize("L", [1, 48, 64])
def test_planted_owner_password_verifies_on_the_model(L):
    base = P.base_fields()
    pw = P.length_word(L)
    planted = P.plant(base, pw, "owner")
    assert M.owner_verifies(planted, pw) and not M.owner_verifies(planted, pw[:-1] + bytes([pw[-1] ^ 1]))
    assert planted[9] == base[9] and planted[11][64:] == base[11][64:]
    assert O.Ctx(planted).verify(b"yak") == 1, "the user password is untouched"


def test_planted_strata_verify():
    base = P.base_fields()
    for e in ENTRIES:
        if e["mode"] == "user":
            assert O.Ctx(P.plant(base, e["password"], "user")).verify(e["password"]) == 1


# ---------------------------------------------------------------- (d) the every-length words
def test_length_words_are_distinct():
    for which, lens in (("user", range(0, 177)), ("owner", range(1, 65))):
        words, hashes = P.length_words(which)
        assert [len(w) for w in words] == list(lens)
        assert all(33 <= b <= 126 for w in words for b in w)
        assert all(not b.startswith(a) for a, b in zip(words, words[1:]) if a)
        assert len(set(hashes)) == len(hashes)
    assert not set(P.length_words("user")[1]) & set(P.length_words("owner")[1])
