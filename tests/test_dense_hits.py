"""Lists in which the password stands at many known positions: every lane, block, slot and seam verifies.

A candidate that does not verify is rejected by a right kernel and by almost any wrong one, so a list with one hit
checks one lane's computation.  dprf_verify_list takes the same candidate any number of times and counts every hit, so
a list holding the password at known positions must hit at exactly those.  Per list-mode family (the password from a
golden stream, an agile_model stream at spinCount 3, or a golden document's owner password):

  all     549 copies (two 256-lane blocks and a ragged tail): hits 0..548, n = 549; cap = 7 keeps the lowest seven
  mixed   1,500 candidates, the password where (k*k + 3*k) % 7 < 3, otherwise one of 64 decoys of ragged lengths;
          stop_on_first returns the first position
  lanes   the mixed list on devices [0, 0] and [0, 0, 0, 0]: the same hits, n exact -- no seam verifies twice or skips
  refill  (R6 user and owner) 150,000 candidates, decoys up to 64 bytes: more than 256 workgroups' slots at that
          column size (r6_capacity: 576 a workgroup), so slots are refilled from the persistent loop
  hybrid  a table of 300 copies of one word under ?w?d: hits 10 w + 7

The decoys and the password are verified on the CPU (the oracle, agile_model, owner_model) in tests not marked gpu.
"""
import contextlib
import functools
import io

import pytest

import agile_model as AM
import owner_model as OM
import r6_plant as P
from conftest import load_golden

O = P.O
gpu = pytest.mark.gpu

N_ALL, N_MIXED, N_REFILL = 549, 1500, 150000
DIGITS = "0123456789"


def is_pw(k):
    return (k * k + 3 * k) % 7 < 3


def decoys(lo, hi):
    """64 fixed words of printable ASCII, lengths spread over [lo, hi]."""
    return [bytes(33 + (5 * j + 3 * k + k * k) % 94 for k in range(lo + 37 * j % (hi - lo + 1)))
            for j in range(64)]


def mixed(pw, dec, n):
    return [pw if is_pw(k) else dec[(k * 29 + k // 64) % 64] for k in range(n)]


def _fields(stream):
    from dprf_amd.brute_force import parse_verification_data
    with contextlib.redirect_stdout(io.StringIO()):
        return parse_verification_data(stream)


def _golden_stream(name):
    return load_golden("streams.json")[name]


def _oracle_family(d, lo, hi):
    ctx = O.Ctx(d["stream"])
    return dict(fields=_fields(d["stream"]), pw=d["password"].encode(), mode="user", lens=(lo, hi),
                verifies=lambda w: ctx.verify(w) == 1)


def _agile(version, bits):
    pw = "Ux7-dense"
    s = AM.make_stream(pw, version, bits, 3, seed=0xDE45E + bits)
    return dict(fields=_fields(s), pw=pw.encode(), mode="user", lens=(1, 32),
                verifies=lambda w: AM.verifies(s, w.decode("ascii")))


def _owner(doc):
    s = load_golden("docs.json")[doc]["streams"]["std"]["stream"]
    f = O.split_stream(s)
    if f[2] == "6":
        U, Ob = bytes.fromhex(f[9]), bytes.fromhex(f[11])
        ver = lambda w: O.pdf_r6_trace(w, Ob[32:40], U[:48])[0] == Ob[:32]   # noqa: E731  (pinned on owner_model)
    else:
        ver = lambda w: OM.owner_verifies(s, w)                              # noqa: E731
    return dict(fields=_fields(s), pw=b"owner", mode="owner", lens=(1, 64), verifies=ver)


FAMILIES = {
    "office2007": lambda: _oracle_family(_golden_stream("office_synth_ok"), 1, 64),
    "agile_sha1": lambda: _agile("2010", 128),
    "agile_sha512": lambda: _agile("2013", 256),
    "odf_std": lambda: _oracle_family(_golden_stream("odt_synth_std_zq"), 1, 64),
    "odf_e": lambda: _oracle_family(_golden_stream("odt_synth_e_ab"), 1, 64),
    "pdf_r2": lambda: _oracle_family(_golden_stream("pdf_synth_r2_key"), 1, 64),
    "pdf_r3_40": lambda: _oracle_family(_golden_stream("pdf_synth_r3_l40_cab"), 1, 64),
    "pdf_r4": lambda: _oracle_family(_golden_stream("pdf_synth_r4_alnum"), 1, 64),
    "pdf_r5": lambda: _oracle_family(_golden_stream("pdf_synth_r5_cat"), 1, 64),
    "pdf_r6": lambda: _oracle_family(_golden_stream("pdf_synth_r6_ox"), 1, 64),
    "pdf_r4_owner": lambda: _owner("pdf_r4.pdf"),
    "pdf_r5_owner": lambda: _owner("pdf_r5.pdf"),
    "pdf_r6_owner": lambda: _owner("pdf_r6.pdf"),
    # the long-list path: a password over the 64-byte slot, decoys on both sides of it
    "odf_long": lambda: _oracle_family(load_golden("long_verdicts.json")["odt_long_std_100"], 1, 150),
    "pdf_r6_long": lambda: _oracle_family(load_golden("long_verdicts.json")["pdf_r6_long100"], 1, 150),
}
NAMES = list(FAMILIES)


@functools.lru_cache(maxsize=None)
def family(name):
    f = FAMILIES[name]()
    f["decoys"] = decoys(*f["lens"])
    return f


@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device: GPU tests need the MI355X box"
    return _lib


def _ctx(dprf, f, devices=None):
    if devices is None:
        return dprf.Context(f["fields"], device=0, pdf_password=f["mode"])
    return dprf.Context(f["fields"], devices=devices, pdf_password=f["mode"])


# ---------------------------------------------------------------- CPU: what the lists are made of
@pytest.mark.parametrize("name", NAMES)
def test_password_verifies_and_no_decoy_does(name):
    f = family(name)
    dec = f["decoys"]
    assert len(set(dec)) == 64 and f["pw"] not in dec
    lo, hi = f["lens"]
    assert lo == min(map(len, dec)) and max(map(len, dec)) <= hi and len(set(map(len, dec))) >= 32
    if name.endswith("_long"):
        assert len(f["pw"]) > 64 and sum(len(w) > 64 for w in dec) >= 16 and sum(len(w) <= 64 for w in dec) >= 16
    assert f["verifies"](f["pw"])
    assert [j for j, w in enumerate(dec) if f["verifies"](w)] == []


def test_mixed_pattern():
    pos = [k for k in range(N_MIXED) if is_pw(k)]
    assert pos[:4] == [0, 4, 7, 11] and len(pos) == 429           # k % 7 in (0, 4)
    words = mixed(b"pw", decoys(1, 64), N_MIXED)
    assert [k for k, w in enumerate(words) if w == b"pw"] == pos
    assert len(set(words)) == 65, "every decoy is used"
    # every lane of a wave holds the password somewhere, and so do both sides of every 256-candidate block edge
    assert {k % 64 for k in pos} == set(range(64))
    assert all(any(is_pw(k) for k in range(b - 4, b)) and any(is_pw(k) for k in range(b, b + 4))
               for b in range(256, N_MIXED, 256))


# ---------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("name", NAMES)
def test_all_copies_hit(dprf, name):
    f = family(name)
    with _ctx(dprf, f) as ctx:
        hits, n, st = ctx.verify_list([f["pw"]] * N_ALL)
        assert hits == list(range(N_ALL)) and n == N_ALL and st["candidates"] == N_ALL
        hits, n, _ = ctx.verify_list([f["pw"]] * N_ALL, cap=7)
        assert hits == list(range(7)) and n == N_ALL


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_mixed_list_hits_at_the_passwords_positions(dprf, name):
    f = family(name)
    words = mixed(f["pw"], f["decoys"], N_MIXED)
    want = [k for k in range(N_MIXED) if is_pw(k)]
    with _ctx(dprf, f) as ctx:
        hits, n, st = ctx.verify_list(words)
        assert hits == want and n == len(want) and st["candidates"] == N_MIXED
        assert ctx.verify_list(words, stop_on_first=True, cap=1)[0] == want[:1]
        # the first position is not always 0: drop the head of the list
        assert ctx.verify_list(words[1:], stop_on_first=True, cap=1)[0] == [want[1] - 1]


@gpu
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]], ids=["2lanes", "4lanes"])
@pytest.mark.parametrize("name", NAMES)
def test_mixed_list_on_several_lanes(dprf, name, devices):
    f = family(name)
    words = mixed(f["pw"], f["decoys"], N_MIXED)
    want = [k for k in range(N_MIXED) if is_pw(k)]
    with _ctx(dprf, f, devices) as ctx:
        hits, n, st = ctx.verify_list(words)
        assert hits == want and n == len(want) and st["candidates"] == N_MIXED
        assert [d["device"] for d in ctx.last_call_devices()] == devices


@gpu
@pytest.mark.parametrize("name", ["pdf_r6", "pdf_r6_owner"])
def test_r6_refill(dprf, name):
    import numpy as np
    f = family(name)
    assert f["lens"] == (1, 64)
    k = np.arange(N_REFILL, dtype=np.int64)
    pw_at = (k * k + 3 * k) % 7 < 3
    which = np.where(pw_at, 64, (k * 29 + k // 64) % 64)
    table = f["decoys"] + [f["pw"]]
    lens = np.array([len(w) for w in table], dtype=np.uint64)
    offs = np.zeros(N_REFILL + 1, dtype=np.uint64)
    np.cumsum(lens[which], out=offs[1:])
    blob = b"".join(table[j] for j in which.tolist())
    assert len(blob) == int(offs[-1])
    want = np.flatnonzero(pw_at)
    with _ctx(dprf, f) as ctx:
        hits, n, st = ctx.verify_blob(blob, offs, cap=N_REFILL)
        assert n == len(want) and st["candidates"] == N_REFILL
        assert np.array_equal(np.array(hits, dtype=np.int64), want)


@gpu
def test_hybrid_repeated_word(dprf):
    """300 copies of one word (two 256-word stagings) under ?w?d: the password is the word and a 7, on an R5 stream
    whose U[0:32] is SHA-256(password || U[32:40])."""
    f = O.split_stream(_golden_stream("pdf_synth_r5_cat")["stream"])
    U = bytes.fromhex(f[9])
    f[9] = O.sha256(b"sun7" + U[32:40]).hex() + f[9][64:]
    octx = O.Ctx(f)
    assert [d for d in DIGITS if octx.verify("sun" + d) == 1] == ["7"]
    want = [10 * w + 7 for w in range(300)]
    with dprf.Context(f, device=0) as ctx:
        ctx.set_words([b"sun"] * 300)
        hits, n, st = ctx.search_hybrid([DIGITS], 0, 0, 3000)
        assert hits == want and n == 300 and st["candidates"] == 3000
        assert ctx.search_hybrid([DIGITS], 0, 0, 3000, stop_on_first=True, cap=1)[0] == [7]
        assert ctx.search_hybrid([DIGITS], 0, 2555, 15)[0] == [2557, 2567]           # the seam of the two stagings
