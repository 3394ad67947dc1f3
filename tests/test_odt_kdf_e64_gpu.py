"""The PBKDF2 SHA-1 loops of k_odt_kdf and k_odf_bf_kdf with their two-input XORs and adds in 8-byte encodings
(dev_crypto.h xor2_e64 / add2_e64 in sha1_compress_pre, sha1_h20_rounds, sha1_h20_word and the kernels' key XOR).  A
wrong bit anywhere in either compression of any of the 1,023 iterations changes the derived key, so a found password
pins the whole loop; the windows pin the shapes around it.

GPU: (a) k_odt_kdf<0>, range windows of 1, 63, 64, 65, 255, 256 and 257 candidates (partial wave, wave, wave + 1,
         block - 1, block, block + 1) holding the document's password at the first, a middle and the last index, the hit
         set equal to the oracle's over the whole window; and a 257-candidate window without the password: empty
     (b) k_odt_kdf<1>, list mode, on documents whose passwords have 1, 55, 56 and 64 bytes (the SHA-256 padding edges of
         the start key in front of the loop); k_odt_kdf<2>, one long-list candidate over 64 bytes
     (c) k_odf_bf_kdf<0>, 65 candidates of an ODF 1.0 / 1.1 stream at its real iteration count, against
         tests/odf_legacy_model.py
CPU: W[31] of the loop's message block.  A three-tap form rol1(W[28] ^ W[23]) ^ rol2(W[25] ^ W[20]) was proposed for
     it (one v_bitop3 and one rotate on the pre-rotation XORs of words 28 and 25).  It does not hold: W[17] and W[15] do
     not cancel -- rol2(W[25] ^ W[20]) is rol1(W[28]), so W[28] drops out, the form is rol1(W[23]) and lacks
     rol1(W[28] ^ W[17] ^ W[15]) -- and it is wrong for every one of 100 random messages.  The kernel keeps the four-tap
     word; the test pins that word against schedules whose digests are hashlib's, and the proposed form's failure, so
     that it is not tried again."""
import hashlib
import random
import struct
import tempfile
import zlib

import pytest

import test_odt_sha1_schedule as S

LOWER = "abcdefghijklmnopqrstuvwxyz"
STD = "odt_testdoc_std"
COUNTS = [1, 63, 64, 65, 255, 256, 257]


# ------------------------------------------------------------------ CPU
def test_w31_is_the_four_tap_word_and_has_no_three_tap_form():
    rng = random.Random(31)
    wrong = 0
    for _ in range(100):
        m = [rng.getrandbits(32) for _ in range(5)]
        w = S.schedule_plain(m)
        # the schedule is the one hashlib hashes with: SHA1(prefix | m) from the prefix's midstate
        prefix = bytes(rng.getrandbits(8) for _ in range(64))
        mid = S.compress(S.IV, S.schedule_plain_block(prefix))
        assert struct.pack(">5I", *S.compress(mid, w)) == hashlib.sha1(prefix + struct.pack(">5I", *m)).digest()
        assert w[31] == S.rol(w[28] ^ w[23] ^ w[17] ^ w[15], 1)
        assert S.schedule_table(m)[31] == w[31]
        three = S.rol(w[28] ^ w[23], 1) ^ S.rol(w[25] ^ w[20], 2)
        assert three == S.rol(w[23], 1) and three ^ w[31] == S.rol(w[28] ^ w[17] ^ w[15], 1)
        wrong += three != w[31]
    assert wrong == 100


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device: GPU tests need the MI355X box"
    return _lib


def _fields(stream):
    import contextlib
    import io
    from dprf_amd.brute_force import parse_verification_data
    with contextlib.redirect_stdout(io.StringIO()):
        return parse_verification_data(stream)


def _index(pw):
    idx = 0
    for ch in pw:
        idx = idx * len(LOWER) + LOWER.index(ch)
    return idx


@pytest.fixture(scope="module")
def around(oracle, streams):
    """(idx, the oracle's hits among the indices idx - 257 .. idx + 256 of the password's keyspace), computed once"""
    pw = streams[STD]["password"]
    idx = _index(pw)
    hits, n = oracle.Ctx(streams[STD]["stream"]).search_range(LOWER, len(pw), idx - 257, 514)
    assert n == len(hits) and idx in hits
    return idx, hits


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_range_windows_hold_the_password(dprf, streams, around, count):
    """(a) k_odt_kdf<0>"""
    idx, ohits = around
    pwlen = len(streams[STD]["password"])
    with dprf.Context(_fields(streams[STD]["stream"]), device=0) as ctx:
        for at in sorted({0, count // 2, count - 1}):
            start = idx - at
            want = [i for i in ohits if start <= i < start + count]
            assert idx in want
            hits, n, st = ctx.search_range(LOWER, pwlen, start, count)
            assert hits == want and n == len(want) and st["candidates"] == count, (count, at, hits)


@pytest.mark.gpu
def test_range_window_without_the_password_is_empty(dprf, streams, around):
    """(a) the 257 indices that end one short of the password"""
    idx, ohits = around
    start = idx - 257
    assert [i for i in ohits if start <= i < start + 257] == []
    with dprf.Context(_fields(streams[STD]["stream"]), device=0) as ctx:
        hits, n, st = ctx.search_range(LOWER, len(streams[STD]["password"]), start, 257)
        assert hits == [] and n == 0 and st["candidates"] == 257


def _planted(L):
    return "".join(chr(33 + (7 * k + 5 * L + k * k) % 90) for k in range(L))


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 55, 56, 64])
def test_list_mode_password_lengths(dprf, oracle, L):
    """(b) k_odt_kdf<1>: the password, one byte less, one byte more (at 64: another last byte) and a changed last byte"""
    import docgen
    from dprf_amd.parsers import odt2hashes
    pw = _planted(L)
    assert len(pw.encode()) == L
    with tempfile.TemporaryDirectory() as t:
        path = t + "/doc.odt"
        docgen.write_odt(path, pw, zlib.crc32(pw.encode()))
        stream = odt2hashes.get_hashes(path)
    shorter = pw[:-1] if L > 1 else "~"
    longer = pw + "x" if L < 64 else pw[:-1] + "~"
    words = [shorter, longer, pw, pw[:-1] + "}"]
    want = [i for i, v in enumerate(oracle.Ctx(stream).verify_list(words)) if v == 1]
    assert want == [2]
    with dprf.Context(_fields(stream), device=0) as ctx:
        assert ctx.kernel == "odf_aes256"
        hits, n, st = ctx.verify_list(words)
        assert hits == want and n == 1 and st["candidates"] == len(words)


@pytest.mark.gpu
def test_long_list_candidate(dprf, oracle, long_verdicts):
    """(b) k_odt_kdf<2> behind k_long_prehash: the one candidate over 64 bytes is the hit"""
    d = long_verdicts["odt_long_std_100"]
    pw = d["password"]
    assert len(pw.encode()) > 64
    words = ["wrong", pw]
    octx = oracle.Ctx(d["stream"])
    assert [octx.verify(w) for w in words] == [0, 1]
    with dprf.Context(_fields(d["stream"]), device=0) as ctx:
        hits, n, st = ctx.verify_list(words)
        assert hits == [1] and n == 1 and st["candidates"] == 2


@pytest.mark.gpu
def test_odf_legacy_range_of_65(dprf):
    """(c) k_odf_bf_kdf<0>: 65 candidates (a wave and one lane) at 1,024 iterations, the password in the second wave"""
    import odf_legacy_model as M
    cs, pwlen, start, count = "678Ux", 5, 1009, 65
    idx = start + 64
    pw = M.word(idx, cs, pwlen)
    s = M.make_stream(pw, 1024, seed=zlib.crc32(pw.encode()))
    want = [start + k for k in range(count) if M.verifies(s, M.word(start + k, cs, pwlen))]
    assert want == [idx]
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.kernel == "odf_bf_sha1"
        hits, n, st = ctx.search_range(cs, pwlen, start, count)
        assert hits == want and n == 1 and st["candidates"] == count
        assert ctx.search_range(cs, pwlen, start, count - 1)[0] == []
