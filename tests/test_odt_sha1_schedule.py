"""The SHA-1 message schedule of k_odt_kdf's PBKDF2 loop (dev_crypto.h sha1_compress_pre): every word t = 16..79 of a
20-byte message's block (W[0..4] the message, W[5] = 0x80000000, W[6..14] = 0, W[15] = 0x2A0) is computed by the
standard recurrence (form 1), its square (form 2) or its fourth power (form 4), over its non-zero inputs only.

CPU: the kernel's table, restated here word for word, gives the plain 80-word schedule and hashlib's digests, and costs
148 XOR/rotate instructions (550 per compression with the rounds).
GPU: the device finds exactly the oracle's hits in range, list and long-list mode (k_odt_kdf<0>, <1>, <2>); a wrong
schedule word in either compression of either PBKDF2 block changes the AES key, so a found password pins them all."""
import hashlib
import random
import struct

import pytest

M32 = 0xFFFFFFFF
PAD, BITS = 0x80000000, (64 + 20) * 8

# (t, form, non-zero inputs): form f reads W[t-3f], W[t-8f], W[t-14f], W[t-16f] and rotates left by f
TABLE = [
    (16, 1, (2, 0)), (17, 1, (3, 1)), (18, 1, (4, 2, 15)), (19, 1, (16, 3, 5)), (20, 1, (17, 4)), (21, 1, (18, 5)),
    (22, 1, (19,)), (23, 1, (20, 15)), (24, 1, (21, 16)), (25, 1, (22, 17)), (26, 1, (23, 18)), (27, 1, (24, 19)),
    (28, 1, (25, 20)), (29, 1, (26, 21, 15)), (30, 1, (27, 22, 16)), (31, 1, (28, 23, 17, 15)),
    (32, 1, (29, 24, 18, 16)), (33, 1, (30, 25, 19, 17)), (34, 2, (28, 18, 2)), (35, 2, (29, 19, 3)),
    (36, 2, (30, 20, 4)), (37, 2, (31, 21, 5)), (38, 2, (32, 22)), (39, 2, (33, 23)), (40, 2, (34, 24)),
    (41, 2, (35, 25)), (42, 2, (36, 26)), (43, 2, (37, 27, 15)), (44, 2, (38, 28, 16)), (45, 2, (39, 29, 17)),
    (46, 2, (40, 30, 18)), (47, 1, (44, 39, 33, 31)), (48, 1, (45, 40, 34, 32)), (49, 1, (46, 41, 35, 33)),
    (50, 1, (47, 42, 36, 34)), (51, 1, (48, 43, 37, 35)), (52, 1, (49, 44, 38, 36)), (53, 1, (50, 45, 39, 37)),
    (54, 1, (51, 46, 40, 38)), (55, 1, (52, 47, 41, 39)), (56, 1, (53, 48, 42, 40)), (57, 1, (54, 49, 43, 41)),
    (58, 1, (55, 50, 44, 42)), (59, 1, (56, 51, 45, 43)), (60, 1, (57, 52, 46, 44)), (61, 1, (58, 53, 47, 45)),
    (62, 1, (59, 54, 48, 46)), (63, 1, (60, 55, 49, 47)), (64, 4, (52, 32, 0)), (65, 4, (53, 33, 1)),
    (66, 4, (54, 34, 2)), (67, 4, (55, 35, 3)), (68, 4, (56, 36, 4)), (69, 4, (57, 37, 5)), (70, 4, (58, 38)),
    (71, 4, (59, 39, 15)), (72, 4, (60, 40, 16)), (73, 4, (61, 41, 17)), (74, 4, (62, 42, 18)),
    (75, 4, (63, 43, 19)), (76, 4, (64, 44, 20)), (77, 4, (65, 45, 21)), (78, 4, (66, 46, 22)),
    (79, 1, (76, 71, 65, 63)),
]


def rol(x, s):
    return ((x << s) | (x >> (32 - s))) & M32


def block(m):
    return list(m) + [PAD] + [0] * 9 + [BITS]


def schedule_plain(m):
    w = block(m)
    for t in range(16, 80):
        w.append(rol(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1))
    return w


def schedule_table(m):
    w = block(m) + [None] * 64
    for t, f, ins in TABLE:
        x = 0
        for i in ins:
            x ^= w[i]
        w[t] = rol(x, f)
    return w


def compress(st, w):
    a, b, c, d, e = st
    for t in range(80):
        if t < 20:
            f, k = (b & c) | (~b & d & M32), 0x5A827999
        elif t < 40:
            f, k = b ^ c ^ d, 0x6ED9EBA1
        elif t < 60:
            f, k = (b & c) | (b & d) | (c & d), 0x8F1BBCDC
        else:
            f, k = b ^ c ^ d, 0xCA62C1D6
        a, b, c, d, e = (rol(a, 5) + f + e + k + w[t]) & M32, a, rol(b, 30), c, d
    return [(x + y) & M32 for x, y in zip(st, (a, b, c, d, e))]


IV = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]


def messages():
    rng = random.Random(20)
    ms = [[rng.getrandbits(32) for _ in range(5)] for _ in range(1000)]
    ms += [[0] * 5, [M32] * 5]
    ms += [[(1 << b) if j == i else 0 for j in range(5)] for i in range(5) for b in range(32)]
    return ms


def test_table_is_the_three_recurrences_over_the_non_zero_inputs():
    assert [t for t, _, _ in TABLE] == list(range(16, 80))
    for t, f, ins in TABLE:
        assert f in (1, 2, 4) and t >= 16 * f
        src = [t - 3 * f, t - 8 * f, t - 14 * f, t - 16 * f]
        assert sorted(ins) == sorted(s for s in src if not 6 <= s <= 14), t
        assert sum(i in (5, 15) for i in ins) <= 1, t             # at most one constant operand per word


def test_table_op_count():
    """ceil((n - 1) / 2) XOR instructions (three-input v_bitop3, or v_xor) and one rotate per word of n non-zero
    inputs: 148 for the 64 words against the standard recurrence's 176, which takes work.INSTR's 578 per compression
    to 550."""
    ops = sum(len(ins) // 2 + 1 for _, _, ins in TABLE)
    assert ops == 148
    std = sum(len([s for s in (t - 3, t - 8, t - 14, t - 16) if not 6 <= s <= 14]) // 2 + 1 for t in range(16, 80))
    assert std == 176
    assert 578 - (std - ops) == 550
    assert [t for t, f, _ in TABLE if f == 2] == list(range(34, 47))
    assert [t for t, f, _ in TABLE if f == 4] == list(range(64, 79))


def test_table_schedule_equals_plain_recurrence_and_hashlib():
    rng = random.Random(21)
    for n, m in enumerate(messages()):
        w = schedule_table(m)
        assert w == schedule_plain(m), m
        if n % 8 == 0:
            # continued from a midstate, as in HMAC: SHA1(prefix | m) with a random 64-byte prefix
            prefix = bytes(rng.getrandbits(8) for _ in range(64))
            mid = compress(IV, schedule_plain_block(prefix))
            want = hashlib.sha1(prefix + struct.pack(">5I", *m)).digest()
            assert struct.pack(">5I", *compress(mid, w)) == want, m


def schedule_plain_block(b64):
    w = list(struct.unpack(">16I", b64))
    for t in range(16, 80):
        w.append(rol(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1))
    return w


# ------------------------------------------------------------------ GPU
LOWER = "abcdefghijklmnopqrstuvwxyz"
ODT = ("odt_testdoc_std", "odt_testdoc_e")


@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device: GPU tests need the MI355X box"
    return _lib


def _ctx(dprf, stream):
    from dprf_amd import brute_force as bf
    return dprf.Context(bf.parse_verification_data(stream))


def _index(pw):
    idx = 0
    for ch in pw:
        idx = idx * len(LOWER) + LOWER.index(ch)
    return idx


@pytest.fixture(scope="module")
def range_verdicts(oracle, streams):
    """oracle verdicts of the keyspace indices idx - 256 .. idx + 256 around each stream's password, computed once"""
    out = {}
    for name in ODT:
        pw = streams[name]["password"]
        idx, octx = _index(pw), oracle.Ctx(streams[name]["stream"])
        out[name] = {i: octx.verify(oracle.index_to_password(i, LOWER, len(pw))) for i in range(idx - 256, idx + 257)}
        assert out[name][idx] == 1
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ODT)
@pytest.mark.parametrize("count", [1, 65, 257])
def test_range_mode_windows(dprf, streams, range_verdicts, name, count):
    """k_odt_kdf<0>: the password alone, and at the first and the last index of windows of 65 (a partial second wave)
    and 257 candidates (a partial second block)"""
    pw = streams[name]["password"]
    idx = _index(pw)
    c = _ctx(dprf, streams[name]["stream"])
    for start in sorted({idx, idx - count + 1}):
        hits, n, st = c.search_range(LOWER, len(pw), start, count)
        want = [i for i in range(start, start + count) if range_verdicts[name][i] == 1]
        assert idx in want
        assert hits == want and n == len(want), (name, start, count)
        assert st["candidates"] == count
    c.close()


def _wrong_words(rng, n):
    return ["".join(rng.choice(LOWER) for _ in range(rng.randint(1, 12))) for _ in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ODT)
def test_list_mode_positions(dprf, oracle, streams, name):
    """k_odt_kdf<1>: 257 candidates, the password at 0, 63, 64 and 256 among wrong ones"""
    pw = streams[name]["password"]
    words = _wrong_words(random.Random(22), 257)
    for k in (0, 63, 64, 256):
        words[k] = pw
    want = [i for i, v in enumerate(oracle.Ctx(streams[name]["stream"]).verify_list(words)) if v == 1]
    assert {0, 63, 64, 256} <= set(want)
    c = _ctx(dprf, streams[name]["stream"])
    hits, n, st = c.verify_list(words)
    assert hits == want and n == len(want) and st["candidates"] == len(words)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["odt_long_std_100", "odt_long_e_200"])
def test_long_list_hit(dprf, oracle, long_verdicts, name):
    """k_odt_kdf<2> behind k_long_prehash: a candidate longer than a 64-byte list slot is the hit, beside a short
    wrong one.  The password of odt_testdoc_std / _e has 8 bytes and cannot be such a hit, so the documents are the
    golden ODF streams whose passwords are long (tests/golden/long_verdicts.json, std and -e); the two short-password
    streams go through the same kernel in test_long_list_miss_beside_short_hit."""
    d = long_verdicts[name]
    pw = d["password"]
    assert len(pw.encode()) > 64
    words = ["wrong", pw]
    octx = oracle.Ctx(d["stream"])
    want = [i for i, w in enumerate(words) if octx.verify(w) == 1]
    assert want == [1]
    c = _ctx(dprf, d["stream"])
    hits, n, st = c.verify_list(words)
    assert hits == want and n == 1 and st["candidates"] == 2
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ODT)
def test_long_list_miss_beside_short_hit(dprf, oracle, streams, name):
    pw = streams[name]["password"]
    words = [pw + "x" * 70, pw, "y" * 65]
    octx = oracle.Ctx(streams[name]["stream"])
    want = [i for i, w in enumerate(words) if octx.verify(w) == 1]
    assert 1 in want
    c = _ctx(dprf, streams[name]["stream"])
    hits, n, st = c.verify_list(words)
    assert hits == want and n == len(want) and st["candidates"] == 3
    c.close()
