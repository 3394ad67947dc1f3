"""CPU restatement of k_spell_hybrid (dprf_amd/csrc/dprf_kernels_spell.hip) and of the host side that feeds it
(dprf_host.cpp: dprf_ctx_set_words' packed table -- converted bytes clipped to a slot, u32 offsets --, and
dprf_search_hybrid's mask table and per-launch arguments: the chunk start's mask digits and its word index) against an
independent speller: divmod(i, M), the mask part by divmod over the positions, bytes concatenated in spelling order,
converted and truncated as the format does.

The model runs the kernel block by block the way the device does, in the manner of test_mask_model (whose mask table,
fastdiv and tile read-out it shares): every lane's first pass over the digits gives the mask part's length and, from
what the digit loop leaves over (rem + carry), the word index w0 + rem + carry; lane 0 and the last live lane publish
the run's ends; the block stages the run's offsets and its bytes as whole u32 words from the word that holds the
run's first byte; the second pass spells right to left, the word before mask position word_at.  LDS the block did
not stage reads as garbage, the device table is exactly as long as the host made it (a read past it raises), and the
output buffers carry a sentinel past the window's end.  A window may be cut into chunks as run_call cuts it.

M = 257 cannot be built -- 257 is prime and a position holds at most 256 symbols --, so the shapes around the block
size are M = 255, 256 and 258 (2 x 129)."""
import os
import random
import re

import pytest

import test_mask_model as mm
from test_mask_model import GARBAGE, M32, NO_TRUNC, SENTINEL, SLOT_WORDS, ST

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dprf_amd", "csrc")
PARAMS = open(os.path.join(CSRC, "dprf_params.h")).read()
RUN = int(re.search(r"#define DPRF_HYB_RUN (\d+)", PARAMS).group(1))     # a block's longest run of words
RUN_WORDS = RUN * SLOT_WORDS + 1                                         # DPRF_HYB_RUN_WORDS
SLOT = 4 * SLOT_WORDS
LOWER, DIGITS = mm.LOWER, mm.DIGITS


class Refused(Exception):
    pass


# ------------------------------------------------------------------ host side (dprf_host.cpp)
def host_words(words, office):
    """dprf_ctx_set_words: (blob as u32 words, offsets, longest converted length).  words: bytes."""
    data, off, longest = bytearray(), [0], 0
    for w in words:
        if not w or b"\0" in w:
            raise Refused("E_DOMAIN")
        if office:
            try:
                w = w.decode("utf-8").encode("utf-16-le")
            except UnicodeDecodeError:
                raise Refused("E_DOMAIN")
        longest = max(longest, len(w))
        data += w[:SLOT]
        off.append(len(data))
    data += bytes(-len(data) % 4)
    return [int.from_bytes(data[4 * k:4 * k + 4], "little") for k in range(len(data) // 4)], off, longest


def host_mask(positions, office):
    if not positions:
        return [0] * mm.TAB_WORDS, 0, [], 0
    tab, npool, radix, _ = mm.host_table(positions, office, NO_TRUNC)      # the slot check is the hybrid call's own
    return tab, npool, radix, sum(max(len(ch.encode("utf-16-le" if office else "utf-8")) for ch in p) for p in positions)


def host_args(radix, npool, trunc, word_at, nwords, bwords, first, count):
    sdig = [0] * (mm.MAX_POS // 4)
    v = first
    for p in range(len(radix) - 1, -1, -1):
        sdig[p >> 2] |= (v % radix[p]) << (8 * (p & 3))
        v //= radix[p]
    assert v < nwords
    return {"count": count, "npos": len(radix), "npool": npool, "trunc": trunc, "sdig": sdig, "word_at": word_at,
            "w0": v, "nwords": nwords, "bwords": bwords}


# ------------------------------------------------------------------ device side (dprf_kernels_spell.hip)
def digit(rec, p, rem, carry):
    r0 = rec[4 * p]
    radix = r0 & 0xffff
    q = rem if radix == 1 else mm.fastdiv(rem, rec[4 * p + 1], rec[4 * p + 2])
    d = ((r0 >> 16) + ((rem - q * radix) & M32) + carry) & M32
    carry = 1 if d >= radix else 0
    d -= radix if carry else 0
    return (rec[4 * p + 3] + d) & (mm.POOL - 1), q, carry


def spell_block(a, tab, wblob, woff, block, slots, lens):
    n = min(a["npos"], mm.MAX_POS)
    np_ = min(a["npool"], mm.POOL)
    rec = [GARBAGE] * mm.POOL_AT
    pw = [GARBAGE] * mm.POOL
    plw = [GARBAGE] * (mm.POOL // 4)
    for tid in range(256):
        if tid < mm.REC_WORDS * n:
            v = tab[tid]
            if tid & 3 == 0:
                v |= ((a["sdig"][tid >> 4] >> (8 * ((tid >> 2) & 3))) & 0xff) << 16
            rec[tid] = v
        for k in range(tid, np_, 256):
            pw[k] = tab[mm.POOL_AT + k]
        for k in range(tid, (np_ + 3) >> 2, 256):
            plw[k] = tab[mm.LENS_AT + k]
    pl = b"".join(w.to_bytes(4, "little") for w in plw)
    tile = bytearray(4 * SLOT_WORDS * ST)
    lim = min(a["trunc"], SLOT)
    base = block * 256
    ends = [GARBAGE, GARBAGE]
    mtotal, word = [0] * 256, [0] * 256
    for tid in range(256):
        g = base + tid
        if g >= a["count"]:
            continue
        rem, carry = g, 0
        for p in range(n - 1, -1, -1):
            en, rem, carry = digit(rec, p, rem, carry)
            mtotal[tid] += pl[en]
        w = (a["w0"] + rem + carry) & M32
        word[tid] = w if w < a["nwords"] else a["nwords"] - 1
        left = a["count"] - base
        if tid == 0:
            ends[0] = word[tid]
        if tid == min(left, 256) - 1:
            ends[1] = word[tid]
    # __syncthreads: the run's offsets and bytes
    wlo = ends[0]
    span = ends[1] - wlo + 1 if ends[1] >= wlo else 1
    nw = min(span, RUN)
    soff = [GARBAGE] * (RUN + 1)
    run = [GARBAGE] * RUN_WORDS
    b0, b1 = woff[wlo], woff[wlo + nw]
    a0 = b0 >> 2
    nu = (b1 - 4 * a0 + 3) >> 2 if b1 > 4 * a0 else 0
    nu = min(nu, RUN_WORDS)
    nu = min(nu, a["bwords"] - a0) if a0 < a["bwords"] else 0
    for tid in range(256):
        for k in range(tid, nw + 1, 256):
            soff[k] = woff[wlo + k]
        for k in range(tid, nu, 256):
            run[k] = wblob[a0 + k]
    rb = b"".join(w.to_bytes(4, "little") for w in run)
    staged = 4 * nu
    for tid in range(256):
        g = base + tid
        if g >= a["count"]:
            continue
        wi = min(word[tid] - wlo, RUN - 1)
        o0, o1 = soff[wi], soff[wi + 1]
        wl = min(o1 - o0 if o1 > o0 else 0, SLOT)
        src = (o0 - 4 * a0) & M32
        src = src if src <= 4 * RUN_WORDS - SLOT else 0
        total = mtotal[tid] + wl
        rem, carry, pos = g, 0, total
        for p in range(n - 1, -2, -1):
            if p + 1 == a["word_at"]:
                pos -= wl
                for j in range(wl):
                    if pos + j < lim:
                        assert src + j < staged, "a word byte the block did not stage"
                        tile[4 * (((pos + j) >> 2) * ST + tid) + ((pos + j) & 3)] = rb[src + j]
            if p < 0:
                break
            en, rem, carry = digit(rec, p, rem, carry)
            k, sy = pl[en], pw[en]
            pos -= k
            for j in range(k):
                if pos + j < lim:
                    tile[4 * (((pos + j) >> 2) * ST + tid) + ((pos + j) & 3)] = (sy >> (8 * j)) & 0xff
        assert pos == 0
        lens[g] = min(total, lim)
    for q in range(4):
        for tid in range(256):
            u = 256 * q + tid
            sl, w0 = u >> 2, 4 * (u & 3)
            if base + sl < a["count"]:
                o = 4 * (base * SLOT_WORDS + 4 * u)
                for i in range(4):
                    t = 4 * ((w0 + i) * ST + sl)
                    slots[o + 4 * i:o + 4 * i + 4] = tile[t:t + 4]


def spell_launch(tab, wblob, woff, a):
    count = a["count"]
    slots = bytearray([SENTINEL]) * (64 * (count + 256))
    lens = bytearray([SENTINEL]) * (count + 256)
    for block in range((count + 255) // 256):
        spell_block(a, tab, wblob, woff, block, slots, lens)
    assert slots[64 * count:] == bytearray([SENTINEL]) * (64 * 256), "a slot past the launch's count was written"
    assert lens[count:] == bytearray([SENTINEL]) * 256, "a length past the launch's count was written"
    return bytes(slots[:64 * count]), bytes(lens[:count])


def model_window(words, positions, word_at, start, count, trunc=NO_TRUNC, office=False, cuts=()):
    """The window as dprf_search_hybrid runs it: the tables once, then one launch per chunk [off, off + n)."""
    wblob, woff, wlong = host_words(words, office)
    tab, npool, radix, mlong = host_mask(positions, office)
    if not 0 <= word_at <= len(positions):
        raise Refused("E_INVALID")
    if min(wlong + mlong, trunc) > SLOT:
        raise Refused("E_PWLEN")
    if start + count > len(words) * mm.space(positions):
        raise Refused("E_INVALID")
    offs = [0] + list(cuts) + [count]
    assert offs == sorted(offs)
    parts = [spell_launch(tab, wblob, woff, host_args(radix, npool, trunc, word_at, len(words), len(wblob),
                                                      start + lo, hi - lo))
             for lo, hi in zip(offs, offs[1:]) if hi > lo]
    return b"".join(p[0] for p in parts), b"".join(p[1] for p in parts)


# ------------------------------------------------------------------ the independent speller
def spell(words, positions, word_at, i):
    w, r = divmod(i, mm.space(positions))
    chars = []
    for p in reversed(positions):
        r, d = divmod(r, len(p))
        chars.append(p[d])
    chars = "".join(reversed(chars))
    return chars[:word_at].encode() + words[w] + chars[word_at:].encode()


def want_window(words, positions, word_at, start, count, trunc=NO_TRUNC, office=False):
    lim = min(trunc, 64)
    slots, lens = [], []
    for i in range(start, start + count):
        b = spell(words, positions, word_at, i)
        b = (b.decode("utf-8").encode("utf-16-le") if office else b)[:lim]
        slots.append(b + bytes(64 - len(b)))
        lens.append(len(b))
    return b"".join(slots), bytes(lens)


def check(words, positions, word_at, start, count, trunc=NO_TRUNC, office=False, cuts=()):
    assert 0 <= start and start + count <= len(words) * mm.space(positions)
    got_s, got_l = model_window(words, positions, word_at, start, count, trunc, office, cuts)
    want_s, want_l = want_window(words, positions, word_at, start, count, trunc, office)
    if got_l != want_l or got_s != want_s:
        for k in range(count):
            a, b = (got_s[64 * k:64 * k + 64], got_l[k]), (want_s[64 * k:64 * k + 64], want_l[k])
            assert a == b, "index %d (window offset %d): model %s len %d, speller %s len %d" % (
                start + k, k, a[0].hex(), a[1], b[0].hex(), b[1])
    assert got_l == want_l and got_s == want_s


def table(n, seed, lo=1, hi=12, wide=False):
    """n words of lo..hi bytes from a fixed seed; wide: some 2-, 3- and 4-byte characters among the letters."""
    rng = random.Random(seed)
    alpha = LOWER + ("é€\U0001D11Eß" if wide else "")
    out = []
    for _ in range(n):
        want = rng.randint(lo, hi)
        w = ""
        while len(w.encode()) < want:
            ch = rng.choice(alpha)
            if len((w + ch).encode()) <= want:
                w += ch
            elif len(w.encode()) < want:
                w += rng.choice(LOWER)
        out.append(w.encode())
    return out


WORDS = table(700, 1, wide=True)
LONGS = table(600, 2, lo=1, hi=64, wide=True)          # 1..64 bytes mixed in every block
M258 = [mm.table(2, 3), mm.table(129, 4)]


def test_constants_are_the_kernel_s():
    assert RUN == 256 and "#define DPRF_HYB_RUN_WORDS (DPRF_HYB_RUN * DPRF_SLOT_WORDS + 1)" in PARAMS
    kernel = open(os.path.join(CSRC, "dprf_kernels_spell.hip")).read()
    for text in ("__shared__ uint32_t soff[DPRF_HYB_RUN + 1];", "__shared__ uint32_t run[DPRF_HYB_RUN_WORDS];",
                 "w = a.w0 + rem + carry;", "constexpr uint32_t ST = 258;"):
        assert text in kernel, text


def test_speller_is_word_major_product():
    import itertools
    words, pos = [b"x", b"yy", b"x"], ["ab", "-", DIGITS]
    ref = [w + "".join(t).encode() for w, t in itertools.product(words, itertools.product(*pos))]
    assert [spell(words, pos, 3, i) for i in range(len(ref))] == [("".join(t).encode() + w) for w, t in
                                                                   itertools.product(words, itertools.product(*pos))]
    assert [spell(words, pos, 0, i) for i in range(len(ref))] == ref
    assert spell(words, pos, 1, 20 + 13) == b"b" + b"yy" + b"-3"


def test_host_table_packs_and_clips():
    wblob, woff, longest = host_words([b"ab", b"c" * 70, "é".encode()], False)
    assert woff == [0, 2, 66, 68] and longest == 70 and len(wblob) == 17
    wblob, woff, longest = host_words(["a\U0001D11E".encode()], True)
    assert woff == [0, 6] and wblob == [0xD8340061, 0xDD1E]
    for bad, office in (([b""], False), ([b"a\0"], False), ([b"\xff"], True)):
        with pytest.raises(Refused, match="E_DOMAIN"):
            host_words(bad, office)
    a = host_args([10, 26], 36, NO_TRUNC, 1, 700, 5, 699 * 260 + 259, 1)
    assert a["w0"] == 699 and a["sdig"][0] == 9 | 25 << 8


@pytest.mark.parametrize("positions", [[], [DIGITS], [mm.table(255)], [mm.table(256)], M258],
                         ids=["M1", "M10", "M255", "M256", "M258"])
def test_shapes_around_the_block_size(positions):
    m = mm.space(positions)
    n = len(WORDS) * m
    for at in sorted({0, len(positions)}):
        check(WORDS, positions, at, 0, min(n, 600))
        check(WORDS, positions, at, n - 300, 300)                         # the keyspace's last block, partial
        check(WORDS, positions, at, 37 * m - 3, 521, cuts=(64, 320))      # chunk starts inside a word
    check(WORDS[:1], positions, 0, 0, min(m, 300))                        # a table of one word


def test_256_distinct_words_in_a_block_of_all_lengths():
    check(LONGS, [], 0, 0, 600)
    check(LONGS, [], 0, 77, 523, cuts=(256,))
    check([bytes([97 + k % 26]) * 64 for k in range(300)], [], 0, 0, 300)      # 256 x 64 bytes: the run is full
    check([b"ab"] + [bytes([97 + k % 26]) * 64 for k in range(300)], [], 0, 0, 301)   # ... and starts at byte 2
    check([b"abc"] + [bytes([97 + k % 26]) * 64 for k in range(300)], [], 0, 1, 300)  # ... and at byte 3


def test_block_inside_one_word_and_word_in_the_middle():
    pos = [LOWER, "-", DIGITS, DIGITS]                                    # M = 2600: ten blocks per word
    for at in range(5):
        check(WORDS, pos, at, 5 * 2600 + 256, 512)
        check(WORDS, pos, at, 6 * 2600 - 100, 300)                        # a word boundary inside a block
    check(WORDS, ["a€", "-", mm.table(255), "é\U0001D11E"], 2, 1020 * 3 - 7, 700)


def test_mask_over_2_32():
    pos = [LOWER] * 7                                                     # 26^7 = 8.0e9 > 2^32
    m = mm.space(pos)
    assert m > 1 << 32
    check(WORDS, pos, 7, (1 << 32) - 100, 400)                            # across 2^32 inside word 0
    check(WORDS, pos, 0, 3 * m + (1 << 32) - 100, 400, cuts=(100,))
    check(WORDS, pos, 3, 5 * m - 300, 600, cuts=(300,))                   # a word boundary at a chunk start
    check(WORDS, pos, 7, len(WORDS) * m - 257, 257)


def test_truncation_and_long_words():
    words = [b"x" * 29 + "€".encode(), b"y" * 70, b"z" * 30, b"w" * 64]
    check(words, ["€é", DIGITS], 2, 0, 80, trunc=32)                      # the cut inside the word's € and in a symbol
    check(words, ["€é", DIGITS], 0, 0, 80, trunc=32)
    check(words[2:], [], 0, 0, 2)                                         # 64 bytes with the empty mask
    with pytest.raises(Refused, match="E_PWLEN"):
        model_window(words, ["ab"], 0, 0, 1)
    with pytest.raises(Refused, match="E_PWLEN"):
        model_window(words, ["ab"], 0, 0, 1, trunc=127)
    check([b"q" * 60, b"r"], ["ab", "-", "cd", "e"], 4, 0, 8)             # exactly 64
    check([b"q" * 60, b"r"], ["ab", "-", "cd", "e"], 1, 0, 8, trunc=127)


def test_office_units():
    words = [w.decode().encode() for w in WORDS[:40]] + ["\U0001D11Eé".encode() * 5]
    check(words, ["a€", DIGITS, "\U00020000b"], 1, 0, 41 * 40, office=True, cuts=(256, 700))
    with pytest.raises(Refused, match="E_PWLEN"):
        model_window([("€" * 32).encode()], ["a"], 0, 0, 1, office=True)   # 64 + 2 bytes of UTF-16LE


def test_host_refusals():
    with pytest.raises(Refused, match="E_INVALID"):
        model_window(WORDS, [DIGITS], 2, 0, 1)
    with pytest.raises(Refused, match="E_INVALID"):
        model_window(WORDS, [DIGITS], 0, 6999, 2)
    model_window(WORDS, [DIGITS], 0, 6999, 1)
