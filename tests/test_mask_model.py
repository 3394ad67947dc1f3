"""CPU restatement of k_spell_mask (csrc/dprf_kernels_spell.hip) and of the host side that feeds it (dprf_host.cpp
dprf_search_mask: the merged symbol pool, the per-position records with their own fastdiv magic, the chunk start's
mixed-radix digits packed into the kernel arguments) against an independent speller: itertools.product over the
positions' symbol lists, "".join(...).encode(), truncated at the format's limit.

The model runs the kernel block by block the way the device does: the records staged as {radix | start digit << 16,
magic, shift, pool base}, the start digit picked from byte p % 4 of argument word p / 4; the pool's words and byte
counts staged for the entries in use only; per thread the digits of g added to the start's digits with carries, last
position first, a radix-1 position taking q = rem without a division; once for the total length and once to store each
symbol's bytes right to left from it under pos + j < lim; lens[g] = min(total, lim); the read-out of the [word][slot]
tile (row stride 258) as 16-byte pieces under base + sl < count.  LDS the block did not stage reads as garbage, and
the output buffers carry a sentinel past the window's end, so a read of an unstaged entry or a store past `count` is
seen.  A window may be cut into chunks (one launch each, digits of start + off), as run_call cuts it."""
import itertools

import pytest

M32 = 0xffffffff
ST = 258                  # the tile's row stride in words
SLOT_WORDS = 16           # DPRF_SLOT_WORDS
MAX_POS = 32              # DPRF_MAX_RANGE_LEN = DPRF_MAX_PW_RANGE
POOL = 2048               # DPRF_MASK_POOL = DPRF_MAX_MASK_SYMBOLS
REC_WORDS = 4
POOL_AT = REC_WORDS * MAX_POS
LENS_AT = POOL_AT + POOL
TAB_WORDS = LENS_AT + POOL // 4
SENTINEL = 0xA5
GARBAGE = 0xDEADBEEF      # LDS words the block never staged
NO_TRUNC = M32            # dprf_search_mask: 32 for PDF R2-R4, 127 for R5, ~0 otherwise


class Refused(Exception):
    """dprf_search_mask's DPRF_E_CHARSET / DPRF_E_PWLEN, by name."""


# ------------------------------------------------------------------ host side (dprf_host.cpp)
def fastdiv_magic(d):
    if d <= 1:
        return 0, 0
    l = 0
    while (1 << l) < d:
        l += 1
    return (((1 << 32) * ((1 << l) - d)) // d + 1) & M32, l - 1


def host_table(positions, office, trunc):
    """The DPRF_MASK_TAB_WORDS words uploaded once per call, the pool entries in use, the radices and the longest
    candidate.  positions: a str of characters per position."""
    if not 1 <= len(positions) <= MAX_POS:
        raise Refused("E_PWLEN")
    tab = [0] * TAB_WORDS
    plen = bytearray(POOL)
    lists, radix, npool, sum_longest = [], [], 0, 0
    for p, chars in enumerate(positions):
        if not chars or len(chars) > 256:
            raise Refused("E_CHARSET")
        li = []
        for ch in chars:
            b = ch.encode("utf-16-le" if office else "utf-8")
            assert 1 <= len(b) <= 4
            v = len(b) << 32 | int.from_bytes(b, "little")
            if v in li:
                raise Refused("E_CHARSET")
            li.append(v)
        sum_longest += max(v >> 32 for v in li)
        radix.append(len(li))
        m, s = fastdiv_magic(len(li))
        same = next((o for o in range(p) if lists[o] == li), None)
        lists.append(li)
        rec = REC_WORDS * p
        tab[rec:rec + 3] = [len(li), m, s]
        if same is not None:
            tab[rec + 3] = tab[REC_WORDS * same + 3]
            continue
        if npool + len(li) > POOL:
            raise Refused("E_CHARSET")
        tab[rec + 3] = npool
        for k, v in enumerate(li):
            tab[POOL_AT + npool + k] = v & M32
            plen[npool + k] = v >> 32
        npool += len(li)
    for k in range(POOL // 4):
        tab[LENS_AT + k] = int.from_bytes(plen[4 * k:4 * k + 4], "little")
    longest = min(sum_longest, trunc)
    if longest > 4 * SLOT_WORDS:
        raise Refused("E_PWLEN")
    return tab, npool, radix, longest


def host_args(radix, npool, trunc, first, count):
    """dprf_mask_args of one launch: `count` candidates from keyspace index `first` (= start + off)."""
    sdig = [0] * (MAX_POS // 4)
    v = first
    for p in range(len(radix) - 1, -1, -1):
        sdig[p >> 2] |= (v % radix[p]) << (8 * (p & 3))
        v //= radix[p]
    assert v == 0
    return {"count": count, "npos": len(radix), "npool": npool, "trunc": trunc, "sdig": sdig}


# ------------------------------------------------------------------ device side (dprf_kernels_spell.hip)
def fastdiv(n, m, s):
    t = (n * m) >> 32
    return ((t + (((n - t) & M32) >> 1)) & M32) >> s


def spell_block(a, tab, block, slots, lens):
    """One 256-thread block of k_spell_mask; slots / lens are the launch's output buffers (bytearrays)."""
    n = min(a["npos"], MAX_POS)
    np_ = min(a["npool"], POOL)
    rec = [GARBAGE] * POOL_AT
    pw = [GARBAGE] * POOL
    plw = [GARBAGE] * (POOL // 4)
    for tid in range(256):
        if tid < REC_WORDS * n:
            v = tab[tid]
            if tid & 3 == 0:
                sw = a["sdig"][tid >> 4]
                v |= ((sw >> (8 * ((tid >> 2) & 3))) & 0xff) << 16
            rec[tid] = v
        for k in range(tid, np_, 256):
            pw[k] = tab[POOL_AT + k]
        for k in range(tid, (np_ + 3) >> 2, 256):
            plw[k] = tab[LENS_AT + k]
    pl = b"".join(w.to_bytes(4, "little") for w in plw)
    tile = bytearray(4 * SLOT_WORDS * ST)                 # every thread zeroes its own column
    lim = min(a["trunc"], 4 * SLOT_WORDS)
    for tid in range(256):
        g = block * 256 + tid
        if g >= a["count"]:
            continue
        total = 0
        for pas in range(2):
            rem, carry, pos = g, 0, total
            for p in range(n - 1, -1, -1):
                r0 = rec[4 * p]
                radix = r0 & 0xffff
                q = rem if radix == 1 else fastdiv(rem, rec[4 * p + 1], rec[4 * p + 2])
                d = ((r0 >> 16) + ((rem - q * radix) & M32) + carry) & M32
                carry = 1 if d >= radix else 0
                d -= radix if carry else 0
                rem = q
                en = (rec[4 * p + 3] + d) & (POOL - 1)
                k = pl[en]
                if pas == 0:
                    total += k
                else:
                    pos -= k
                    w = pw[en]
                    for j in range(k):
                        if pos + j < lim:
                            tile[4 * (((pos + j) >> 2) * ST + tid) + ((pos + j) & 3)] = (w >> (8 * j)) & 0xff
        lens[g] = min(total, lim)
    base = block * 256
    for q in range(4):
        for tid in range(256):
            u = 256 * q + tid
            sl, w0 = u >> 2, 4 * (u & 3)
            if base + sl < a["count"]:
                o = 4 * (base * SLOT_WORDS + 4 * u)
                for i in range(4):
                    t = 4 * ((w0 + i) * ST + sl)
                    slots[o + 4 * i:o + 4 * i + 4] = tile[t:t + 4]


def spell_launch(tab, a):
    """launch_spell_mask: GRID(count, 256) blocks.  Returns (slots, lens); 256 slots of sentinel stay behind them."""
    count = a["count"]
    slots = bytearray([SENTINEL]) * (64 * (count + 256))
    lens = bytearray([SENTINEL]) * (count + 256)
    for block in range((count + 255) // 256):
        spell_block(a, tab, block, slots, lens)
    assert slots[64 * count:] == bytearray([SENTINEL]) * (64 * 256), "a slot past the launch's count was written"
    assert lens[count:] == bytearray([SENTINEL]) * 256, "a length past the launch's count was written"
    return bytes(slots[:64 * count]), bytes(lens[:count])


def model_window(positions, start, count, trunc=NO_TRUNC, office=False, cuts=()):
    """The window as dprf_search_mask runs it: the table once, then one launch per chunk [off, off + n)."""
    tab, npool, radix, _ = host_table(positions, office, trunc)
    offs = [0] + list(cuts) + [count]
    assert offs == sorted(offs)
    parts = [spell_launch(tab, host_args(radix, npool, trunc, start + lo, hi - lo))
             for lo, hi in zip(offs, offs[1:]) if hi > lo]
    return b"".join(p[0] for p in parts), b"".join(p[1] for p in parts)


# ------------------------------------------------------------------ the independent speller
def space(positions):
    n = 1
    for p in positions:
        n *= len(p)
    return n


def words(positions, start, count):
    """itertools.product itself where the window lies within reach of islice; above that, block by block: product
    over the trailing positions (the fewest that make a block of 4096 or more) behind the block's fixed leading
    characters, which divmod finds."""
    if start + count <= 1 << 16:
        return ["".join(t) for t in itertools.islice(itertools.product(*positions), start, start + count)]
    split, tail = len(positions), 1
    while split > 0 and tail < 1 << 12:
        split -= 1
        tail *= len(positions[split])
    out = []
    while count:
        lo = start % tail
        n = min(count, tail - lo)
        head, v = [], start // tail
        for p in reversed(positions[:split]):
            v, r = divmod(v, len(p))
            head.append(p[r])
        head = "".join(reversed(head))
        out += [head + "".join(t) for t in itertools.islice(itertools.product(*positions[split:]), lo, lo + n)]
        start, count = start + n, count - n
    return out


def want_window(positions, start, count, trunc=NO_TRUNC, office=False):
    lim = min(trunc, 64)
    slots, lens = [], []
    for w in words(positions, start, count):
        b = w.encode("utf-16-le" if office else "utf-8")[:lim]
        slots.append(b + bytes(64 - len(b)))
        lens.append(len(b))
    assert len(lens) == count
    return b"".join(slots), bytes(lens)


def check(positions, start, count, trunc=NO_TRUNC, office=False, cuts=()):
    assert 0 <= start and start + count <= space(positions)
    got_s, got_l = model_window(positions, start, count, trunc, office, cuts)
    want_s, want_l = want_window(positions, start, count, trunc, office)
    if got_l != want_l or got_s != want_s:
        for k in range(count):
            a, b = (got_s[64 * k:64 * k + 64], got_l[k]), (want_s[64 * k:64 * k + 64], want_l[k])
            assert a == b, "index %d (window offset %d): model %s len %d, speller %s len %d" % (
                start + k, k, a[0].hex(), a[1], b[0].hex(), b[1])
    assert got_l == want_l and got_s == want_s


def table(nsym, salt=0):
    """nsym distinct characters of mixed widths: UTF-8 bytes 1, 2, 3, 4 by k % 4.  salt > 0 gives further tables that
    share no character with each other or with table 0 (2, 2, 3, 4 bytes: ASCII has no room for them)."""
    bases = (0x30 if salt == 0 else 0x400, 0x100, 0x1000, 0x10400)
    out = [chr(bases[k % 4] + k // 4 + 64 * salt) for k in range(nsym)]
    widths = (1 if salt == 0 else 2, 2, 3, 4)
    assert len(set(out)) == nsym and all(len(c.encode()) == widths[j % 4] for j, c in enumerate(out))
    return "".join(out)


LOWER = "abcdefghijklmnopqrstuvwxyz"
DIGITS = "0123456789"
# radices 2, 1, 255, 256, 3 and 1 again, with symbols of 1-4 bytes: keyspace 391,680
MIXED = ["a€", "-", table(255), table(256, 1), "x\U0001D11Eé", "é"]


def index_of(positions, w):
    i = 0
    for p, ch in zip(positions, w):
        i = i * len(p) + p.index(ch)
    return i


def test_far_speller_is_itertools_product():
    pos = ["ab", "cde", LOWER, "-", DIGITS, "xy"]
    ref = ["".join(t) for t in itertools.product(*pos)]
    assert words(pos, 0, len(ref)) == ref
    big = [LOWER] * 5
    ref = ["".join(t) for t in itertools.product(*big)]
    for start, count in ((1 << 16, 700), (26 ** 5 - 333, 333), (3 * 26 ** 3 - 100, 300), (26 ** 4 - 1, 2)):
        assert words(big, start, count) == ref[start:start + count], (start, count)


def test_host_table_merges_identical_positions():
    pos = [LOWER.upper(), LOWER, LOWER, "-", DIGITS, LOWER, "-", DIGITS]
    tab, npool, radix, longest = host_table(pos, False, NO_TRUNC)
    assert npool == 26 + 26 + 1 + 10 and radix == [26, 26, 26, 1, 10, 26, 1, 10] and longest == 8
    bases = [tab[REC_WORDS * p + 3] for p in range(len(pos))]
    assert bases == [0, 26, 26, 52, 53, 26, 52, 53]
    assert [tab[REC_WORDS * p + 1:REC_WORDS * p + 3] for p in (0, 3, 4)] == [list(fastdiv_magic(26)), [0, 0],
                                                                          list(fastdiv_magic(10))]
    assert tab[POOL_AT + 26] == ord("a") and tab[POOL_AT + 52] == ord("-") and tab[LENS_AT] == 0x01010101
    # Office: the same characters as UTF-16LE; lists that differ only in order are not merged
    tab, npool, _, longest = host_table(["a€", "€a", "\U0001D11E"], True, NO_TRUNC)
    assert npool == 5 and longest == 8 and tab[POOL_AT:POOL_AT + 5] == [0x61, 0x20AC, 0x20AC, 0x61, 0xDD1ED834]
    assert tab[LENS_AT] == 0x02020202 and tab[LENS_AT + 1] == 4


def test_start_digits_are_packed_one_byte_per_position():
    radix = [2, 1, 255, 256, 3, 1]
    a = host_args(radix, 0, NO_TRUNC, index_of(MIXED, "€-" + MIXED[2][254] + MIXED[3][255] + "é" + "é"), 1)
    assert a["sdig"][:2] == [1 | 0 << 8 | 254 << 16 | 255 << 24, 2 | 0 << 8] and a["npos"] == 6


def test_whole_small_keyspaces():
    for pos in (["a"], ["é"] * 32, ["ab"], ["a€", "-", "xyz"], ["-", "a€\U0001D11E", "-"], ["Inv-"[k] for k in range(4)] +
                [DIGITS, DIGITS, "€é"]):
        n = space(pos)
        check(pos, 0, n)
        if n > 64:
            check(pos, 0, n, cuts=(64,))
            check(pos, 0, n, trunc=127)


@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_mixed_radices_1_2_255_256(count):
    sp = space(MIXED)
    check(MIXED, 0, count)
    check(MIXED, sp - count, count)                                   # ends at the keyspace's last index
    check(MIXED, 3 * 256 * 255 - 100, count, trunc=32)


def test_carries_through_positions_of_different_radices():
    """Starts whose lower positions all hold their maximum digit: g = 1 carries through radices 1, 3, 256, 255 and 1
    into the first position."""
    start = index_of(MIXED, "a-" + MIXED[2][254] + MIXED[3][255] + "é" + "é")
    assert start == 255 * 256 * 3 - 1
    check(MIXED, start, 4)
    check(MIXED, start - 300, 700, cuts=(64, 320))
    start = index_of(MIXED, "a-" + MIXED[2][7] + MIXED[3][255] + "é" + "é")   # ... and one that stops at radix 255
    check(MIXED, start - 1, 300)
    wide = [DIGITS, "-", table(255), "ab", "-", table(256), "xyz", "-", "-"] + ["ab"] * 20    # keyspace > 2^32
    assert space(wide) > 1 << 40
    low = space(wide[1:])
    check(wide, 7 * low - 2, 300)                                     # every lower position rolls over
    check(wide, (1 << 32) - 100, 333, cuts=(128,))
    check(wide, (1 << 32) + 98765, 300)


def test_truncation_inside_a_multibyte_character():
    """PDF R2-R4 hash 32 bytes: ten literal € are 30 bytes, so the cut falls after E2 82 of an 11th € or ₭."""
    pos = ["€"] * 10 + ["a€é₭", "ab", "ab", "ab"]
    check(pos, 0, 32, trunc=32)
    check(pos, 0, 32)
    slots, lens = model_window(pos, 0, 32, trunc=32)
    assert set(lens) == {32}
    cut = ("€" * 10).encode() + b"\xe2\x82" + bytes(32)
    assert [k for k in range(32) if slots[64 * k:64 * k + 64] == cut] == list(range(8, 16)) + list(range(24, 32))


def test_slot_filled_and_office_units():
    check(["αβ"] * 32, (1 << 32) - 300, 300)
    check(["αβ"] * 32, 12345, 300, trunc=127)                         # PDF R5's limit lies past the slot: lim = 64
    check(["a€", "é\U0001D11E", "P", DIGITS, "\U00020000b"], 0, 80, office=True)
    check([table(256), "-", table(255, 1), table(3, 2)], 255 * 3 * 200 - 5, 300, office=True, cuts=(64,))


def test_pool_at_the_cap_and_one_over():
    eight = [table(256, k) for k in range(8)]
    tab, npool, _, _ = host_table(eight, False, NO_TRUNC)
    assert npool == POOL and tab[REC_WORDS * 7 + 3] == POOL - 256
    check(eight, 256 ** 8 - 300, 300)                                 # the pool's last entries are read
    check(eight, 0x1234567890AB, 257)
    # a ninth position with one of the same lists is merged and fits; one more distinct symbol does not
    host_table(eight + [eight[3]], False, NO_TRUNC)
    check(eight + [eight[3]], 256 ** 9 - 600, 300)
    for extra in ("-", table(256, 8)):
        with pytest.raises(Refused, match="E_CHARSET"):
            host_table(eight + [extra], False, NO_TRUNC)


def test_host_refusals():
    for pos, tr, what in (([], NO_TRUNC, "E_PWLEN"), (["a"] * 33, NO_TRUNC, "E_PWLEN"), (["ab", ""], NO_TRUNC, "E_CHARSET"),
                          ([table(256) + "~"], NO_TRUNC, "E_CHARSET"), (["aba"], NO_TRUNC, "E_CHARSET"),
                          (["a€"] * 22, NO_TRUNC, "E_PWLEN"), (["a€"] * 22, 127, "E_PWLEN")):
        with pytest.raises(Refused, match=what):
            host_table(pos, False, tr)
    host_table(["a€"] * 22, False, 32)                                # 66 bytes, but R2-R4 hash 32
    host_table(["a€"] * 21 + ["a"], False, NO_TRUNC)                  # 64 bytes fill the slot
