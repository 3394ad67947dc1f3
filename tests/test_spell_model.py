"""CPU restatement of k_spell_symbols (dprf_amd/csrc/dprf_kernels_spell.hip) and of the host side that feeds it
(dprf_host.cpp dprf_search_symbols: the symbol table, the chunk start's digits, the fastdiv magic) against an independent
speller: divmod digits of the index, "".join(...).encode(), truncated at the format's limit.

The model runs the kernel block by block the way the device does: the block's [word][slot] LDS tile with a row stride
of 258 words, zeroed column by column; per thread the digits of g added to the chunk start's digits with carries, last
position first, once for the total length and once to store each symbol's bytes right to left from it under the guard
pos + j < lim; lens[g] = min(total, lim); then the read-out of the tile as 16-byte pieces u = 256 q + tid under the
guard base + sl < count.  A window may be cut into chunks (one launch each, digits of start + off), as run_call cuts it
at multiples of 64.  The output buffers carry a sentinel past the window's end, so a store past `count` is seen.

payload.spell_utf8 -- the host speller every GPU self-comparison in test_symbols.py leans on -- is pinned against the
same independent speller."""
import itertools

import pytest

M32 = 0xffffffff
ST = 258                  # the tile's row stride in words
SLOT_WORDS = 16           # DPRF_SLOT_WORDS
MAX_RANGE_LEN = 32        # DPRF_MAX_RANGE_LEN
SENTINEL = 0xA5
NO_TRUNC = M32            # dprf_search_symbols: 32 for PDF R2-R4, 127 for R5, ~0 otherwise


# ------------------------------------------------------------------ host side (dprf_host.cpp)
def utf8_to_utf16le(s):
    """utf8_to_utf16le of dprf_doc.cpp for one valid character: code point by shifts, surrogates by arithmetic."""
    b = s[0]
    if b < 0x80:
        cp, k = b, 1
    elif (b & 0xE0) == 0xC0:
        cp, k = b & 0x1F, 2
    elif (b & 0xF0) == 0xE0:
        cp, k = b & 0x0F, 3
    else:
        assert (b & 0xF8) == 0xF0
        cp, k = b & 0x07, 4
    assert k == len(s)
    for j in range(1, k):
        assert (s[j] & 0xC0) == 0x80
        cp = (cp << 6) | (s[j] & 0x3F)
    if cp >= 0x10000:
        v = cp - 0x10000
        hi, lo = 0xD800 | (v >> 10), 0xDC00 | (v & 0x3FF)
        return bytes([hi & 0xff, hi >> 8, lo & 0xff, lo >> 8])
    return bytes([cp & 0xff, cp >> 8])


def symbol_table(charset, office):
    """The 512 words the kernel reads: [256] LE-packed symbol bytes (Office: UTF-16LE), [256] byte counts."""
    tab = [0] * 512
    for k, ch in enumerate(charset):
        b = ch.encode("utf-8")
        if office:
            b = utf8_to_utf16le(b)
        assert 1 <= len(b) <= 4
        w = 0
        for j, x in enumerate(b):
            w |= x << (8 * j)
        tab[k], tab[256 + k] = w, len(b)
    return tab


def fastdiv_magic(d):
    if d <= 1:
        return 0, 0
    l = 0
    while (1 << l) < d:
        l += 1
    return (((1 << 32) * ((1 << l) - d)) // d + 1) & M32, l - 1


def host_enum(nsym, pwlen, first, count):
    """The dprf_enum of one launch: `count` candidates from keyspace index `first` (= start + off)."""
    sdig = [0] * MAX_RANGE_LEN
    v = first
    for p in range(pwlen - 1, -1, -1):
        sdig[p] = (v % nsym) & 0xff
        v //= nsym
    m, s = fastdiv_magic(nsym)
    return {"count": count, "pwlen": pwlen, "cslen": nsym, "div_m": m, "div_s": s, "sdig": sdig}


# ------------------------------------------------------------------ device side (dprf_kernels_spell.hip)
def fastdiv(n, m, s):
    t = (n * m) >> 32
    return ((t + (((n - t) & M32) >> 1)) & M32) >> s


def spell_block(e, tab, trunc, block, slots, lens):
    """One 256-thread block of k_spell_symbols; slots / lens are the launch's output buffers (bytearrays)."""
    sym, syl = tab[:256], tab[256:]
    tile = bytearray(4 * SLOT_WORDS * ST)                 # every thread zeroes its own column
    n = min(e["pwlen"], MAX_RANGE_LEN)
    lim = min(trunc, 4 * SLOT_WORDS)
    for tid in range(256):
        g = block * 256 + tid
        if g >= e["count"]:
            continue
        total = 0
        for pas in range(2):
            rem, carry, pos = g, 0, total
            for p in range(n - 1, -1, -1):
                q = rem if e["cslen"] == 1 else fastdiv(rem, e["div_m"], e["div_s"])
                d = (e["sdig"][p] + ((rem - q * e["cslen"]) & M32) + carry) & M32
                carry = 1 if d >= e["cslen"] else 0
                d -= e["cslen"] if carry else 0
                rem = q
                k = syl[d]
                if pas == 0:
                    total += k
                else:
                    pos -= k
                    w = sym[d]
                    for j in range(k):
                        if pos + j < lim:
                            tile[4 * (((pos + j) >> 2) * ST + tid) + ((pos + j) & 3)] = (w >> (8 * j)) & 0xff
        lens[g] = min(total, lim)
    # __syncthreads(); the read-out: 16-byte piece u of the block's slots is slot u / 4, words 4 (u % 4) ..
    base = block * 256
    for q in range(4):
        for tid in range(256):
            u = 256 * q + tid
            sl, w0 = u >> 2, 4 * (u & 3)
            if base + sl < e["count"]:
                o = 4 * (base * SLOT_WORDS + 4 * u)
                for i in range(4):
                    t = 4 * ((w0 + i) * ST + sl)
                    slots[o + 4 * i:o + 4 * i + 4] = tile[t:t + 4]


def spell_launch(charset, pwlen, first, count, trunc, office):
    """launch_spell_symbols: GRID(count, 256) blocks.  Returns (slots, lens) with 256 slots of sentinel behind."""
    e = host_enum(len(charset), pwlen, first, count)
    tab = symbol_table(charset, office)
    slots = bytearray([SENTINEL]) * (64 * (count + 256))
    lens = bytearray([SENTINEL]) * (count + 256)
    for block in range((count + 255) // 256):
        spell_block(e, tab, trunc, block, slots, lens)
    assert slots[64 * count:] == bytearray([SENTINEL]) * (64 * 256), "a slot past the launch's count was written"
    assert lens[count:] == bytearray([SENTINEL]) * 256, "a length past the launch's count was written"
    return bytes(slots[:64 * count]), bytes(lens[:count])


def model_window(charset, pwlen, start, count, trunc=NO_TRUNC, office=False, cuts=()):
    """The window as dprf_search_symbols runs it: one launch per chunk [off, off + n), each into its own buffer that
    the list kernels address as slot off + g."""
    offs = [0] + list(cuts) + [count]
    assert offs == sorted(offs)
    parts = [spell_launch(charset, pwlen, start + a, b - a, trunc, office) for a, b in zip(offs, offs[1:]) if b > a]
    return b"".join(p[0] for p in parts), b"".join(p[1] for p in parts)


# ------------------------------------------------------------------ the independent speller
def word(i, cs, n):
    out = []
    for _ in range(n):
        i, r = divmod(i, len(cs))
        out.append(cs[r])
    return "".join(reversed(out))


def spelled(i, cs, n, office=False):
    return word(i, cs, n).encode("utf-16-le" if office else "utf-8")


def want_window(cs, n, start, count, trunc=NO_TRUNC, office=False):
    lim = min(trunc, 64)
    slots, lens = [], []
    for i in range(start, start + count):
        b = spelled(i, cs, n, office)[:lim]
        slots.append(b + bytes(64 - len(b)))
        lens.append(len(b))
    return b"".join(slots), bytes(lens)


def check(cs, n, start, count, trunc=NO_TRUNC, office=False, cuts=()):
    assert 0 <= start and start + count <= len(cs) ** n
    got_s, got_l = model_window(cs, n, start, count, trunc, office, cuts)
    want_s, want_l = want_window(cs, n, start, count, trunc, office)
    if got_l != want_l or got_s != want_s:
        for k in range(count):
            a, b = (got_s[64 * k:64 * k + 64], got_l[k]), (want_s[64 * k:64 * k + 64], want_l[k])
            assert a == b, "index %d (window offset %d): model %s len %d, speller %s len %d" % (
                start + k, k, a[0].hex(), a[1], b[0].hex(), b[1])
    assert got_l == want_l and got_s == want_s


def table(nsym):
    """nsym distinct characters of mixed widths: UTF-8 bytes 1, 2, 3, 4 by k % 4 (UTF-16 units 1, 1, 1, 2)."""
    out = []
    for k in range(nsym):
        out.append(chr((0x30, 0x100, 0x1000, 0x10400)[k % 4] + k // 4))
    assert len(set(out)) == nsym and all(len(c.encode()) == 1 + j % 4 for j, c in enumerate(out))
    return "".join(out)


GREEK2 = "αβ"
CUT = "a€é₭"              # 1, 3, 2, 3 bytes; € = E2 82 AC and ₭ = E2 82 AD share the two bytes that survive the cut


def test_speller_is_itertools_product_order():
    cs, n = "aé€\U0001D11Eb", 4
    ref = ["".join(t) for t in itertools.product(cs, repeat=n)]
    assert [word(i, cs, n) for i in range(len(cs) ** n)] == ref
    assert [spelled(i, cs, n) for i in range(len(cs) ** n)] == [r.encode() for r in ref]


def test_symbol_table_is_le_packed_bytes_and_counts():
    tab = symbol_table("aé€\U0001D11E", False)
    assert tab[:4] == [0x61, 0xA9C3, 0xAC82E2, 0x9E849DF0] and tab[256:260] == [1, 2, 3, 4] and tab[4] == tab[260] == 0
    tab = symbol_table("aé€\U0001D11E", True)
    assert tab[:4] == [0x0061, 0x00E9, 0x20AC, 0xDD1ED834] and tab[256:260] == [2, 2, 2, 4]
    for ch in table(256) + "\uffff\U0010ffff\U00010000\u07ff\u0800\x7f\x80":
        assert utf8_to_utf16le(ch.encode()) == ch.encode("utf-16-le")


@pytest.mark.parametrize("cs,n", [("\U0001D11E", 1), ("é", 32), ("a\U0001D11E", 1), ("é€", 10), ("a€\U0001D11E", 6),
                                  ("aé€\U0001D11Eb", 4)],
                         ids=["1x1", "1x32", "2x1", "2x10", "3x6", "5x4"])
def test_whole_keyspaces(cs, n):
    space = len(cs) ** n
    check(cs, n, 0, space)
    if space > 256:
        check(cs, n, 0, space, cuts=(64, 320))              # chunk offsets that are multiples of 64, not of 256
        check(cs, n, 0, space, trunc=127)                   # PDF R5's limit lies past the slot: lim = 64


@pytest.mark.parametrize("nsym", [255, 256])
@pytest.mark.parametrize("n", [2, 8])
def test_large_tables(nsym, n):
    cs = table(nsym)
    space = nsym ** n
    check(cs, n, 0, 300)
    check(cs, n, space - 517, 517)                          # ends at space - 1
    check(cs, n, nsym - 3, 700, cuts=(192,))                # the last table entries, a digit roll-over, a 64-cut
    if n == 8:
        check(cs, n, (1 << 32) + 12345, 333)
        check(cs, n, 5 * nsym ** 7 - 2, 300)                # g = 2.. carries through 7 positions into the first
        check(cs, n, 9 * nsym ** 7 - 1, 451, cuts=(64, 128))


def test_slot_filled_exactly_by_32_two_byte_symbols():
    space = 1 << 32
    check(GREEK2, 32, 0, 300)
    check(GREEK2, 32, space - 700, 700, cuts=(320,))        # every slot 64 bytes, the last all second symbols
    check(GREEK2, 32, (1 << 31) - 2, 389)                   # a carry through 31 positions
    _, lens = model_window(GREEK2, 32, space - 3, 3)
    assert lens == bytes([64, 64, 64])


@pytest.mark.parametrize("cs,n,low", [("aé€\U0001D11Eb", 8, 7), ("aé€bc", 20, 19), (table(7), 12, 9)],
                         ids=["5x8", "5x20", "7x12"])
def test_carries_ripple_through_many_positions(cs, n, low):
    """Starts whose low digits are all nsym - 1: g = 1..3 carries through `low` >= 7 positions."""
    nsym = len(cs)
    for top in (1, nsym - 1):
        start = top * nsym ** low - 1                       # digits: top - 1, then `low` times nsym - 1
        if start > nsym ** n - 400:
            start = nsym ** low - 1
        assert all((start // nsym ** p) % nsym == nsym - 1 for p in range(low))
        check(cs, n, start, 4)
        check(cs, n, start - 2, 333)
    if nsym ** n > 1 << 33:
        start = ((1 << 32) // nsym ** low + 1) * nsym ** low - 1
        assert start > 1 << 32
        check(cs, n, start, 300)


def test_truncation_inside_a_character():
    """PDF R2-R4 hash 32 bytes: "€" * 10 is 30 bytes, so the cut falls after E2 82 of a following € or ₭, and the
    two spell the same 32 bytes."""
    n = 14
    p = 0
    for ch in "€" * 10:
        p = p * 4 + CUT.index(ch)
    first = p * 256
    check(CUT, n, first - 150, 700, trunc=32, cuts=(128, 448))
    check(CUT, n, first - 150, 700)                         # the same window untruncated (ODF, R6)
    check(CUT, n, 4 ** n - 300, 300, trunc=32)
    check(CUT, n, 0, 417, trunc=32)
    slots, lens = model_window(CUT, n, first, 256, trunc=32)
    eur, kip = CUT.index("€") * 64, CUT.index("₭") * 64     # the 11th character is € or ₭: the same 32 bytes
    assert slots[64 * eur:64 * (eur + 64)] == slots[64 * kip:64 * (kip + 64)]
    assert slots[64 * eur:64 * eur + 64] == ("€" * 10).encode() + b"\xe2\x82" + bytes(32) and set(lens) == {32}


def test_office_units():
    cs = "aé€\U0001D11E"                                   # UTF-16LE bytes 2, 2, 2, 4
    check(cs, 4, 0, 256, office=True)
    check(cs, 4, 3, 250, office=True, cuts=(64,))
    check("aé€\U0001D11E\U00020000b", 4, 0, 6 ** 4, office=True)
    check(table(256), 8, (1 << 40) + 7, 300, office=True)


@pytest.mark.parametrize("count", [1, 63, 65, 255, 257, 300, 513])
def test_counts_off_the_block_and_wave_sizes(count):
    cs = "aé€\U0001D11Eb"
    check(cs, 6, 5 ** 6 - count, count)
    check(cs, 6, 1000, count, trunc=32)


def test_host_speller_equals_independent_speller():
    """payload.spell_utf8 (numpy) against the divmod speller: blob and offsets of two of the windows above."""
    from dprf_amd.payload import spell_utf8
    for cs, n, start, count in ((table(256), 8, 9 * 256 ** 7 - 1, 451), (CUT, 14, 4 ** 14 - 300, 300),
                                ("aé€\U0001D11Eb", 4, 0, 625)):
        blob, offs = spell_utf8(cs, n, start, count)
        want = [spelled(i, cs, n) for i in range(start, start + count)]
        assert len(offs) == count + 1 and int(offs[0]) == 0
        assert [blob[int(a):int(b)] for a, b in zip(offs, offs[1:])] == want
