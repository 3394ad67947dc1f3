"""k_spell_combine, every byte: dprf_spell_combine over whole small keyspaces equals dprf_amd.combine.candidate slot by
slot and length by length, after the format's cut (Office: the UTF-16LE of the pair).

About 300 left words of 1..12 characters of 1-4 bytes against right tables of N2 = 1, 2, 3, 255, 256, 257, 258 and 600
words: N2 = 1 puts 256 left words into one block; 2 and 3 wrap many times per block (the whole right table is staged)
and 3 drifts against the block size; 255 and 256 are the largest tables staged whole; 257, 258 and 600 wrap once per
block, at lane 1, lane 2 and mid-block (two byte ranges).  Then windows whose start is no multiple of 64 and whose end
leaves a partial block, the length edges 63 + 1, 1 + 63 and 32 + 32, the PDF R4 cut inside a character of either word
and exactly between them, and Office words with BMP and surrogate-pair characters, 16 + 16 units."""
import functools

import numpy as np
import pytest

from dprf_amd import combine
from test_hybrid_windows import ALPHA, table
from test_mask_windows import R4, R5, _fields, _stream_of

WIDE = ALPHA + "\U0001D11E\U00020000"                        # 1-4 byte characters
LEFT = table(300, 0xC0DE, 1, 12, WIDE)                        # at most 48 bytes
RIGHTS = {n: table(n, 0xC100 + n, 1, 4, WIDE) for n in (1, 2, 3, 255, 256, 257, 258, 600)}   # at most 16 bytes


def model(left, right, start, count, office=False, trunc=None):
    """(slots, lens) as dprf_spell_combine must write them, from combine.candidate."""
    slots = np.zeros((count, 64), dtype=np.uint8)
    lens = np.zeros(count, dtype=np.uint8)
    for k in range(count):
        b = combine.candidate(left, right, start + k)
        if office:
            b = b.decode("utf-8").encode("utf-16-le")
        b = b[:trunc]
        assert len(b) <= 64
        slots[k, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        lens[k] = len(b)
    return slots, lens


@functools.lru_cache(maxsize=None)
def whole(n2):
    """The model over the whole keyspace LEFT x RIGHTS[n2]: computed once, shared, never written to."""
    slots, lens = model(LEFT, RIGHTS[n2], 0, len(LEFT) * n2)
    slots.setflags(write=False)
    lens.setflags(write=False)
    return slots, lens


def _stream(kw):
    return _stream_of("pdf", tuple(sorted(kw.items())), "sun7")


def _same(got, want, what):
    gs, gl = got
    ws, wl = want
    assert gl.shape == wl.shape and gs.shape == ws.shape, what
    bad = np.nonzero((gl != wl) | (gs != ws).any(axis=1))[0]
    assert bad.size == 0, (what, "first differing candidate %d of %d" % (bad[0], bad.size), bytes(gs[bad[0]]),
                           int(gl[bad[0]]), bytes(ws[bad[0]]), int(wl[bad[0]]))


def test_the_tables_are_what_the_cases_claim():
    assert len(LEFT) == 300 and {len(w.decode()) for w in LEFT} == set(range(1, 13))
    assert max(len(w) for w in LEFT) <= 48 and max(len(w) for r in RIGHTS.values() for w in r) <= 16
    widths = {len(ch.encode()) for w in LEFT + RIGHTS[600] for ch in w.decode()}
    assert widths == {1, 2, 3, 4}
    assert len({len(w) for w in LEFT[:256]}) >= 15 and len({len(w) for w in RIGHTS[600]}) >= 8   # byte lengths
    for n2, right in RIGHTS.items():
        assert len(right) == n2
    slots, lens = whole(3)                                                  # the model itself: pairs in product order
    assert bytes(slots[4][:lens[4]]) == LEFT[1] + RIGHTS[3][1] and bytes(slots[4][lens[4]:]) == bytes(64 - lens[4])
    # a block of 256 wraps once past N2 = 257 and 258, at lane 1 and 2 of the keyspace's first block, and 600 mid-block
    assert [256 - n2 % 256 for n2 in (257, 258)] == [255, 254] and 600 % 256 == 88
    assert all(w for r in RIGHTS.values() for w in r) and all(LEFT)


@pytest.mark.gpu
@pytest.mark.parametrize("n2", sorted(RIGHTS))
def test_whole_keyspace_every_byte(n2):
    from dprf_amd import _lib
    total = len(LEFT) * n2
    with _lib.Context(_fields(_stream(R5)), device=0) as ctx:
        ctx.set_words(LEFT)
        ctx.set_right_words(RIGHTS[n2])
        assert (ctx.words, ctx.right_words) == (300, n2)
        _same(ctx.spell_combine_raw(0, total), whole(n2), "N2 = %d" % n2)
        assert ctx.last_call_devices() == []                                # nothing was verified


@pytest.mark.gpu
@pytest.mark.parametrize("n2,start,count", [(257, 77, 1000), (600, 600 * 3 + 599, 513), (600, 345, 1), (3, 1, 770),
                                           (256, 255, 258), (1, 44, 256), (258, 258 * 299 + 1, 257)])
def test_windows_off_the_block_grid(n2, start, count):
    """A start that is no multiple of 64 (so r0 != 0 wherever N2 does not divide it) and a partial last block."""
    from dprf_amd import _lib
    assert start % 64 and start + count <= 300 * n2
    ws, wl = whole(n2)
    with _lib.Context(_fields(_stream(R5)), device=0) as ctx:
        ctx.set_words(LEFT)
        ctx.set_right_words(RIGHTS[n2])
        _same(ctx.spell_combine_raw(start, count), (ws[start:start + count], wl[start:start + count]),
              (n2, start, count))
        # the spelled strings are the same candidates
        k = count // 2
        assert ctx.spell_combine(start + k, 1) == [combine.candidate(LEFT, RIGHTS[n2], start + k)]


@pytest.mark.gpu
def test_length_edges_fill_the_slot():
    from dprf_amd import _lib
    with _lib.Context(_fields(_stream(R5)), device=0) as ctx:
        for ll, rl in ((63, 1), (1, 63), (32, 32), (64 - 7, 7)):
            left, right = [b"k", b"L" * ll, b"m"], [b"R" * rl, b"s"]
            ctx.set_words(left)
            ctx.set_right_words(right)
            got = ctx.spell_combine_raw(0, 6)
            _same(got, model(left, right, 0, 6), (ll, rl))
            assert int(got[1][2]) == 64 and bytes(got[0][2]) == b"L" * ll + b"R" * rl
        ctx.set_words([b"L" * 33])                                          # one byte more is refused, by name
        ctx.set_right_words([b"s", b"R" * 32])
        with pytest.raises(_lib.DprfError) as ei:
            ctx.spell_combine_raw(0, 1)
        assert ei.value.code == _lib.E_PWLEN and "left word 0 takes 33 bytes, right word 1 takes 32" in str(ei.value)


@pytest.mark.gpu
def test_pdf_r4_cuts_at_32_bytes_wherever_the_cut_falls():
    from dprf_amd import _lib
    left = [b"A" * 64, b"B" * 70, ("x" * 30 + "€").encode(), b"C" * 32, b"D" * 30, b"E" * 31, b"f"]
    right = [b"z" * 64, "€uro".encode(), b"r" * 100, b"q"]
    with _lib.Context(_fields(_stream(R4)), device=0) as ctx:
        ctx.set_words(left)
        ctx.set_right_words(right)
        n = len(left) * len(right)
        got = ctx.spell_combine_raw(0, n)
        _same(got, model(left, right, 0, n, trunc=32), "R4")
        cand = lambda l, r: bytes(got[0][l * len(right) + r][:got[1][l * len(right) + r]])
        assert cand(0, 0) == b"A" * 32 and cand(1, 2) == b"B" * 32          # both words 64 bytes or more: the left's 32
        assert cand(2, 3) == b"x" * 30 + b"\xe2\x82"                        # inside a character of the left word
        assert cand(3, 1) == b"C" * 32                                      # exactly between the words
        assert cand(4, 1) == b"D" * 30 + b"\xe2\x82" and cand(5, 1) == b"E" * 31 + b"\xe2"   # inside the right's
        assert cand(6, 3) == b"fq" and int(got[1].max()) == 32


@pytest.mark.gpu
def test_office_pairs_are_utf16le_of_both_words():
    from dprf_amd import _lib
    office = _stream_of("docx", (), "sun7")
    left = ["€" * 16, "\U0001D11E" * 8, "aé", "P\U00020000b", "z"]
    right = ["\U00020000" * 8, "ß" * 16, "\U0001D11E", "€x", "7"]
    lb, rb = [w.encode() for w in left], [w.encode() for w in right]
    with _lib.Context(_fields(office), device=0) as ctx:
        ctx.set_words(lb)
        ctx.set_right_words(rb)
        got = ctx.spell_combine_raw(0, 25)
        _same(got, model(lb, rb, 0, 25, office=True), "office")
        assert int(got[1][0]) == int(got[1][6]) == 64                       # 16 + 16 units, BMP and pairs
        assert bytes(got[0][0]) == (left[0] + right[0]).encode("utf-16-le")
        assert bytes(got[0][6]) == (left[1] + right[1]).encode("utf-16-le")
        ctx.set_right_words(["\U00020000" * 8 + "x"])                       # 17 units on the right
        with pytest.raises(_lib.DprfError) as ei:
            ctx.spell_combine_raw(0, 1)
        assert ei.value.code == _lib.E_PWLEN
