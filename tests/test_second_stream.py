"""The second stream's spelled-slot buffer, once per window kind (symbols, mask, hybrid) and once in owner mode.

PDF R2-R4 alternate their launches between two streams, each with its own buffer of spelled slots; the list kernels
address a chunk's slots from a base pointer offset back by the chunk's offset in the window.  Every other window test
fits one first chunk (2^24 candidates for R2-R4, 2^23 in owner mode), so the second buffer and a non-zero offset are
only reached here: a window of one first chunk plus 4,097 candidates on a fresh context is two launches, the second on
the other stream, and the password is planted in that second launch.  A 10-candidate window on the same context follows:
a smaller window after a larger one, which grows no buffer.

The CPU half of each case needs no scan of the window: the reference (the oracle; owner_model in owner mode) verifies
the planted password and refuses its neighbour, and the project's spellers and this file's agree on the index."""
import functools
import os
import tempfile

import pytest

import test_mask_windows as mw
from test_mask_windows import DIGITS, LOWER

FIRST, FIRST_OWNER, TAIL = 1 << 24, 1 << 23, 4097
SYMBOLS = LOWER + "äöüßéè"                                # 32 symbols, six of two bytes; 32^5 = 2^25
HYBRID_WORDS = [(("é" if k % 3 == 0 else "x") + format(k, "x")).encode() for k in range(1 << 11)]
CASES = {
    # kind, positions, word slot, candidates of the window, planted index (among the last 4,096)
    "symbols": ("symbols", [SYMBOLS] * 5, None, FIRST + TAIL, FIRST + TAIL - 1000),
    "mask": ("mask", [LOWER] * 4 + [DIGITS] * 2, None, FIRST + TAIL, FIRST + 1),
    "hybrid": ("hybrid", [DIGITS] * 4, 0, FIRST + TAIL, FIRST + TAIL - 1),
    "owner-mask": ("mask", [LOWER] * 4 + [DIGITS] * 2, None, FIRST_OWNER + TAIL, FIRST_OWNER + 2049),
}
USER = "Usr!"                                             # the owner case's user password: outside the mask


def _spell(name, i):
    kind, pos, at, _, _ = CASES[name]
    if kind != "hybrid":
        return mw.word(i, pos).encode()
    w, r = divmod(i, mw.space(pos))
    chars = mw.word(r, pos)
    return chars[:at].encode() + HYBRID_WORDS[w] + chars[at:].encode()


@functools.lru_cache(maxsize=None)
def _stream(name):
    pw = _spell(name, CASES[name][4]).decode()
    if name != "owner-mask":
        return mw._stream_of("pdf", tuple(sorted(mw.R4.items())), pw)
    import docgen
    from dprf_amd.parsers import pdf2john
    with tempfile.TemporaryDirectory() as t:
        path = os.path.join(t, "d.pdf")
        docgen.write_pdf(path, USER, mw.SEED, owner=pw, **mw.R4)
        return pdf2john.get_hash(path)


@pytest.mark.parametrize("name", list(CASES))
def test_the_planted_password_lies_in_the_second_launch_and_verifies(name, oracle):
    from dprf_amd import brute_force, hybrid, mask as masks
    kind, pos, at, count, idx = CASES[name]
    first = FIRST_OWNER if name == "owner-mask" else FIRST
    keyspace = mw.space(pos) * (len(HYBRID_WORDS) if kind == "hybrid" else 1)
    assert count == first + TAIL and count - 4096 <= idx < count <= keyspace
    pw, near = _spell(name, idx), _spell(name, idx - 1)
    assert len(pw) <= 32 and pw != near
    if kind == "symbols":
        assert any(len(ch.encode()) == 2 for ch in SYMBOLS) and len(set(SYMBOLS)) == 32
        assert brute_force._index_to_password(idx, SYMBOLS, 5).encode() == pw
    elif kind == "mask":
        assert masks.word(pos, idx).encode() == pw and masks.index_of(pos, pw.decode()) == idx
    else:
        assert len(set(HYBRID_WORDS)) == 1 << 11
        assert hybrid.candidate(HYBRID_WORDS, pos, at, idx) == pw and hybrid.index_of(HYBRID_WORDS, pos, at, pw) == idx
    if name == "owner-mask":
        import owner_model
        assert owner_model.owner_verifies(_stream(name), pw) and not owner_model.owner_verifies(_stream(name), near)
        assert not owner_model.owner_verifies(_stream(name), USER.encode())
    else:
        c = oracle.Ctx(_stream(name))
        assert c.verify(pw) and not c.verify(near)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_second_stream_buffer_then_a_smaller_window(name):
    from dprf_amd import _lib
    kind, pos, at, count, idx = CASES[name]
    with _lib.Context(mw._fields(_stream(name)), device=0,
                      pdf_password="owner" if name == "owner-mask" else "user") as ctx:
        assert ctx.kernel == ("pdf_r24_owner" if name == "owner-mask" else "pdf_r24")
        if kind == "hybrid":
            ctx.set_words(HYBRID_WORDS)

        def search(start, n):
            if kind == "symbols":
                return ctx.search_symbols(SYMBOLS, 5, start, n, stop_on_first=False)
            if kind == "mask":
                return ctx.search_mask(pos, start, n, stop_on_first=False)
            return ctx.search_hybrid(pos, at, start, n, stop_on_first=False)

        hits, nhits, st = search(0, count)
        print(name, hits, nhits, st)
        assert st["launches"] == 2, "the window must be two launches for the second stream to run"
        assert hits == [idx] and nhits == 1 and st["candidates"] == count
        hits, nhits, st = search(idx - 3, 10)
        print(name, hits, nhits, st)
        assert hits == [idx] and nhits == 1 and st["candidates"] == 10 and st["launches"] == 1
