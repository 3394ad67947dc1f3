"""The four device spellers (dprf_kernels_spell.hip) on one candidate sequence: the 625 candidates of S^4 over
S = a, b, é, €, 𝄞 (1 to 4 UTF-8 bytes; three blocks, the last with 113 live lanes), in itertools.product order, spelled

  symbols   as a symbol window over S                                            k_spell_symbols
  mask      as a mask with S at every position                                   k_spell_mask
  hybrid    as the 25 words of S^2 (product order) at word_at = 0 before [S, S]   k_spell_hybrid
  rules     as the 625 spelled words under the single rule ":"                    k_spell_rules

so index i means the same candidate in every kind, and what the kernels share -- tile, byte store, read-out, mask and
run staging -- is checked against itself as well as against the documents.  Four PDF R5 documents have the password
planted at index 0, 255, 256 and 624 (a block's first and last lane, the keyspace's last candidate); one Office 2007
document at 256 takes the UTF-16 paths and k_spell_rules<2>.  Over the windows [0, 625) and [200, 625) every kind must
find exactly the planted index, or nothing where it lies before the window's start.

A CPU test on the oracle alone shows that the planted index is each window's only hit, so no comparison passes
vacuously.  The oracle's sets are computed once and shared."""
import functools
import itertools

import pytest

from test_mask_windows import R5, _fields, _stream_of, word

S = "abé€\U0001D11E"
NPOS = 4
N = len(S) ** NPOS
POS = [S] * NPOS
WORDS2 = ["".join(t) for t in itertools.product(S, repeat=2)]
ALL = [word(i, POS) for i in range(N)]
DOCS = {"r5-0": ("pdf", R5, 0), "r5-255": ("pdf", R5, 255), "r5-256": ("pdf", R5, 256), "r5-624": ("pdf", R5, 624),
        "office-256": ("docx", {}, 256)}
WINDOWS = ((0, N), (200, N - 200))
KINDS = ("symbols", "mask", "hybrid", "rules")


def want(doc, start):
    idx = DOCS[doc][2]
    return [idx] if idx >= start else []


@functools.lru_cache(maxsize=None)
def stream(doc):
    kind, kw, idx = DOCS[doc]
    return _stream_of(kind, tuple(sorted(kw.items())), ALL[idx])


@functools.lru_cache(maxsize=None)
def oracle_hits(doc):
    """The oracle's hit indices over the whole keyspace, once per document."""
    import pyoracle
    verdicts = pyoracle.Ctx(stream(doc)).verify_list([w.encode() for w in ALL], nthreads=16)
    return [i for i, v in enumerate(verdicts) if v]


def search(ctx, kind, start, count):
    if kind == "symbols":
        return ctx.search_symbols(S, NPOS, start, count)
    if kind == "mask":
        return ctx.search_mask(POS, start, count)
    if kind == "hybrid":
        ctx.set_words(WORDS2)
        return ctx.search_hybrid([S, S], 0, start, count)
    from dprf_amd import rules
    ctx.set_words(ALL)
    return ctx.search_rules([rules.parse_rule(":")], start, count)


def test_the_four_spellings_are_one_sequence():
    assert N == 625 and (N + 255) // 256 == 3 and N - 512 == 113
    assert sorted(len(ch.encode()) for ch in S) == [1, 1, 2, 3, 4]
    assert len(WORDS2) == 25 and len(set(ALL)) == N
    assert ALL == ["".join(t) for t in itertools.product(S, repeat=NPOS)]          # symbols, mask
    assert ALL == [w + word(m, [S, S]) for w in WORDS2 for m in range(25)]         # hybrid: word i // 25, mask i % 25
    assert max(len(w.encode()) for w in ALL) == 16 and max(len(w.encode("utf-16-le")) for w in ALL) == 16
    assert [(s, s + c) for s, c in WINDOWS] == [(0, 625), (200, 625)]
    assert sorted(d[2] for d in DOCS.values()) == [0, 255, 256, 256, 624]


@pytest.mark.parametrize("doc", sorted(DOCS))
def test_planted_index_is_the_only_hit_on_the_oracle(doc):
    assert oracle_hits(doc) == [DOCS[doc][2]]
    for start, count in WINDOWS:
        assert [h for h in oracle_hits(doc) if start <= h < start + count] == want(doc, start)


@pytest.mark.gpu
@pytest.mark.parametrize("doc", sorted(DOCS))
def test_every_kind_finds_the_planted_index(doc):
    from dprf_amd import _lib
    assert oracle_hits(doc) == [DOCS[doc][2]]
    with _lib.Context(_fields(stream(doc)), device=0) as ctx:
        for start, count in WINDOWS:
            for kind in KINDS:
                hits, nh, st = search(ctx, kind, start, count)
                assert [h - start for h in hits] == [i - start for i in want(doc, start)], (doc, kind, start, hits)
                assert nh == len(hits) and st["candidates"] == count, (doc, kind, start, nh, st)
