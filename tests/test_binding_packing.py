"""What _lib.Context hands to the library's search and verify exports, byte for byte: a recorder stands in for
libdprf.so (no device, no library), notes every argument and answers two hits.  Pins the symbol blob and the offset
arrays (their element widths too: the exports read uint32 symbol / position offsets and uint64 candidate offsets), the
order of the scalar arguments, and which methods add `start` to the indices the library reports."""
import ctypes

import numpy as np
import pytest

from dprf_amd import _lib

HANDLE = ctypes.c_void_p(0x1234)
REPORTED = [3, 5]                                         # what the recorder writes into `hits`


class _Recorder:
    """Every dprf_* export: notes (name, arguments before `hits`) and answers REPORTED through hits / nhits."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("dprf_"):
            raise AttributeError(name)

        def export(handle, *args):
            assert handle is HANDLE
            hits, cap, nh, st = args[-4:]
            assert isinstance(hits, ctypes.Array) and hits._type_ is ctypes.c_uint64 and len(hits) == max(1, cap)
            assert isinstance(st._obj, _lib.Stats) and isinstance(nh._obj, ctypes.c_int64)
            head = list(args[:-4])
            for k, a in enumerate(head):                  # a pointer into an array the method owns: read it now
                if isinstance(a, ctypes.POINTER(ctypes.c_uint64)):
                    head[k] = ("uint64 *", [a[j] for j in range(head[k + 1] + 1)])
            self.calls.append((name, tuple(head), cap))
            for k, h in enumerate(REPORTED[:cap]):
                hits[k] = h
            nh._obj.value = len(REPORTED)
            st._obj.candidates = 77
            return 0

        return export


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: r)
    return r


@pytest.fixture
def ctx():
    c = _lib.Context.__new__(_lib.Context)
    c._h = HANDLE
    yield c
    c._h = None


def _u32(arr):
    assert isinstance(arr, ctypes.Array) and arr._type_ is ctypes.c_uint32, arr
    return list(arr)


def _answer(res, start):
    hits, total, stats = res
    assert hits == [start + h for h in REPORTED] and total == 2 and stats["candidates"] == 77, res
    assert all(type(h) is int for h in hits)


def test_search_symbols_packs_characters_and_adds_start(rec, ctx):
    _answer(ctx.search_symbols("aé€\U0001D11E", 3, 100, 50, stop_on_first=True, cap=4), 100)
    _answer(ctx.search_symbols(b"\xffb", 2, 1, 3), 1)
    (n1, a1, c1), (n2, a2, c2) = rec.calls
    assert n1 == n2 == "dprf_search_symbols" and (c1, c2) == (4, 1 << 16)
    blob, off, nsym, pwlen, start, count, stop = a1
    assert blob == "aé€\U0001D11E".encode() and _u32(off) == [0, 1, 3, 6, 10]
    assert (nsym, pwlen, start, count, stop) == (4, 3, 100, 50, 1)
    blob, off, nsym, pwlen, start, count, stop = a2
    assert blob == b"\xffb" and _u32(off) == [0, 1, 2] and (nsym, pwlen, start, count, stop) == (2, 2, 1, 3, 0)


def test_search_mask_packs_positions_and_adds_start(rec, ctx):
    _answer(ctx.search_mask(["aé", b"\xff\x01", "€"], 7, 9), 7)
    (name, args, cap), = rec.calls
    blob, sym_off, pos_off, npos, start, count, stop = args
    assert name == "dprf_search_mask" and cap == 1 << 16
    assert blob == b"a\xc3\xa9\xff\x01\xe2\x82\xac"
    assert _u32(sym_off) == [0, 1, 3, 4, 5, 8] and _u32(pos_off) == [0, 2, 4, 5]
    assert (npos, start, count, stop) == (3, 7, 9, 0)


def test_search_hybrid_packs_positions_word_slot_and_adds_start(rec, ctx):
    _answer(ctx.search_hybrid([], 0, 40, 2), 40)                       # the bare word: no position at all
    _answer(ctx.search_hybrid(["é€", b"x", "\U0001D11E-"], 2, 1 << 40, 6, stop_on_first=True, cap=2), 1 << 40)
    (n1, a1, _), (n2, a2, c2) = rec.calls
    assert n1 == n2 == "dprf_search_hybrid" and c2 == 2
    blob, sym_off, pos_off, npos, word_at, start, count, stop = a1
    assert blob == b"" and _u32(sym_off) == [0] and _u32(pos_off) == [0]
    assert (npos, word_at, start, count, stop) == (0, 0, 40, 2, 0)
    blob, sym_off, pos_off, npos, word_at, start, count, stop = a2
    assert blob == "é€x\U0001D11E-".encode() and _u32(sym_off) == [0, 2, 5, 6, 10, 11] and _u32(pos_off) == [0, 2, 3, 5]
    assert (npos, word_at, start, count, stop) == (3, 2, 1 << 40, 6, 1)


def test_search_range_and_the_lists_report_indices_as_the_library_does(rec, ctx):
    _answer(ctx.search_range("abc", 4, 1000, 20, stop_on_first=True, cap=8), 0)
    _answer(ctx.verify_list(["pä", b"\xff", ""], cap=3), 0)
    _answer(ctx.verify_blob(b"abcde", np.array([0, 2, 5], dtype=np.int32), stop_on_first=True), 0)
    (n1, a1, c1), (n2, a2, c2), (n3, a3, c3) = rec.calls
    assert (n1, c1) == ("dprf_search_range", 8) and a1 == (b"abc", 3, 4, 1000, 20, 1)
    assert (n2, c2) == ("dprf_verify_list", 3) and (n3, c3) == ("dprf_verify_list", 1 << 16)
    blob, off, n, stop = a2
    assert isinstance(off, ctypes.Array) and off._type_ is ctypes.c_uint64
    assert blob == b"p\xc3\xa4\xff" and list(off) == [0, 3, 4, 4] and (n, stop) == (3, 0)
    blob, off, n, stop = a3
    assert blob == b"abcde" and off == ("uint64 *", [0, 2, 5]) and (n, stop) == (2, 1)


def test_a_cap_below_the_hit_count_returns_cap_indices_and_the_total(rec, ctx):
    hits, total, _ = ctx.search_mask(["ab"], 10, 2, cap=1)
    assert hits == [13] and total == 2
