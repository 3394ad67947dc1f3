"""What _lib.Context hands to the combinator exports, byte for byte, in the recorder style of test_binding_packing.py: a
recorder stands in for libdprf.so (no device, no library).  Pins the right table's blob and its uint64 offsets, the order
of dprf_search_combine's scalars and that `start` is added to the indices it reports, the buffers dprf_spell_combine
writes into, and the window check before ctypes would wrap an oversized int."""
import ctypes

import numpy as np
import pytest

from dprf_amd import _lib

HANDLE = ctypes.c_void_p(0x1234)
REPORTED = [3, 5]
SPELLED = [b"sun7", b"", "é€".encode(), b"x" * 64]          # what the recorder spells, whatever is asked


class _Recorder:
    def __init__(self):
        self.calls = []
        self.right = 0

    def dprf_ctx_set_right_words(self, handle, blob, offs, n):
        assert handle is HANDLE and isinstance(offs, ctypes.POINTER(ctypes.c_uint64))
        self.calls.append(("dprf_ctx_set_right_words", bytes(blob), [offs[k] for k in range(n + 1)], n))
        self.right = n
        return 0

    def dprf_ctx_right_words(self, handle):
        assert handle is HANDLE
        return self.right

    def dprf_search_combine(self, handle, start, count, stop, hits, cap, nh, st):
        assert handle is HANDLE
        assert isinstance(hits, ctypes.Array) and hits._type_ is ctypes.c_uint64 and len(hits) == max(1, cap)
        assert isinstance(st._obj, _lib.Stats) and isinstance(nh._obj, ctypes.c_int64)
        self.calls.append(("dprf_search_combine", start, count, stop, cap))
        for k, h in enumerate(REPORTED[:cap]):
            hits[k] = h
        nh._obj.value = len(REPORTED)
        st._obj.candidates = 77
        return 0

    def dprf_spell_combine(self, handle, start, count, slots, lens):
        assert handle is HANDLE and isinstance(slots, int) and isinstance(lens, int)
        self.calls.append(("dprf_spell_combine", start, count))
        s = (ctypes.c_uint8 * (64 * count)).from_address(slots)
        n = (ctypes.c_uint8 * count).from_address(lens)
        assert not any(s) and not any(n)                      # the buffers come zeroed, count slots of 64 bytes
        for k in range(count):
            w = SPELLED[k % len(SPELLED)]
            s[64 * k:64 * k + len(w)] = w
            n[k] = len(w)
        return 0


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


def test_the_library_exports_and_the_binding_declares_the_four_symbols():
    L = _lib.lib()
    for name in ("dprf_ctx_set_right_words", "dprf_ctx_right_words", "dprf_search_combine", "dprf_spell_combine"):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert L.dprf_ctx_right_words.restype is ctypes.c_int64
    assert L.dprf_search_combine.argtypes[1:4] == [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
    assert L.dprf_abi_version() == 9


def test_set_right_words_packs_the_blob_and_uint64_offsets(rec, ctx):
    ctx.set_right_words(["é€", b"\xff\x00", "", b"2024"])
    ctx.set_right_words([])
    (n1, blob, offs, n), (n2, blob2, offs2, m) = rec.calls
    assert n1 == n2 == "dprf_ctx_set_right_words"
    assert blob == "é€".encode() + b"\xff\x00" + b"2024" and offs == [0, 5, 7, 7, 11] and n == 4
    assert blob2 == b"" and offs2 == [0] and m == 0                         # an empty sequence clears the table
    rec.right = 9
    assert ctx.right_words == 9 and type(ctx.right_words) is int


def test_search_combine_passes_the_window_and_adds_start(rec, ctx):
    hits, total, stats = ctx.search_combine(1 << 40, 6, stop_on_first=True, cap=4)
    assert hits == [(1 << 40) + 3, (1 << 40) + 5] and total == 2 and stats["candidates"] == 77
    assert all(type(h) is int for h in hits)
    assert ctx.search_combine(10, 2, cap=1)[:2] == ([13], 2)                # cap indices, the total beside them
    ctx.search_combine(0, 0)
    assert rec.calls == [("dprf_search_combine", 1 << 40, 6, 1, 4), ("dprf_search_combine", 10, 2, 0, 1),
                         ("dprf_search_combine", 0, 0, 0, 1 << 16)]


def test_spell_combine_hands_over_zeroed_buffers_and_cuts_by_the_lengths(rec, ctx):
    slots, lens = ctx.spell_combine_raw(100, 6)
    assert slots.shape == (6, 64) and slots.dtype == np.uint8 and lens.shape == (6,) and lens.dtype == np.uint8
    assert [int(x) for x in lens] == [4, 0, 5, 64, 4, 0]
    assert ctx.spell_combine(7, 5) == SPELLED + SPELLED[:1]
    assert ctx.spell_combine(7, 0) == []                                    # room for one slot, nothing returned
    assert rec.calls == [("dprf_spell_combine", 100, 6), ("dprf_spell_combine", 7, 5), ("dprf_spell_combine", 7, 0)]


def test_a_window_that_does_not_fit_64_bits_is_refused_before_ctypes_wraps_it(rec, ctx):
    for call in (lambda: ctx.search_combine(0, 1 << 64), lambda: ctx.search_combine(-1, 1),
                 lambda: ctx.search_combine((1 << 64) - 1, 1), lambda: ctx.spell_combine(1 << 64, 1),
                 lambda: ctx.spell_combine_raw(0, -1)):
        with pytest.raises(_lib.DprfError) as ei:
            call()
        assert ei.value.code == _lib.E_INVALID
    assert rec.calls == []


def test_a_library_without_the_exports_says_so(monkeypatch, ctx):
    class Old:
        pass
    monkeypatch.setattr(_lib, "lib", lambda: Old())
    for call in (lambda: ctx.set_right_words([b"a"]), lambda: ctx.right_words, lambda: ctx.search_combine(0, 1),
                 lambda: ctx.spell_combine(0, 1)):
        with pytest.raises(_lib.DprfError) as ei:
            call()
        assert ei.value.code == _lib.E_INVALID and "rebuild" in str(ei.value)
