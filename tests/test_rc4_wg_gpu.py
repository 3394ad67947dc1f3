"""The two-wave RC4 workgroup (dprf_amd/csrc/rc4_wg.h) at the window sizes where its frame can go wrong, for every
kernel of that shape: k_pdf_r24 (R2, R3 with a 40-bit key, R4), which is built on the header, and k_pdf_r24_owner and
k_oldoffice (MD5 and SHA-1 family), which write the same frame out; each in range mode and in list mode (the same
candidates packed with verify_list).

A workgroup takes NBAT batches of 64 candidates.  Window counts 1, 64, 65, 128, 129 and 192 give 1, 1, 2, 2, 3 and 3
batches: the owner pipeline's prologue (a second batch; a batch b + 2), and a last batch of one valid lane.  64 NBAT
and 64 NBAT + 1 fill one workgroup and start a second one with a single candidate.  Every window ends at the planted
password, so the hit sits in the last valid lane of the last batch.

The expected hit set is computed, never assumed: owner mode from tests/owner_model.py, user mode from the pinned
oracle (search_range for the range cases, verify_list for the list cases), Office 97-2003 from
tests/oldoffice_model.py -- the oracle has no verifier for that stream, the model is its pinned definition
(tests/test_oldoffice_model.py).  Each subject's verdicts are computed once over its largest window and shared."""
import contextlib
import functools
import io
import zlib

import pytest

import oldoffice_model as OM
import owner_model as M
from conftest import load_golden

pytestmark = pytest.mark.gpu

CS = "zyxwvutsrqponmlkjihgfedcba"           # every planted password's index leaves room for the largest window below it
CS5 = "678Ux"
SMALL = (1, 64, 65, 128, 129, 192)
# subject -> (document or Office 97-2003 type, role, batches per workgroup: R34_BATCHES, R2_BATCHES, OLDOFFICE_BATCHES)
SUBJECTS = {
    "r2-user": ("pdf_r2.pdf", "user", 36), "r2-owner": ("pdf_r2.pdf", "owner", 36),
    "r3_40-user": ("pdf_r3_l40.pdf", "user", 12), "r3_40-owner": ("pdf_r3_l40.pdf", "owner", 12),
    "r4-user": ("pdf_r4.pdf", "user", 12), "r4-owner": ("pdf_r4.pdf", "owner", 12),
    "office-md5": (1, "office", 32), "office-sha1": (4, "office", 32),
}
OFFICE_IDX = 3100                            # of 5^5 = 3125


@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device: GPU tests need the MI355X box"
    return _lib


def _fields(stream):
    from dprf_amd.brute_force import parse_verification_data
    with contextlib.redirect_stdout(io.StringIO()):
        return parse_verification_data(stream)


def counts(nbat):
    return SMALL + (64 * nbat, 64 * nbat + 1)


@functools.lru_cache(maxsize=None)
def subject(key):
    """(stream, charset, pwlen, index of the planted password) of a subject."""
    doc, role, _ = SUBJECTS[key]
    if role == "office":
        pw = OM.word(OFFICE_IDX, CS5, 5)
        s = OM.make_stream(pw, doc, seed=zlib.crc32(repr((pw, doc)).encode()))
        assert OM.verifies(s, pw)
        return s, CS5, 5, OFFICE_IDX
    d = load_golden("docs.json")[doc]
    pw = "owner" if role == "owner" else d["password"]
    return d["streams"]["std"]["stream"], CS, len(pw), M.index_of(pw, CS)


def reference(key, mode, oracle=None):
    """Hit indices of the subject's largest window [planted - widest + 1, planted], absolute, from the reference side;
    computed once per (subject, mode) and never changed."""
    return _reference(key, mode if SUBJECTS[key][1] == "user" else "any", oracle)


@functools.lru_cache(maxsize=None)
def _reference(key, mode, oracle):
    stream, cs, pwlen, idx = subject(key)
    role, widest = SUBJECTS[key][1], max(counts(SUBJECTS[key][2]))
    lo = idx - widest + 1
    assert lo >= 0
    if role == "owner":
        return tuple(lo + k for k in M.window_hits(stream, cs, pwlen, lo, widest))
    if role == "office":
        return tuple(k for k in range(lo, idx + 1) if OM.verifies(stream, OM.word(k, cs, pwlen)))
    octx = oracle.Ctx(stream)
    if mode == "range":
        hits, n = octx.search_range(cs, pwlen, lo, widest)
        assert n == len(hits)
        return tuple(hits)
    return tuple(lo + k for k, v in enumerate(octx.verify_list([M.word(lo + k, cs, pwlen) for k in range(widest)])) if v == 1)


@pytest.mark.parametrize("mode", ["range", "list"])
@pytest.mark.parametrize("key", list(SUBJECTS))
def test_window_ends_at_the_planted_password(dprf, oracle, key, mode):
    stream, cs, pwlen, idx = subject(key)
    role, nbat = SUBJECTS[key][1], SUBJECTS[key][2]
    ref = reference(key, mode, oracle)
    assert idx in ref, "the reference side finds the planted password"
    kw = {"pdf_password": "owner"} if role == "owner" else {}
    with dprf.Context(_fields(stream), device=0, **kw) as ctx:
        for count in counts(nbat):
            start = idx - count + 1
            want = [k for k in ref if k >= start]
            if mode == "range":
                run = lambda **o: ctx.search_range(cs, pwlen, start, count, **o)
            else:
                words = [M.word(start + k, cs, pwlen) for k in range(count)]
                want = [k - start for k in want]
                run = lambda **o: ctx.verify_list(words, **o)
            hits, n, st = run()
            print(key, mode, count, "hits", hits, "want", want, "candidates", st["candidates"])
            assert hits == want and n == len(want), (key, mode, count, hits, want)
            assert st["candidates"] == count, (key, mode, count, st["candidates"])
            first, n1, _ = run(stop_on_first=True, cap=1)
            assert n1 >= 1 and first == want[:1], (key, mode, count, first, want)
