"""Owner-password search on the device (ABI 9: dprf_ctx_set_pdf_password; k_pdf_r24_owner, k_pdf_r5_owner,
k_pdf_r6_owner) against tests/owner_model.py, the Python statement of the check, which tests/test_owner_model.py pins on
the CPU.  Everything runs through the ABI on the golden streams or on documents written into tmp_path by
docgen.write_pdf(..., owner=...) and parsed by the project's parser.

  (a) range windows around "owner" on every revision, two-way: the window's whole hit set equals the model's, which is
      asserted to hold exactly one index, and stop_on_first returns it
  (b) one context in both modes: the owner window hits only in owner mode, the user window only in user mode
  (c) planted owner passwords of the lengths at which the message layout changes, in list mode
  (d) mask and multi-byte symbol windows
  (e) two lanes on one device
  (f) the refusals, after which the context still serves"""
import contextlib
import functools
import io
import os

import pytest

import owner_model as M
from conftest import load_golden

pytestmark = pytest.mark.gpu

LOWER = "abcdefghijklmnopqrstuvwxyz"
OWNER_IDX = M.index_of("owner", LOWER)
assert OWNER_IDX == 6793245

# document of tests/golden/docs.json -> half width of the window around "owner": R3/R4 workgroups take 768 candidates
# (the window crosses four, its count is no multiple of 64), R2's take 2304; R6 costs the model 0.25 s per candidate
WINDOWS = [("pdf_r3_l128.pdf", 1500), ("pdf_r3_l40.pdf", 1500), ("pdf_r4.pdf", 1500), ("pdf_r4_meta0.pdf", 1500),
           ("pdf_r2.pdf", 2500), ("pdf_r5.pdf", 1500), ("pdf_r6.pdf", 12)]


@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device: GPU tests need the MI355X box"
    return _lib


@functools.lru_cache(maxsize=None)
def _docs():
    return load_golden("docs.json")


def _stream(name):
    return _docs()[name]["streams"]["std"]["stream"]


def _fields(stream):
    from dprf_amd.brute_force import parse_verification_data
    with contextlib.redirect_stdout(io.StringIO()):
        return parse_verification_data(stream)


@functools.lru_cache(maxsize=None)
def _model_window(name, half):
    """The model's hit set of the window, relative to its start; computed once and shared."""
    return tuple(M.window_hits(_stream(name), LOWER, 5, OWNER_IDX - half, 2 * half))


def _write(tmp_path, user, owner, seed, **kw):
    import docgen
    from dprf_amd.parsers import pdf2john
    path = os.path.join(str(tmp_path), "d_%d_%d.pdf" % (kw.get("R", 3), seed))
    docgen.write_pdf(path, user, seed, owner=owner, **kw)
    return pdf2john.get_hash(path)


# ---------------------------------------------------------------- (a) range windows
@pytest.mark.parametrize("name,half", WINDOWS)
def test_range_window_equals_the_model(dprf, name, half):
    want = list(_model_window(name, half))
    assert want == [half], "the model finds exactly the planted owner password in the window"
    start = OWNER_IDX - half
    with dprf.Context(_fields(_stream(name)), device=0, pdf_password="owner") as ctx:
        assert ctx.pdf_password == "owner" and ctx.kernel.endswith("_owner")
        hits, n, st = ctx.search_range(LOWER, 5, start, 2 * half)
        assert n == len(hits) and [h - start for h in hits] == want
        assert st["candidates"] == 2 * half
        first, n1, _ = ctx.search_range(LOWER, 5, start, 2 * half, stop_on_first=True, cap=1)
        assert n1 >= 1 and first[0] - start == want[0]


# ---------------------------------------------------------------- (b) one context, both modes
def test_same_context_both_modes(dprf):
    name, half = "pdf_r4.pdf", 1500
    assert list(_model_window(name, half)) == [half]
    user_pw = _docs()[name]["password"]
    assert user_pw == "fox"
    fox = M.index_of(user_pw, LOWER)
    lo = max(0, fox - 1500)
    with dprf.Context(_fields(_stream(name)), device=0) as ctx:
        assert ctx.pdf_password == "user" and ctx.kernel == "pdf_r24"
        ctx.set_pdf_password("owner")
        assert ctx.pdf_password == "owner" and ctx.kernel == "pdf_r24_owner"
        assert ctx.search_range(LOWER, 5, OWNER_IDX - half, 2 * half)[0] == [OWNER_IDX]
        assert ctx.search_range(LOWER, 3, lo, 3000)[0] == []
        ctx.set_pdf_password("user")
        assert ctx.pdf_password == "user" and ctx.kernel == "pdf_r24"
        assert ctx.search_range(LOWER, 5, OWNER_IDX - half, 2 * half)[0] == []
        assert ctx.search_range(LOWER, 3, lo, 3000)[0] == [fox]


# ---------------------------------------------------------------- (c) planted lengths, list mode
def _planted(L, salt):
    """L deterministic printable ASCII bytes."""
    return "".join(chr(33 + (7 * k + 13 * salt + k * k) % 90) for k in range(L))


def _changed_last(pw):
    return pw[:-1] + ("!" if pw[-1] != "!" else "#")


R24_DOCS = [{"R": 2, "length": 40}, {"R": 3, "length": 40}, {"R": 4, "length": 128}]
PLANTED = ([(kw, L) for kw in R24_DOCS for L in (1, 31, 32, 33)] +
           [({"R": 5, "length": 256}, L) for L in (1, 7, 8, 9, 32, 63, 64)] +
           [({"R": 6, "length": 256}, L) for L in (1, 15, 16, 17, 32, 64)])


@pytest.mark.parametrize("kw,L", PLANTED, ids=["R%d-%d-len%d" % (kw["R"], kw["length"], L) for kw, L in PLANTED])
def test_planted_owner_lengths(dprf, tmp_path, kw, L):
    owner = _planted(L, kw["R"])
    user = "usr"
    stream = _write(tmp_path, user, owner, 0x0B00 + L, **kw)
    words = [owner, _changed_last(owner), user]
    # R2-R4 hash the first 32 bytes: at 33 the changed byte lies past the cut and both spellings verify
    want = [0, 1] if (kw["R"] <= 4 and L == 33) else [0]
    assert [k for k, w in enumerate(words) if M.owner_verifies(stream, w.encode())] == want
    with dprf.Context(_fields(stream), device=0, pdf_password="owner") as ctx:
        assert ctx.verify_list(words)[0] == want
        ctx.set_pdf_password("user")
        assert ctx.verify_list(words)[0] == [2]


@pytest.mark.parametrize("R", [5, 6])
def test_long_owner_candidates_are_refused(dprf, tmp_path, R):
    import numpy as np
    stream = _write(tmp_path, "usr", "own", 0x0C00 + R, R=R, length=256)
    words = [b"own", b"x" * 65, b"y" * 64]
    blob = b"".join(words)
    offs = np.cumsum([0] + [len(w) for w in words]).astype(np.uint64)
    with dprf.Context(_fields(stream), device=0, pdf_password="owner") as ctx:
        with pytest.raises(dprf.DprfError) as ei:
            ctx.verify_list(words)
        assert ei.value.code == dprf.E_PWLEN and "owner" in str(ei.value) and "not supported yet" in str(ei.value)
        assert list(ctx.list_status(blob, offs)) == [0, dprf.E_PWLEN, 0]
        assert ctx.verify_list([words[0], words[2]])[0] == [0]             # the context still serves
        ctx.set_pdf_password("user")
        assert list(ctx.list_status(blob, offs)) == [0, 0, 0]              # user mode takes long candidates
        assert ctx.verify_list(words)[0] == []


# ---------------------------------------------------------------- (d) mask and symbols
@pytest.mark.parametrize("name", ["pdf_r4.pdf", "pdf_r6.pdf"])
def test_mask_window(dprf, name):
    from dprf_amd import mask as masks
    positions = masks.parse_mask("own?l?l", ())
    assert masks.space(positions) == 676 and masks.word(positions, 4 * 26 + 17) == "owner"
    assert M.owner_verifies(_stream(name), b"owner") and not M.owner_verifies(_stream(name), b"ownes")
    with dprf.Context(_fields(_stream(name)), device=0, pdf_password="owner") as ctx:
        assert ctx.search_mask(positions, 0, 676)[0] == [121]
        ctx.set_pdf_password("user")
        assert ctx.search_mask(positions, 0, 676)[0] == []


def test_symbol_window_multibyte(dprf, tmp_path):
    owner, charset = "пар€", "апр€"
    stream = _write(tmp_path, "usr", owner, 0x0D03, R=3, length=128)
    idx = M.index_of(owner, charset)
    want = [k for k in range(len(charset) ** 4) if M.owner_verifies(stream, M.word(k, charset, 4).encode("utf-8"))]
    assert want == [idx]
    with dprf.Context(_fields(stream), device=0, pdf_password="owner") as ctx:
        assert ctx.search_symbols(charset, 4, 0, len(charset) ** 4)[0] == [idx]
        assert ctx.verify_list([owner.encode("utf-8"), "пар$".encode("utf-8")])[0] == [0]


# ---------------------------------------------------------------- (e) two lanes on one device
def test_two_lanes_one_device(dprf):
    name, half = "pdf_r4.pdf", 1500
    assert list(_model_window(name, half)) == [half]
    start = OWNER_IDX - half
    with dprf.Context(_fields(_stream(name)), devices=[0, 0], pdf_password="owner") as ctx:
        hits, n, _ = ctx.search_range(LOWER, 5, start, 2 * half, stop_on_first=True, cap=1)
        assert [h - start for h in hits] == [half]
        per = ctx.last_call_devices()
        assert [d["device"] for d in per] == [0, 0]
        assert all(d["launches"] >= 1 and d["candidates"] > 0 for d in per), per


# ---------------------------------------------------------------- (f) refusals
def test_owner_mode_is_pdf_only(dprf, streams):
    for key in ("office_testdoc", "odt_testdoc_e"):
        with dprf.Context(_fields(streams[key]["stream"]), device=0) as ctx:
            with pytest.raises(dprf.DprfError) as ei:
                ctx.set_pdf_password("owner")
            assert ei.value.code == dprf.E_INVALID
    with dprf.Context(_fields(_stream("pdf_r4.pdf")), device=0) as ctx:
        with pytest.raises(dprf.DprfError) as ei:
            ctx.set_pdf_password("both")
        assert ei.value.code == dprf.E_INVALID and ctx.pdf_password == "user"
        assert dprf.lib().dprf_ctx_set_pdf_password(ctx._h, 7) == dprf.E_INVALID and ctx.pdf_password == "user"


def short_u_fields():
    """The R6 golden document with U cut to the 40 bytes the user check needs: the owner check, which reads 48, is out
    of domain on it.  tests/test_doc_layer.py runs the same fields through the document layer without a device."""
    fields = _fields(_stream("pdf_r6.pdf"))
    assert fields[8] == "48" and len(fields[9]) == 96
    fields[8], fields[9] = "40", fields[9][:80]
    return fields


def test_short_u_is_out_of_domain_and_user_mode_survives(dprf):
    e = _docs()["pdf_r6.pdf"]
    fields = short_u_fields()
    pw = e["password"]
    idx = M.index_of(pw, LOWER)
    with dprf.Context(fields, device=0) as ctx:
        with pytest.raises(dprf.DprfError) as ei:
            ctx.set_pdf_password("owner")
        assert ei.value.code == dprf.E_DOMAIN
        assert ctx.pdf_password == "user" and ctx.kernel == "pdf_r6"
        assert ctx.verify_list([pw, pw + "x"])[0] == [0]
        lo = max(0, idx - 32)
        assert ctx.search_range(LOWER, len(pw), lo, 64)[0] == [idx]
    with pytest.raises(dprf.DprfError) as ei:
        dprf.Context(fields, device=0, pdf_password="owner")
    assert ei.value.code == dprf.E_DOMAIN
