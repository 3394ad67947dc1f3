"""The 40-bit key search on the device (dprf_search_key40: k_key40_pdf, k_key40_oldoffice) against tests/key40_model.py,
the Python statement of the definition, which tests/test_key40_model.py ties to the oracle, the Office model and the
public hashcat vectors on the CPU.  Documents are planted by the model (key40_model.plant): U, or encryptedVerifier /
encryptedVerifierHash, rewritten so that exactly the chosen key verifies.  The shapes are the smallest at which these
kernels can go wrong.

  (a) the keys of the golden streams and the public vectors, 100 keys either side
  (b) window edges on planted documents of all four families; index 2^32; key 0; the last key; a window past 2^40
  (c) every lane and seam of a window of two full workgroups plus a partial batch
  (d) the compares in the rejecting direction: one bit of U / evh flipped at every byte the full compare reads
  (e) a 2^20-key window per family
  (f) stop_on_first; two lanes on one device
  (g) refusals, after each of which the context still serves; owner mode; a never-matching context
  (h) end to end from generated documents: --key40 FROM-TO, and one run with --checkpoint"""
import contextlib
import functools
import io
import os

import pytest

import doc_layer
import key40_model as km
from conftest import load_golden

pytestmark = pytest.mark.gpu

FAMILIES = ["pdf_r2", "pdf_r34", "office_md5", "office_sha1"]
# keys per workgroup: 64 lanes x the batches per workgroup of the family's kernel (dprf_kernels.hip R2_BATCHES 36,
# R34_BATCHES 12; dprf_kernels_oldoffice.hip OLDOFFICE_BATCHES 32)
BATCHES = {"pdf_r2": 36, "pdf_r34": 12, "office_md5": 32, "office_sha1": 32}
SPACE = 1 << 40


@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _base(fam):
    return tuple(km.base_documents()[fam])


def _planted(fam, index):
    return km.plant(list(_base(fam)), km.key_bytes(index), seed=index & 0xffff)


def _search(dprf, fields, start, count, **kw):
    with dprf.Context(fields, device=0) as ctx:
        return ctx.search_key40(start, count, **kw)


def _model_hits(fields, start, count):
    return [i for i in range(start, start + count) if km.key_verifies(fields, km.key_bytes(i))]


# ---------------------------------------------------------------- (a)
def _vector_cases():
    vec = load_golden("key40_vectors.json")
    streams = load_golden("streams.json")
    out = [(n, streams[n]["stream"], e["key"]) for n, e in sorted(vec["streams"].items())]
    out += [(n, e["stream"], e["key"]) for n, e in sorted(vec["public"].items())]
    return out


@pytest.mark.parametrize("name", [c[0] for c in _vector_cases()])
def test_a_golden_and_public_keys(dprf, name):
    _, stream, key = [c for c in _vector_cases() if c[0] == name][0]
    fields = km.fields_of(stream)
    idx = km.key_index(key)
    assert km.key_verifies(fields, bytes.fromhex(key))
    hits, n, st = _search(dprf, fields, idx - 100, 200)
    assert hits == [idx] and n == 1
    assert st["candidates"] == 200


# ---------------------------------------------------------------- (b)
@pytest.mark.parametrize("fam", FAMILIES)
def test_b_window_edges(dprf, fam):
    start = 0x3a7f12c5                                      # no multiple of anything
    for count in (1, 63, 65, 125, 513):
        for idx in sorted({start, start + count - 1}):
            with dprf.Context(_planted(fam, idx), device=0) as ctx:
                hits, n, st = ctx.search_key40(start, count)
                assert (hits, n, st["candidates"]) == ([idx], 1, count), (count, idx)
                # one key either side of the window: the key is outside
                if idx == start:
                    assert ctx.search_key40(start + 1, count)[0] == []
                else:
                    assert ctx.search_key40(start, count - 1)[0] == []


@pytest.mark.parametrize("fam", FAMILIES)
def test_b_index_two_to_the_32(dprf, fam):
    """One launch crosses index 2^32: the kernel's start + g is a 64-bit add."""
    lo = (1 << 32) - 100
    for idx in (0x00ffffffff, 0x0100000000):
        hits, n, st = _search(dprf, _planted(fam, idx), lo, 200)
        assert (hits, n, st["candidates"]) == ([idx], 1, 200), hex(idx)


@pytest.mark.parametrize("fam", FAMILIES)
def test_b_first_and_last_key(dprf, fam):
    hits, n, _ = _search(dprf, _planted(fam, 0), 0, 125)    # five 00 bytes
    assert (hits, n) == ([0], 1)
    hits, n, st = _search(dprf, _planted(fam, SPACE - 1), SPACE - 125, 125)   # ffffffffff
    assert (hits, n, st["candidates"]) == ([SPACE - 1], 1, 125)


@pytest.mark.parametrize("fam", FAMILIES)
def test_b_window_past_the_space_is_invalid_and_the_context_still_serves(dprf, fam):
    import ctypes
    idx = SPACE - 7
    with dprf.Context(_planted(fam, idx), device=0) as ctx:
        with pytest.raises(dprf.DprfError) as ei:
            ctx.search_key40(SPACE - 124, 125)              # start + count = 2^40 + 1: refused in Python
        assert ei.value.code == dprf.E_INVALID
        # ... and by the library itself, called past the Python check; a start + count that wraps 2^64 too
        L = dprf.lib()
        hits, nh, st = (ctypes.c_uint64 * 4)(), ctypes.c_int64(), dprf.Stats()
        for start, count in ((SPACE - 124, 125), (1, SPACE), ((1 << 64) - 1, 2)):
            rc = L.dprf_search_key40(ctx._h, start, count, 0, hits, 4, ctypes.byref(nh), ctypes.byref(st))
            assert rc == dprf.E_INVALID, (start, count)
            assert "2^40" in L.dprf_last_error().decode()
        assert L.dprf_search_key40(ctx._h, 0, 1, 0, hits, 4, None, ctypes.byref(st)) == dprf.E_INVALID   # null nhits
        assert ctx.search_key40(SPACE - 125, 125)[0] == [idx]


# ---------------------------------------------------------------- (c)
@pytest.mark.parametrize("fam", FAMILIES)
def test_c_every_lane_and_seam(dprf, fam):
    nbat = BATCHES[fam]
    wg = 64 * nbat
    start, count = 0x5100000123, 2 * wg + 37                # two full workgroups and a partial batch of 37 keys
    mid = 64 * (nbat // 2)
    offsets = [0, 63, mid, mid + 63, wg - 64, wg - 1, wg, wg + 63, 2 * wg - 1, 2 * wg, count - 1]
    for off in offsets:
        hits, n, st = _search(dprf, _planted(fam, start + off), start, count)
        assert (hits, n, st["candidates"]) == ([start + off], 1, count), off
    # the first key past the partial batch is not searched
    assert _search(dprf, _planted(fam, start + count), start, count)[0] == []


# ---------------------------------------------------------------- (d)
def _flip(hexfield, byte):
    b = bytearray(bytes.fromhex(hexfield))
    b[byte] ^= 0x10
    return b.hex()


@pytest.mark.parametrize("fam,field,compared", [
    ("pdf_r2", 9, range(4, 32)),        # after the 4-byte early reject: the full 32-byte compare
    ("pdf_r34", 9, range(2, 16)),       # after the 2-byte early reject: the full 16-byte compare
    ("office_md5", 4, range(0, 16)),    # every byte of encryptedVerifierHash
    ("office_sha1", 4, range(0, 20)),
])
def test_d_full_compare_rejects(dprf, fam, field, compared):
    idx = 0x77004bc3d1
    good = _planted(fam, idx)
    assert _search(dprf, good, idx - 10, 20)[0] == [idx]
    for byte in compared:
        bad = list(good)
        bad[field] = _flip(good[field], byte)
        assert not km.key_verifies(bad, km.key_bytes(idx))
        hits, n, st = _search(dprf, bad, idx - 10, 20)
        assert (hits, n, st["candidates"]) == ([], 0, 20), byte


@pytest.mark.parametrize("fam,byte", [("pdf_r2", 0), ("pdf_r2", 3), ("pdf_r34", 0), ("pdf_r34", 1)])
def test_d_prefilter_bytes_reject_too(dprf, fam, byte):
    idx = 0x77004bc3d1
    bad = _planted(fam, idx)
    bad[9] = _flip(bad[9], byte)
    assert _search(dprf, bad, idx - 10, 20)[0] == []


# ---------------------------------------------------------------- (e)
@pytest.mark.parametrize("fam", FAMILIES)
def test_e_a_megakey_window(dprf, fam):
    """2^20 keys with one planted: every reported index is re-verified by the model and the planted one is among them.
    Exactly one is expected; a larger set would be a finding."""
    start = 0x2b00000000 - (1 << 19) - 11
    idx = start + 777777
    fields = _planted(fam, idx)
    hits, n, st = _search(dprf, fields, start, 1 << 20)
    assert st["candidates"] == 1 << 20 and n == len(hits)
    for h in hits:
        assert km.key_verifies(fields, km.key_bytes(h)), hex(h)
    assert idx in hits
    assert hits == [idx]


# ---------------------------------------------------------------- (f)
@pytest.mark.parametrize("fam", FAMILIES)
def test_f_stop_on_first_and_two_lanes(dprf, fam):
    start, count = 0x0fedcba987, 8269
    idx = start + 6001                                      # in the second half
    fields = _planted(fam, idx)
    full, n, st = _search(dprf, fields, start, count)
    assert full == [idx] and st["candidates"] == count
    first, _, _ = _search(dprf, fields, start, count, stop_on_first=True, cap=1)
    assert first == [min(full)]
    with dprf.Context(fields, devices=[0, 0]) as ctx:
        hits, n, st = ctx.search_key40(start, count)
        assert hits == full and n == 1 and st["candidates"] == count and st["devices"] == 2
        lanes = ctx.last_call_devices()
        assert len(lanes) == 2 and all(d["launches"] >= 1 for d in lanes)
        assert sum(d["candidates"] for d in lanes) == count
        assert ctx.search_key40(start, count, stop_on_first=True, cap=1)[0] == [idx]


# ---------------------------------------------------------------- (g)
@pytest.mark.parametrize("label", ["pdf_r3_128", "pdf_r5", "pdf_r6", "oldoffice_4", "office_2007", "agile_2010", "odt",
                                   "odf"])
def test_g_refused_documents_still_serve_passwords(dprf, label):
    fields, pw, family, _ = doc_layer.case(label)
    with dprf.Context(fields, device=0) as ctx:
        assert ctx.kernel == family
        with pytest.raises(dprf.DprfError) as ei:
            ctx.search_key40(0, 64)
        assert ei.value.code == dprf.E_DOMAIN and "not a 40-bit document" in str(ei.value)
        hits, _, _ = ctx.verify_list(["no", pw, "nope"])
        assert hits == [1]


def test_g_owner_mode_finds_the_same_key(dprf):
    streams = load_golden("streams.json")
    vec = load_golden("key40_vectors.json")["streams"]
    for name in ("pdf_synth_r2_key", "pdf_synth_r3_l40_cab"):
        fields = km.fields_of(streams[name]["stream"])
        idx = vec[name]["index"]
        with dprf.Context(fields, device=0) as ctx:
            user = ctx.search_key40(idx - 100, 200)[0]
            ctx.set_pdf_password("owner")
            assert ctx.kernel == "pdf_r24_owner"            # dprf_ctx_kernel keeps naming the password family
            assert ctx.search_key40(idx - 100, 200)[0] == user == [idx]
            ctx.set_pdf_password("user")
            assert ctx.verify_list([streams[name]["password"]])[0] == [0]


def test_g_never_matching_context_makes_no_launch(dprf):
    fields = list(_base("pdf_r2"))
    fields[2] = "3"                                         # V 1 with R 3: the reference's verdict is constant
    with dprf.Context(fields, device=0) as ctx:
        assert ctx.flags & dprf.FLAG_NEVER_MATCHES
        hits, n, st = ctx.search_key40(0, 1 << 20)
        assert (hits, n) == ([], 0) and st["launches"] == 0 and st["candidates"] == 1 << 20


# ---------------------------------------------------------------- (h)
def _write(kind, path):
    import docgen
    import oldoffice_docgen
    pw = "Ux7"
    if kind == "pdf_r2":
        docgen.write_pdf(path, pw, seed=402, R=2, length=40)
        return "3", pw
    if kind == "pdf_r3_40":
        docgen.write_pdf(path, pw, seed=403, R=3, length=40)
        return "3", pw
    if kind == "doc_type1":
        oldoffice_docgen.write_doc(path, pw, 1, seed=401)
        return "1", pw
    oldoffice_docgen.write_xls(path, pw, 3, seed=404)
    return "1", pw


def _cli(argv):
    from dprf_amd import brute_force
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ret = brute_force.main(argv)
    return ret, out.getvalue()


def _document(kind, tmp_path):
    from dprf_amd import brute_force
    path = str(tmp_path / {"pdf_r2": "a.pdf", "pdf_r3_40": "b.pdf", "doc_type1": "c.doc", "xls_type3": "d.xls"}[kind])
    doc_type, pw = _write(kind, path)
    with contextlib.redirect_stdout(io.StringIO()):
        fields = list(brute_force.parse_verification_data(brute_force.get_verification_data(doc_type, path)))
    idx = km.key_index(km.key_of_password(fields, pw))
    lo = min(max(0, idx - 2048), SPACE - 4096)
    return doc_type, path, idx, "%010x-%010x" % (lo, lo + 4095)


@pytest.mark.parametrize("kind", ["pdf_r2", "pdf_r3_40", "doc_type1", "xls_type3"])
def test_h_cli_end_to_end(kind, tmp_path):
    from dprf_amd import key40
    doc_type, path, idx, window = _document(kind, tmp_path)
    ret, text = _cli([doc_type, path, "--key40", window, "--devices", "0"])
    assert ret == (1, "%010x" % idx)
    assert "Key found: %010x\n" % idx in text
    assert any(s in text for s in key40.SENTENCES.values())
    assert "of 2^40" in text
    # a window beside the key: nothing verifies
    lo = int(window[:10], 16)
    if lo >= 4096:
        ret, text = _cli([doc_type, path, "--key40", "%010x-%010x" % (lo - 4096, lo - 1), "--devices", "0"])
        assert ret == (0, "default_password_allocation") and "Key found" not in text


def test_h_cli_checkpoint_stop_and_resume(tmp_path, monkeypatch):
    from dprf_amd import brute_force
    doc_type, path, idx, window = _document("doc_type1", tmp_path)
    cursor = str(tmp_path / "cursor.json")
    argv = [doc_type, path, "--key40", window, "--devices", "0", "--checkpoint", cursor]
    # rounds of 1,024 keys until a rate is known; the run is interrupted after its first round (the key lies in the
    # third quarter of the window)
    monkeypatch.setattr(brute_force, "FIRST_ROUND", 1024)

    def stop(*a):
        raise KeyboardInterrupt
    monkeypatch.setattr(brute_force, "progress", stop)
    with pytest.raises(SystemExit) as ei:
        _cli(argv)
    assert ei.value.code == 0
    import json
    rec = json.load(open(cursor))
    lo = int(window[:10], 16)
    assert rec["search"] == "key40" and rec["window"] == [lo, lo + 4095]
    assert rec["next_index"] == lo + 1024 and rec["found"] is None
    monkeypatch.undo()
    ret, text = _cli(argv)
    assert ret == (1, "%010x" % idx) and "resuming at key %010x" % (lo + 1024) in text
    ret, text = _cli(argv)                                   # answered from the finished checkpoint
    assert ret == (1, "%010x" % idx) and "already finished" in text
    # the same file under another window is refused
    with pytest.raises(ValueError, match="different search"):
        _cli([doc_type, path, "--key40", "%010x-%010x" % (lo, lo + 4094), "--devices", "0", "--checkpoint", cursor])


def test_h_cli_refuses_a_128_bit_document_with_the_library_message(tmp_path):
    import docgen
    path = str(tmp_path / "e.pdf")
    docgen.write_pdf(path, "Ux7", seed=405, R=3, length=128)
    out = io.StringIO()
    with contextlib.redirect_stdout(out), pytest.raises(SystemExit) as ei:
        from dprf_amd import brute_force
        brute_force.main(["3", path, "--key40", "--devices", "0"])
    assert ei.value.code == 1
    assert "not a 40-bit document" in out.getvalue() and "Traceback" not in out.getvalue()
