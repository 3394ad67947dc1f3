"""Office 97-2003 RC4 / RC4 CryptoAPI on the device (k_oldoffice, kernel families "office_rc4_md5" and
"office_rc4_sha1") against tests/oldoffice_model.py, the Python statement of the definition, which
tests/test_oldoffice_model.py pins on the CPU (public vectors included).  Streams come from oldoffice_model.make_stream;
the shapes are the smallest at which this kernel can go wrong.  In types 0 / 1 only 40 bits of the first hash survive,
so the expected hit set of every test is what the model says, never "exactly one".

  (a) the two public vectors: the password among three near misses
  (b) every type: a 125-candidate range window (no multiple of 64), the whole hit set, and stop_on_first
  (c) window edges: 1, 63, 65, 257 and 513 candidates from a non-zero start, the password at either end
  (d) planted lengths in list mode: MD5's first message crosses to two blocks at 28 characters, SHA-1's at 20
  (e) non-ASCII candidates: list, symbol window, mask
  (f) dense hits: a 300-entry list with the password at eight positions; two and four lanes on one device
  (g) tampered streams, and the refusals, after each of which the context or the library still serves
  (h) hybrid and rule windows; dprf_spell_rules returns UTF-16LE slots
  (i) end to end from the .doc and .xls files of oldoffice_docgen: --mask, a wordlist, -pr with --checkpoint
  (j) the server and the GPU client; the 2007 and Agile streams are served as before"""
import contextlib
import functools
import io
import json
import os
import zlib

import pytest

import oldoffice_model as M
from conftest import load_golden

pytestmark = pytest.mark.gpu

FAMILY = {0: "office_rc4_md5", 1: "office_rc4_md5", 3: "office_rc4_sha1", 4: "office_rc4_sha1"}
CS5 = "678Ux"
PW = "Ux7"
PW_IDX = M.index_of(PW, CS5)
assert PW_IDX == 96 and M.word(PW_IDX, CS5, 3) == PW


@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device: GPU tests need the MI355X box"
    return _lib


def _fields(stream):
    from dprf_amd.brute_force import parse_verification_data
    with contextlib.redirect_stdout(io.StringIO()):
        return parse_verification_data(stream)


@functools.lru_cache(maxsize=None)
def _stream(pw, typ):
    """One stream per (password, type), made once and shared."""
    s = M.make_stream(pw, typ, seed=zlib.crc32(repr((pw, typ)).encode()))
    assert M.verifies(s, pw)
    return s


def _model_hits(s, words):
    return [k for k, w in enumerate(words) if M.verifies(s, w)]


# ---------------------------------------------------------------- (a) public vectors
@pytest.mark.parametrize("name", ["oldoffice_type1_hashcat", "oldoffice_type3_hashcat"])
def test_public_vectors(dprf, name):
    v = load_golden("oldoffice_vectors.json")[name]
    f = _fields(v["stream"])
    words = ["hashca", "hashcat", "hashcatx", "Hashcat"]
    assert _model_hits(f, words) == [1]
    with dprf.Context(f, device=0) as ctx:
        assert ctx.kernel == FAMILY[int(f[1])] and ctx.flags == 0 and ctx.format == dprf.FMT_OFFICE
        hits, n, st = ctx.verify_list(words)
        assert hits == [1] and n == 1 and st["candidates"] == 4


# ---------------------------------------------------------------- (b) range windows, every type
@pytest.mark.parametrize("typ", M.TYPES)
def test_range_window(dprf, typ):
    s = _stream(PW, typ)
    want = _model_hits(s, [M.word(k, CS5, 3) for k in range(125)])
    assert PW_IDX in want
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.kernel == FAMILY[typ] and ctx.flags == 0
        hits, n, st = ctx.search_range(CS5, 3, 0, 125)
        assert hits == want and n == len(want) and st["candidates"] == 125
        first, n1, _ = ctx.search_range(CS5, 3, 0, 125, stop_on_first=True, cap=1)
        assert first == [want[0]] and n1 >= 1


# ---------------------------------------------------------------- (c) window edges
@pytest.mark.parametrize("typ", [1, 4])
@pytest.mark.parametrize("count", [1, 63, 65, 257, 513])
def test_window_edges(dprf, typ, count):
    start = 1009                                            # 5^5 = 3125 candidates; 1009 + 513 stays inside
    for idx in sorted({start, start + count - 1}):
        pw = M.word(idx, CS5, 5)
        s = _stream(pw, typ)
        want = [k for k in range(start, start + count) if M.verifies(s, M.word(k, CS5, 5))]
        assert idx in want
        with dprf.Context(_fields(s), device=0) as ctx:
            hits, n, st = ctx.search_range(CS5, 5, start, count)
            assert hits == want and n == len(want) and st["candidates"] == count, (idx, hits)
            first, _, _ = ctx.search_range(CS5, 5, start, count, stop_on_first=True, cap=1)
            assert first == [hits[0]]
            # one candidate to either side of the password and the window misses it
            if idx == start and count > 1:
                assert idx not in ctx.search_range(CS5, 5, start + 1, count - 1)[0]
            if idx == start + count - 1 and count > 1:
                assert idx not in ctx.search_range(CS5, 5, start, count - 1)[0]


# ---------------------------------------------------------------- (d) planted lengths, list mode
def _planted(L):
    return "".join(chr(33 + (7 * k + 5 * L + k * k) % 90) for k in range(L))


LENGTHS = [(t, L) for t in (0, 1) for L in (1, 15, 16, 27, 28, 31, 32)] + \
          [(t, L) for t in (3, 4) for L in (1, 19, 20, 27, 28, 32)]


@pytest.mark.parametrize("typ,L", LENGTHS)
def test_planted_lengths(dprf, typ, L):
    pw = _planted(L)
    s = _stream(pw, typ)
    # decoys one character shorter and longer; the empty candidate (below 1) and a 33-character one (above the slot)
    # are refusals, tested in (g) -- at those ends a decoy of the same length with its last character changed stands in
    shorter = pw[:-1] if L > 1 else "~"
    longer = pw + "x" if L < 32 else pw[:-1] + "~"
    words = [shorter, longer, pw, pw[:-1] + "}"]
    want = _model_hits(s, words)
    assert 2 in want
    nbytes = 2 * L
    if typ in (0, 1):
        assert (nbytes > 55) == (L >= 28)                   # MD5(pw16): one block up to 27 characters, two from 28
    else:
        assert (16 + nbytes > 55) == (L >= 20)              # SHA1(salt || pw16): one block up to 19, two from 20
    with dprf.Context(_fields(s), device=0) as ctx:
        hits, n, _ = ctx.verify_list(words)
        assert hits == want and n == len(want)


# ---------------------------------------------------------------- (e) non-ASCII candidates
@pytest.mark.parametrize("typ", [0, 4])
def test_non_ascii_list(dprf, typ):
    words = ["été", "日本語", "\U0001F600ok", "ete", "日本", "ok"]      # a BMP character, a surrogate pair
    for k in range(3):
        s = _stream(words[k], typ)
        want = _model_hits(s, words)
        assert k in want
        with dprf.Context(_fields(s), device=0) as ctx:
            assert ctx.verify_list(words)[0] == want
            assert ctx.verify_list([w.encode("utf-8") for w in words])[0] == want


@pytest.mark.parametrize("typ", [1, 3])
def test_symbol_window_and_mask(dprf, typ):
    from dprf_amd import mask as masks
    charset = "aé\U0001F600"
    pw = "é\U0001F600a"
    idx = M.index_of(pw, charset)
    s = _stream(pw, typ)
    want = _model_hits(s, [M.word(k, charset, 3) for k in range(27)])
    assert idx in want
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.search_symbols(charset, 3, 0, 27)[0] == want
        assert ctx.search_symbols(charset, 3, idx, 1, stop_on_first=True, cap=1)[0] == [idx]
        assert ctx.search_symbols(charset, 3, 0, idx)[0] == [k for k in want if k < idx]
    positions = masks.parse_mask("U?1?d", ("xé",))
    assert masks.space(positions) == 20
    mpw = "Ué7"
    midx = masks.index_of(positions, mpw)
    assert midx == 17 and masks.word(positions, midx) == mpw
    s = _stream(mpw, typ)
    want = _model_hits(s, [masks.word(positions, k) for k in range(20)])
    assert midx in want
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.search_mask(positions, 0, 20)[0] == want


# ---------------------------------------------------------------- (f) dense hits; lanes on one device
AT = (0, 63, 64, 127, 128, 255, 256, 299)


@functools.lru_cache(maxsize=None)
def _dense(typ):
    s = _stream(PW, typ)
    words = [PW if k in AT else "d%03dy" % k for k in range(300)]
    want = _model_hits(s, words)
    assert set(AT) <= set(want)
    return s, words, want


@pytest.mark.parametrize("typ", M.TYPES)
@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0, 0]])
def test_dense_hits_and_lanes(dprf, typ, devices):
    s, words, want = _dense(typ)
    with dprf.Context(_fields(s), devices=devices) as ctx:
        hits, n, st = ctx.verify_list(words)
        assert hits == want and n == len(want) and st["candidates"] == 300
        first, _, _ = ctx.verify_list(words, stop_on_first=True, cap=1)
        assert first == [want[0]]
        assert [d["device"] for d in ctx.last_call_devices()] == devices
        if len(devices) > 1:
            rhits, _, rst = ctx.search_range(CS5, 3, 0, 125)
            assert PW_IDX in rhits and rst["candidates"] == 125 and all(M.verifies(s, M.word(k, CS5, 3)) for k in rhits)


# ---------------------------------------------------------------- (g) tampered streams and refusals
@pytest.mark.parametrize("typ", M.TYPES)
def test_tampered_streams(dprf, typ):
    base = _fields(_stream(PW, typ))
    n = 16 if typ < 2 else 20
    assert len(base[4]) == 2 * n
    cases = [(4, pos, (pos * 3) % 8) for pos in range(n)] + [(3, pos, (pos + 1) % 8) for pos in (0, 7, 15)] + \
            [(2, 0, 0), (2, 15, 7)]
    for k, pos, bit in cases:
        raw = bytearray(bytes.fromhex(base[k]))
        raw[pos] ^= 1 << bit
        f = list(base)
        f[k] = bytes(raw).hex()
        assert not M.verifies(f, PW)
        with dprf.Context(f, device=0) as ctx:
            hits, nh, st = ctx.verify_list([PW, "Ux8"])
            assert hits == [] and nh == 0 and st["candidates"] == 2, (k, pos, bit)
    with dprf.Context(base, device=0) as ctx:
        assert ctx.verify_list([PW, "Ux8"])[0] == [0]


def _serves(dprf, s):
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.verify_list([PW, "Ux8"])[0] == [0]


REFUSAL_TYPES = [1, 3]


def refusal_base(typ):
    """The stream the refused ones are made from, and its fields."""
    good = _stream(PW, typ)
    return good, _fields(good)


def bad_streams(base):
    """What is refused with DPRF_E_DOMAIN, as changes to `base`: (the field name the message carries, field index,
    value).  tests/test_doc_layer.py runs the same list through the document layer without a device."""
    return [
        ("type", 1, "2"), ("type", 1, "5"), ("type", 1, ""), ("type", 1, "01"),
        ("salt", 2, base[2][:30]), ("salt", 2, base[2] + "00"), ("salt", 2, "g" + base[2][1:]),
        ("encryptedVerifier", 3, base[3][:-2]), ("encryptedVerifier", 3, base[3] + "ab"),
        ("encryptedVerifier", 3, base[3][:5] + "x" + base[3][6:]),
        ("encryptedVerifierHash", 4, base[4][:-8]), ("encryptedVerifierHash", 4, base[4] + "00000000"),
        ("encryptedVerifierHash", 4, base[4][:-1] + "z"),
    ]


@pytest.mark.parametrize("typ", REFUSAL_TYPES)
def test_stream_refusals(dprf, typ):
    good, base = refusal_base(typ)
    bad = bad_streams(base)
    for name, k, v in bad:
        f = list(base)
        f[k] = v
        with pytest.raises(dprf.DprfError) as ei:
            dprf.Context(f, device=0)
        assert ei.value.code == dprf.E_DOMAIN, (name, v)
        assert name in str(ei.value), (name, str(ei.value))          # the message names the field
        _serves(dprf, good)
    for f in (base[:4], base + ["00"]):                              # a wrong field count is no oldoffice stream
        with pytest.raises(dprf.DprfError) as ei:
            dprf.Context(f, device=0)
        assert ei.value.code == dprf.E_INVALID
    # the hash length belongs to the type: 40 digits with type 1, 32 with type 3
    other = _fields(_stream(PW, 4 - typ))
    f = list(base)
    f[4] = other[4]
    with pytest.raises(dprf.DprfError) as ei:
        dprf.Context(f, device=0)
    assert ei.value.code == dprf.E_DOMAIN and "encryptedVerifierHash" in str(ei.value)
    _serves(dprf, good)


@pytest.mark.parametrize("typ", [0, 4])
def test_candidate_refusals(dprf, typ):
    import numpy as np
    s = _stream(PW, typ)
    words = [PW.encode(), b"y" * 33, b"z" * 32, b""]
    blob = b"".join(words)
    offs = np.cumsum([0] + [len(w) for w in words]).astype(np.uint64)
    with dprf.Context(_fields(s), device=0) as ctx:
        with pytest.raises(dprf.DprfError) as ei:
            ctx.verify_list(words[:3])
        assert ei.value.code == dprf.E_PWLEN and "not supported yet" in str(ei.value)
        assert list(ctx.list_status(blob, offs)) == [0, dprf.E_PWLEN, 0, dprf.E_DOMAIN]
        assert ctx.verify_list([words[0], words[2]])[0] == [0]                 # the context still serves
        with pytest.raises(dprf.DprfError) as ei:
            ctx.verify_list([PW, ""])
        assert ei.value.code == dprf.E_DOMAIN
        with pytest.raises(dprf.DprfError) as ei:
            ctx.verify_list([PW.encode(), b"\xff\xfe"])                        # invalid UTF-8
        assert ei.value.code == dprf.E_DOMAIN
        with pytest.raises(dprf.DprfError) as ei:
            ctx.search_range("aé".encode("utf-8"), 2, 0, 4)                    # Office: ASCII-only range charset
        assert ei.value.code == dprf.E_CHARSET
        with pytest.raises(dprf.DprfError) as ei:
            ctx.set_pdf_password("owner")                                      # not a PDF context
        assert ei.value.code == dprf.E_INVALID
        assert PW_IDX in ctx.search_range(CS5, 3, 0, 125)[0]


# ---------------------------------------------------------------- (h) hybrid and rule windows
@pytest.mark.parametrize("typ", [1, 3])
def test_hybrid_and_rules(dprf, typ):
    from dprf_amd import hybrid, rules as rulemod
    words = [b"winter", "été".encode("utf-8"), b"summer", b"x" * 31]
    positions, word_at = hybrid.parse_hybrid("?w?d")
    space = hybrid.space(len(words), positions)
    assert space == 40
    pw = "summer4"
    idx = hybrid.index_of(words, positions, word_at, pw.encode("utf-8"))
    assert idx == 24
    s = _stream(pw, typ)
    want = _model_hits(s, [hybrid.candidate(words, positions, word_at, k).decode("utf-8") for k in range(space)])
    assert idx in want
    with dprf.Context(_fields(s), device=0) as ctx:
        ctx.set_words(words)
        hits, n, st = ctx.search_hybrid(positions, word_at, 0, space)
        assert hits == want and st["candidates"] == space
        assert ctx.search_hybrid(positions, word_at, 3, space - 3, stop_on_first=True, cap=1)[0] == [want[0]]
    rules = [rulemod.parse_rule(":"), rulemod.parse_rule("c $1"), rulemod.parse_rule("u")]
    rspace = rulemod.space(len(words), len(rules))
    rpw = "Summer1"
    ridx = rulemod.index_of(words, rules, rpw, office=True)
    assert ridx == 2 * 3 + 1
    s = _stream(rpw, typ)
    cands = [rulemod.candidate(words, rules, k, office=True) for k in range(rspace)]
    want = _model_hits(s, [c.decode("utf-16-le") for c in cands])
    assert ridx in want
    with dprf.Context(_fields(s), device=0) as ctx:
        ctx.set_words(words)
        hits, n, st = ctx.search_rules(rules, 0, rspace)
        assert hits == want and st["candidates"] == rspace
        assert ctx.spell_rules(rules, 0, rspace) == cands                     # UTF-16LE slots
        # case functions touch ASCII letters only: "c" leaves the leading é as it is
        assert cands[ridx] == rpw.encode("utf-16-le") and cands[4] == "été1".encode("utf-16-le")


# ---------------------------------------------------------------- (i) end to end from a document
@pytest.mark.parametrize("kind,typ", [("doc", 1), ("xls", 3), ("doc", 4), ("xls", 0)])
def test_document_end_to_end(dprf, tmp_path, kind, typ):
    import oldoffice_docgen as G
    from dprf_amd import brute_force
    t = str(tmp_path)
    path = os.path.join(t, "old." + kind)
    want = (G.write_doc if kind == "doc" else G.write_xls)(path, PW, typ, 0xD0C + typ)
    with contextlib.redirect_stdout(io.StringIO()):
        assert brute_force.main(["1", path, "--mask", "U?l?d", "--devices", "0"]) == (1, PW)
        stream = brute_force.get_verification_data("1", path)
        assert stream == want
        fields = brute_force.parse_verification_data(stream)
        assert fields[:2] == ["oldoffice", str(typ)] and M.verifies(stream, PW)
        assert brute_force.init_listbased_brute_force(fields, ["Ux6", "ux7", PW, "Ux8"], devices=[0]) == (1, PW)
        assert brute_force.init_listbased_brute_force(fields, ["Ux6", "ux7"], devices=[0])[0] == 0
        wl = os.path.join(t, "words.txt")
        with open(wl, "w") as f:
            f.write("winter\nUx\nsummer\n")
        assert brute_force.main(["1", path, "--wordlist", wl, "--mask", "?w?d", "--devices", "0"]) == (1, PW)
        rl = os.path.join(t, "r.rule")
        with open(rl, "w") as f:
            f.write(":\nc $7\n")
        with open(wl, "w") as f:
            f.write("winter\nux\n")
        assert brute_force.main(["1", path, "--wordlist", wl, "--rules", rl, "--devices", "0"]) == (1, PW)
        # -pr / --charset with a checkpoint: the cursor file records the search and its result
        cp = os.path.join(t, "cursor.json")
        argv = ["1", path, "-pr", "3", "--charset", CS5, "--devices", "0", "--checkpoint", cp]
        assert brute_force.main(argv) == (1, PW)
        assert json.load(open(cp))["found"] == PW
        assert brute_force.main(argv) == (1, PW)                                # answered from the checkpoint
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert brute_force.main(["1", path, "--wordlist", wl, "--rules", rl, "--stdout", "--devices", "0"])[1] == 4
    assert out.getvalue().splitlines()[-4:] == ["winter", "Winter7", "ux", "Ux7"]


# ---------------------------------------------------------------- (j) server and client; the other families as before
def test_server_and_gpu_client(dprf):
    """The work-distribution pair on an $oldoffice$ stream: the server's payloads, verified by the GPU client."""
    import socket
    import threading
    from dprf_amd import client as cl, server as sv
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    hb = s.getsockname()[1]
    s.close()
    stream = _stream("ok", 3)
    srv = sv.Server(stream, password_range=2, payload_size=300, heartbeat_port=hb, quiet=True)
    out = {}
    th = threading.Thread(target=lambda: out.setdefault("pw", srv.run("127.0.0.1", 0)), daemon=True)
    th.start()
    assert srv.bound.wait(10)
    ver = cl.GpuVerifier([0])
    rc, pw = cl.connect_to_server("127.0.0.1", srv.address[1], "gpu", ver, quiet=True)
    ver.close()
    th.join(10)
    assert (rc, pw) == (0, "ok") and out["pw"] == "ok"


def test_other_office_streams_are_served_as_before(dprf, streams, hitsets):
    import agile_model
    for typ in M.TYPES:
        assert dprf.plan_chunk(FAMILY[typ], 0, 1, 1, 1, 0) != 0
    for family in ("office_std", "office_agile_sha1", "office_agile_sha512", "odf_aes256", "pdf_r24", "pdf_r5", "pdf_r6"):
        assert dprf.plan_chunk(family, 0, 1, 1, 1, 0) == 1, family
    h = hitsets["office_synth_ok/lower^2"]
    with dprf.Context(_fields(streams["office_synth_ok"]["stream"]), device=0) as ctx:
        assert ctx.kernel == "office_std" and ctx.format == dprf.FMT_OFFICE
        hits, _, st = ctx.search_range(h["charset"], h["pwlen"], h["start"], h["count"])
        assert hits == h["hits"] == [374] and st["candidates"] == 676
    a = agile_model.make_stream(PW, "2013", 256, 3, seed=11)
    with dprf.Context(_fields(a), device=0) as ctx:
        assert ctx.kernel == "office_agile_sha512"
        assert ctx.search_range(CS5, 3, 0, 125)[0] == [PW_IDX]
