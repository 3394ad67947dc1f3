"""ODF 1.0 / 1.1 (Blowfish-CFB, SHA-1) on the device (k_odf_bf_kdf + k_odf_bf_check, kernel family "odf_bf_sha1")
against tests/odf_legacy_model.py, the Python statement of the definition, which tests/test_odf_legacy_model.py pins on
the CPU.  Streams come from odf_legacy_model.make_stream; expected hit sets come from the model.  The shapes are the
smallest at which these kernels can go wrong; iterations are 1024 (the real value) only where noted.

  (a) iteration edges: 1 (no loop trip), 2, 3 and 1024, the password among near misses in a list
  (b) start-key padding edges: planted list candidates of 1, 55, 56, 63 and 64 bytes, and one with bytes >= 0x80
  (c) every lane of the check kernel: the password at every index of two full workgroups and a ragged tail, and at none
  (d) range windows from a non-zero start: 1, one short of, exactly and one past a check workgroup, no multiple of 64
  (e) dense hits; two and four lanes on one device
  (f) the rejecting direction: one bit changed in every checksum byte, content blocks, every iv byte, the salt
  (g) symbols, mask, hybrid, rules
  (h) refusals, after each of which the context or the library still serves
  (i) end to end from a docgen file: --mask, wordlist with rules, -pr with --checkpoint; server and GPU client"""
import contextlib
import functools
import io
import json
import os
import re
import zlib

import pytest

import odf_legacy_model as M
from conftest import REPO

pytestmark = pytest.mark.gpu

FAMILY = "odf_bf_sha1"
CS5 = "678Ux"
PW = "Ux7"
PW_IDX = M.index_of(PW, CS5)
assert PW_IDX == 96 and M.word(PW_IDX, CS5, 3) == PW
# candidates per workgroup of the check kernel and of the KDF kernel, from the kernel's own constants
_SRC = open(os.path.join(REPO, "dprf_amd", "csrc", "dprf_kernels_odf.hip")).read()
WG = int(re.search(r"#define ODF_BF_CANDS (\d+)", _SRC).group(1))
KDF_WG = int(re.search(r"#define ODF_KDF_THREADS (\d+)", _SRC).group(1))


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
def _stream(pw, iterations=2):
    """One stream per (password, iterations), made once and shared."""
    s = M.make_stream(pw, iterations, seed=zlib.crc32(repr((pw, iterations)).encode()))
    assert M.verifies(s, pw)
    return s


@functools.lru_cache(maxsize=None)
def _verifies(s, w):
    return M.verifies(s, w)


def _model_hits(s, words):
    return [k for k, w in enumerate(words) if _verifies(s, w)]


# ---------------------------------------------------------------- (a) iteration edges
@pytest.mark.parametrize("iterations", [1, 2, 3, 1024])
def test_iteration_edges(dprf, iterations):
    s = _stream(PW, iterations)
    words = ["Ux", "Ux8", PW, "ux7", "Ux77", ""]
    assert _model_hits(s, words) == [2]
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.kernel == FAMILY and ctx.flags == 0 and ctx.format == dprf.FMT_ODT
        hits, n, st = ctx.verify_list(words)
        assert hits == [2] and n == 1 and st["candidates"] == len(words)


# ---------------------------------------------------------------- (b) start-key padding edges
def _planted(L):
    return "".join(chr(33 + (7 * k + 5 * L + k * k) % 90) for k in range(L))


@pytest.mark.parametrize("L", [1, 55, 56, 63, 64])
def test_planted_lengths(dprf, L):
    pw = _planted(L)
    assert len(pw.encode()) == L
    s = _stream(pw)
    # a 65-byte candidate is a refusal (h): at 64 a decoy of the same length with another last byte stands in
    shorter = pw[:-1] if L > 1 else "~"
    longer = pw + "x" if L < 64 else pw[:-1] + "~"
    words = [shorter, longer, pw, pw[:-1] + "}"]
    assert _model_hits(s, words) == [2]
    with dprf.Context(_fields(s), device=0) as ctx:
        hits, n, _ = ctx.verify_list(words)
        assert hits == [2] and n == 1


def test_high_bytes(dprf):
    words = ["pässwörd", "passwort", "pässwört", "日本語", "\U0001F600ok", b"\xff\xfe\x80"]
    for k in (0, 3, 4, 5):
        s = _stream(words[k])
        assert _model_hits(s, words) == [k]
        with dprf.Context(_fields(s), device=0) as ctx:
            assert ctx.verify_list(words)[0] == [k]


# ---------------------------------------------------------------- (c) every lane of the check kernel
def test_every_lane_hits_and_none_does(dprf):
    n = 2 * WG + WG // 2 + 3                                  # two full check workgroups and a ragged tail
    s = _stream(PW)
    assert _verifies(s, PW) and not _verifies(s, "Ux8")
    with dprf.Context(_fields(s), device=0) as ctx:
        hits, nh, st = ctx.verify_list([PW] * n)
        assert hits == list(range(n)) and nh == n and st["candidates"] == n
        hits, nh, st = ctx.verify_list(["Ux8"] * n)
        assert hits == [] and nh == 0 and st["candidates"] == n
        for at in (0, WG - 1, WG, 2 * WG - 1, 2 * WG, n - 1):  # one lane alone, at each edge of the shape
            assert ctx.verify_list([PW if k == at else "Ux8" for k in range(n)])[0] == [at]


# ---------------------------------------------------------------- (d) range windows
@pytest.mark.parametrize("count", [1, WG - 1, WG, WG + 1, 100, KDF_WG + 1])
def test_window_edges(dprf, count):
    start = 1009                                              # 5^5 = 3125 candidates; 1009 + 257 stays inside
    for idx in sorted({start, start + count - 1}):
        pw = M.word(idx, CS5, 5)
        s = _stream(pw)
        with dprf.Context(_fields(s), device=0) as ctx:
            hits, n, st = ctx.search_range(CS5, 5, start, count)
            assert hits == [idx] and n == 1 and st["candidates"] == count, (idx, hits)
            assert ctx.search_range(CS5, 5, start, count, stop_on_first=True, cap=1)[0] == [idx]
            # one candidate to either side of the password and the window misses it
            if idx == start and count > 1:
                assert ctx.search_range(CS5, 5, start + 1, count - 1)[0] == []
            if idx == start + count - 1 and count > 1:
                assert ctx.search_range(CS5, 5, start, count - 1)[0] == []


def test_range_window_against_the_model(dprf):
    s = _stream(PW)
    want = _model_hits(s, [M.word(k, CS5, 3) for k in range(125)])
    assert want == [PW_IDX]
    with dprf.Context(_fields(s), device=0) as ctx:
        hits, n, st = ctx.search_range(CS5, 3, 0, 125)
        assert hits == want and n == 1 and st["candidates"] == 125


def test_stop_on_first_returns_the_lowest(dprf):
    s = _stream(PW)
    words = [PW if k in (70, 71, 200, 299) else "d%03dy" % k for k in range(300)]
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.verify_list(words, stop_on_first=True, cap=1)[0] == [70]
        assert ctx.verify_list(words)[0] == [70, 71, 200, 299]


# ---------------------------------------------------------------- (e) dense hits; lanes on one device
AT = (0, 63, 64, 127, 128, 255, 256, 299)


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]])
def test_dense_hits_and_lanes(dprf, devices):
    s = _stream(PW)
    words = [PW if k in AT else "d%03dy" % k for k in range(300)]
    assert not _verifies(s, "d001y")
    with dprf.Context(_fields(s), devices=devices) as ctx:
        hits, n, st = ctx.verify_list(words)
        assert hits == list(AT) and n == len(AT) and st["candidates"] == 300
        assert ctx.verify_list(words, stop_on_first=True, cap=1)[0] == [0]
        assert [d["device"] for d in ctx.last_call_devices()] == devices
        rhits, _, rst = ctx.search_range(CS5, 3, 0, 125)
        assert rhits == [PW_IDX] and rst["candidates"] == 125


# ---------------------------------------------------------------- (f) the rejecting direction
def _flip(hexfield, pos, bit):
    raw = bytearray(bytes.fromhex(hexfield))
    raw[pos] ^= 1 << bit
    return bytes(raw).hex()


def test_tampered_streams(dprf):
    base = _fields(_stream(PW))
    CK, IV, SALT, CONTENT = 5, 7, 9, 11
    cases = [(CK, pos, (pos * 3) % 8) for pos in range(20)]                          # every checksum byte: all 5 words
    cases += [(CONTENT, 8 * blk + blk % 8, blk % 8) for blk in (0, 1, 63, 64, 126, 127)]
    cases += [(CONTENT, 64 * b + 8 * ((3 * b) % 8) + b % 8, (b + 5) % 8) for b in range(16)]   # each SHA-1 message block
    cases += [(IV, pos, (pos + 1) % 8) for pos in range(8)]
    cases += [(SALT, 0, 0), (SALT, 15, 7)]
    for k, pos, bit in cases:
        f = list(base)
        f[k] = _flip(base[k], pos, bit)
        assert not M.verifies("$odf$*" + "*".join(f[1:]), PW), (k, pos, bit)
        with dprf.Context(f, device=0) as ctx:
            hits, nh, st = ctx.verify_list([PW, "Ux8"])
            assert hits == [] and nh == 0 and st["candidates"] == 2, (k, pos, bit)
        with dprf.Context(base, device=0) as ctx:
            assert ctx.verify_list([PW, "Ux8"])[0] == [0]


# ---------------------------------------------------------------- (g) every search mode once
def test_symbol_window_and_mask(dprf):
    from dprf_amd import mask as masks
    charset = "aé\U0001F600"
    pw = "é\U0001F600a"
    idx = M.index_of(pw, charset)
    s = _stream(pw)
    want = _model_hits(s, [M.word(k, charset, 3) for k in range(27)])
    assert want == [idx]
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.search_symbols(charset, 3, 0, 27)[0] == want
        assert ctx.search_symbols(charset, 3, idx, 1, stop_on_first=True, cap=1)[0] == [idx]
        assert ctx.search_symbols(charset, 3, 0, idx)[0] == []
    positions = masks.parse_mask("U?1?d", ("xé",))
    assert masks.space(positions) == 20
    mpw = "Ué7"
    midx = masks.index_of(positions, mpw)
    assert midx == 17 and masks.word(positions, midx) == mpw
    s = _stream(mpw)
    assert _model_hits(s, [masks.word(positions, k) for k in range(20)]) == [midx]
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.search_mask(positions, 0, 20)[0] == [midx]


def test_hybrid_and_rules(dprf):
    from dprf_amd import hybrid, rules as rulemod
    words = [b"winter", "été".encode("utf-8"), b"summer", b"x" * 63]
    positions, word_at = hybrid.parse_hybrid("?w?d")
    space = hybrid.space(len(words), positions)
    assert space == 40
    pw = "summer4"
    idx = hybrid.index_of(words, positions, word_at, pw.encode("utf-8"))
    assert idx == 24
    s = _stream(pw)
    assert _model_hits(s, [hybrid.candidate(words, positions, word_at, k) for k in range(space)]) == [idx]
    with dprf.Context(_fields(s), device=0) as ctx:
        ctx.set_words(words)
        hits, n, st = ctx.search_hybrid(positions, word_at, 0, space)
        assert hits == [idx] and st["candidates"] == space
        assert ctx.search_hybrid(positions, word_at, 3, space - 3, stop_on_first=True, cap=1)[0] == [idx]
    rules = [rulemod.parse_rule(":"), rulemod.parse_rule("c $1"), rulemod.parse_rule("u")]
    rspace = rulemod.space(len(words), len(rules))
    rpw = "Summer1"
    ridx = rulemod.index_of(words, rules, rpw.encode())
    assert ridx == 2 * 3 + 1
    s = _stream(rpw)
    cands = [rulemod.candidate(words, rules, k) for k in range(rspace)]
    assert _model_hits(s, cands) == [ridx]
    with dprf.Context(_fields(s), device=0) as ctx:
        ctx.set_words(words)
        hits, n, st = ctx.search_rules(rules, 0, rspace)
        assert hits == [ridx] and st["candidates"] == rspace
        assert ctx.spell_rules(rules, 0, rspace) == cands                      # byte slots, as for the $odt$ stream
        assert cands[ridx] == rpw.encode() and cands[4] == "été1".encode("utf-8")


# ---------------------------------------------------------------- (h) refusals
def _serves(dprf, s):
    with dprf.Context(_fields(s), device=0) as ctx:
        assert ctx.verify_list([PW, "Ux8"])[0] == [0]


def refusal_base():
    """The stream the refused ones are made from, and its fields."""
    good = _stream(PW)
    return good, _fields(good)


def bad_streams(base):
    """What is refused with DPRF_E_DOMAIN, as changes to `base`: (what the message carries, then field index and value,
    once or twice).  tests/test_doc_layer.py runs the same list through the document layer without a device."""
    return [
        ("cipher", 1, "2"), ("$odt$", 1, "1", 2, "1"), ("checksum type", 2, "1"), ("key size", 4, "32"),
        ("iv length", 6, "16"), ("salt length", 8, "32"), ("inplace", 10, "1"),
        ("iterations", 3, "0"), ("iterations", 3, "10000001"), ("iterations", 3, ""), ("iterations", 3, "1k"),
        ("iterations", 3, "-5"),
        ("checksum", 5, base[5][:-2]), ("checksum", 5, base[5] + "00"), ("checksum", 5, "g" + base[5][1:]),
        ("iv", 7, base[7][:-2]), ("iv", 7, base[7][:5] + "x" + base[7][6:]),
        ("salt", 9, base[9] + "ab"), ("salt", 9, base[9][:-1] + "z"),
        ("content", 11, base[11][:-16]), ("content", 11, base[11] + "00"), ("content", 11, base[11][:100] + "q" + base[11][101:]),
    ]


def test_stream_refusals(dprf):
    good, base = refusal_base()
    bad = bad_streams(base)
    for name, *changes in bad:
        f = list(base)
        for k, v in zip(changes[0::2], changes[1::2]):
            f[k] = v
        with pytest.raises(dprf.DprfError) as ei:
            dprf.Context(f, device=0)
        assert ei.value.code == dprf.E_DOMAIN, (name, changes)
        assert name in str(ei.value), (name, str(ei.value))                   # the message names the field
        _serves(dprf, good)
    for f in (base[:11], base + ["00"]):                                       # a wrong field count is no odf stream
        with pytest.raises(dprf.DprfError) as ei:
            dprf.Context(f, device=0)
        assert ei.value.code == dprf.E_INVALID
    _serves(dprf, good)


def test_candidate_refusals(dprf):
    import numpy as np
    s = _stream(PW)
    words = [PW.encode(), b"y" * 65, b"z" * 64, b"a\0b"]
    blob = b"".join(words)
    offs = np.cumsum([0] + [len(w) for w in words]).astype(np.uint64)
    with dprf.Context(_fields(s), device=0) as ctx:
        with pytest.raises(dprf.DprfError) as ei:
            ctx.verify_list(words[:3])
        assert ei.value.code == dprf.E_PWLEN and "not supported yet" in str(ei.value) and "ODF 1.0/1.1" in str(ei.value)
        assert list(ctx.list_status(blob, offs)) == [0, dprf.E_PWLEN, 0, dprf.E_INVALID]
        assert ctx.verify_list([words[0], words[2]])[0] == [0]                  # the context still serves
        with pytest.raises(dprf.DprfError) as ei:
            ctx.set_pdf_password("owner")                                       # not a PDF context
        assert ei.value.code == dprf.E_INVALID
        assert ctx.search_range(CS5, 3, 0, 125)[0] == [PW_IDX]


# ---------------------------------------------------------------- (i) end to end from a document
def test_document_end_to_end(dprf, tmp_path):
    import odf_legacy_docgen as G
    from dprf_amd import brute_force
    t = str(tmp_path)
    path = os.path.join(t, "old.odt")
    G.write_odf11(path, PW, seed=0x0DF)                                         # iteration-count 1024
    with contextlib.redirect_stdout(io.StringIO()):
        assert brute_force.main(["2", path, "--mask", "U?l?d", "--devices", "0"]) == (1, PW)
        stream = brute_force.get_verification_data("2", path)
        fields = brute_force.parse_verification_data(stream)
        assert fields[:5] == ["odf", "0", "0", "1024", "16"] and M.verifies(stream, PW)
        assert brute_force.init_listbased_brute_force(fields, ["Ux6", "ux7", PW, "Ux8"], devices=[0]) == (1, PW)
        assert brute_force.init_listbased_brute_force(fields, ["Ux6", "ux7"], devices=[0])[0] == 0
        wl = os.path.join(t, "words.txt")
        with open(wl, "w") as f:
            f.write("winter\nUx\nsummer\n")
        assert brute_force.main(["2", path, "--wordlist", wl, "--mask", "?w?d", "--devices", "0"]) == (1, PW)
        rl = os.path.join(t, "r.rule")
        with open(rl, "w") as f:
            f.write(":\nc $7\n")
        with open(wl, "w") as f:
            f.write("winter\nux\n")
        assert brute_force.main(["2", path, "--wordlist", wl, "--rules", rl, "--devices", "0"]) == (1, PW)
        # -pr / --charset with a checkpoint: the cursor file records the search and its result
        cp = os.path.join(t, "cursor.json")
        argv = ["2", path, "-pr", "3", "--charset", CS5, "--devices", "0", "--checkpoint", cp]
        assert brute_force.main(argv) == (1, PW)
        assert json.load(open(cp))["found"] == PW
        assert brute_force.main(argv) == (1, PW)                                # answered from the checkpoint
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert brute_force.main(["2", path, "--wordlist", wl, "--rules", rl, "--stdout", "--devices", "0"])[1] == 4
    assert out.getvalue().splitlines()[-4:] == ["winter", "Winter7", "ux", "Ux7"]


def _serve(stream, want):
    import socket
    import threading
    from dprf_amd import client as cl, server as sv
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    hb = s.getsockname()[1]
    s.close()
    srv = sv.Server(stream, password_range=2, payload_size=300, heartbeat_port=hb, quiet=True)
    out = {}
    th = threading.Thread(target=lambda: out.setdefault("pw", srv.run("127.0.0.1", 0)), daemon=True)
    th.start()
    assert srv.bound.wait(10)
    ver = cl.GpuVerifier([0])
    rc, pw = cl.connect_to_server("127.0.0.1", srv.address[1], "gpu", ver, quiet=True)
    ver.close()
    th.join(10)
    assert (rc, pw) == (0, want) and out["pw"] == want


def test_server_and_gpu_client(dprf):
    """The work-distribution pair on an $odf$ stream: the server's payloads, verified by the GPU client."""
    _serve("old.odt:" + _stream("ok", 1024), "ok")


def test_odf_1_2_stream_is_served_as_before(dprf, tmp_path, streams, hitsets):
    import docgen
    from dprf_amd.parsers import odt2hashes
    assert dprf.plan_chunk(FAMILY, 0, 1, 1, 1, 0) == 1
    for family in ("office_std", "odf_aes256", "pdf_r24", "pdf_r5", "pdf_r6", "office_rc4_md5"):
        assert dprf.plan_chunk(family, 0, 1, 1, 1, 0) == 1, family
    path = os.path.join(str(tmp_path), "new.odt")
    docgen.write_odt(path, "ok", 21)
    stream = odt2hashes.get_hashes(path)
    with dprf.Context(_fields(stream), device=0) as ctx:
        assert ctx.kernel == "odf_aes256" and ctx.format == dprf.FMT_ODT
        assert ctx.verify_list(["ok", "ko"])[0] == [0]
    _serve(stream, "ok")
